"""Stream order of every stream-taking entry point of include/range_hip.h, on a stream that is busy (`-m gpu`).

Every case goes through the staged-call harness of tests/stream_order.py: the call is issued on a fresh stream
behind a running delay kernel, with its inputs copied in behind that delay and decoys copied back behind the call,
then issued a second time back to back.  The first result has to be the bits of the default-stream reference on the
real batch, the second those on the decoy batch, and - for every call the header does not state as synchronising -
the delay has to be still running when both calls have returned to the host.

The shapes are the smallest that take each route (encoder: one persistent launch, 33 .. 128 tiles, separate split
launches, main launch plus split tail, 16-query workgroups; forward: one pass, one launch per pass, chunks with
pass 1 of the next chunk on the context's auxiliary stream, the stream-K walk, sharp temperatures, bf16 planes).
Then: a cold start (the first call a context ever sees is the staged one), two contexts interleaved on two streams,
the harness's own control, and a coverage check that parses the five public headers - it needs no GPU - so that a
new entry point with a ``range_stream_t`` parameter and no case fails the suite."""
import functools
import os

import numpy as np
import pytest
import torch

import stream_order as SO
from range_amd import _native, posenc
from range_amd._native import _check
from stream_order import Case

gpu = pytest.mark.gpu
DEV = "cuda:0"
L = 10
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
RANGE, PLUS = _native.MODEL_RANGE, _native.MODEL_RANGE_PLUS
MODELS = ((RANGE, 1.0), (PLUS, 0.5))
TAU = (12.0, 40.0)
N_BANK = 4100
CHUNK1 = (("RANGE_FWD_OVERLAP", "1"), ("RANGE_P2_STREAMK", "0"))
CHUNK2 = (("RANGE_FWD_OVERLAP", "2"), ("RANGE_P2_STREAMK", "0"))
UNFUSED = (("RANGE_TOPKS_FUSED", "0"),)


#: entry points with a range_stream_t parameter that no staged case can judge, and why
NO_STAGED_CASE = {
    "range_debug_raise_async_error": "test hook; the header states its stream as unused, and what it arms is a give-up path",
}


# ---------------------------------------------------------------------------------------------- contexts and batches
def _new_engine(H=128, N=N_BANK, env=(), pv="exact", taus=None, seed=31):
    from tools import synth
    old = {k: os.environ.get(k) for k, _ in env}
    os.environ.update(dict(env))
    try:
        eng = _native.HipEngine(DEV)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    w = synth.make_encoder_weights(L, H, 256, 2, 5)
    eng.set_encoder(L, H, 2, 256, _native.SH_ANALYTIC, [w["layers.0.weight"], w["layers.1.weight"], w["last_layer.weight"]],
                    [w["layers.0.bias"], w["layers.1.bias"], w["last_layer.bias"]])
    if N:
        bank = _bank(N, seed)
        eng.set_bank(bank.keys, bank.values, bank.xyz, 0)
    if pv != "exact":
        eng.set_pv_mode(pv)
    if taus:
        eng.set_temperatures(*taus)
    return eng


_engine = functools.lru_cache(maxsize=None)(_new_engine)


@functools.lru_cache(maxsize=None)
def _bank(N, seed):
    from range_amd.bank import prepare_bank
    from tools import synth
    return prepare_bank(*synth.make_bank(N, seed))


def _q(B, seed):
    from tools import synth
    return torch.from_numpy(synth.make_queries(B, seed=seed, lat_max=90.0)).to(DEV)


def _pair(B):
    """The real and the decoy batch of B locations."""
    return _q(B, 1000 + B), _q(B, 2000 + B)


@functools.lru_cache(maxsize=None)
def _encoded(B):
    """(e64, e32, xq, stats at TAU) of both batches of B locations, from the shared context, synchronised."""
    eng = _engine()
    out = []
    for x in _pair(B):
        e64, e32, xq = eng.encode(x)
        out.append((e64, e32, xq, eng.scan_stats(e32, xq, *TAU)))
    torch.cuda.synchronize()
    return out


def _rand(shape, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64).to(dtype).to(DEV)


# ---------------------------------------------------------------------------------------------- the case tables
def _encode_case(H, B, raw):
    def build():
        eng = _engine(H=H, N=0)
        return _pair(B)[:1], _pair(B)[1:], (lambda x: (eng.encode_raw(x),)) if raw else (lambda x: eng.encode(x))
    fn = "range_encode_raw" if raw else "range_encode"
    return Case(f"{fn[6:]}_H{H}_B{B}", (fn,), build)


def _features_cases():
    def coord():
        eng = _engine(N=0)
        return _pair(300)[:1], _pair(300)[1:], lambda x: tuple(eng.coord_features(x, m) for m in _native.COORD_DIMS)

    def pos():
        eng = _engine(N=0)
        freq = posenc.freq_list("s2vec_spheremplus")
        return _pair(300)[:1], _pair(300)[1:], lambda x: (eng.posenc_features(x, posenc.KIND_SPHEREMPLUS, freq),)
    return [Case("coord_features", ("range_coord_features",), coord), Case("posenc_features", ("range_posenc_features",), pos)]


def _pass_cases():
    B = 130

    def io(*cols):
        (ra, de) = _encoded(B)
        return tuple(ra[c] for c in cols), tuple(de[c] for c in cols)

    def scan(**kw):
        def build():
            eng = _engine()

            def call(e32, xq):
                out = eng.scan_stats(e32, xq, *TAU, **kw)
                return out if isinstance(out, tuple) else (out,)
            return (*io(1, 2), call)
        return build

    def scan_at():
        eng = _engine()
        ns = eng.p1_splits(B)

        def call(e32, xq):
            a = eng.scan_stats_at(e32[:64], xq[:64], *TAU, 0, B, ns)
            b = eng.scan_stats_at(e32[64:], xq[64:], *TAU, 64, B, ns)
            st = torch.cat([a, b])
            return a, b, eng.attend_kept(0, xq, *TAU, 0.5, st)
        return (*io(1, 2), call)

    def kept(first):
        def build():
            eng = _engine()

            def call(e32, xq):
                st = eng.scan_stats(e32, xq, *TAU, keep_logits=True)
                return st, eng.attend_kept(first, xq[first:], *TAU, 0.5, st[first:])
            return (*io(1, 2), call)
        return build

    def stats_kept():
        eng = _engine()

        def call(e32, xq):
            eng.scan_stats(e32, xq, *TAU, keep_logits=True)
            return eng.stats_kept(0, xq, [TAU, (50.0, 0.0), (15.0, 0.0)]), eng.stats_kept(64, xq[64:], [(15.0, 30.0)])
        return (*io(1, 2), call)

    def attend():
        eng = _engine()
        return (*io(1, 2, 3), lambda e32, xq, st: (eng.attend(e32, xq, *TAU, 0.5, st),))

    def attend_diag():
        eng = _engine()

        def call(e32, xq, st):
            eng.attend_diag(e32, xq, *TAU, 0.5, st)          # (cycle counts: not compared; the launch shares the slabs)
            return (eng.attend(e32, xq, *TAU, 0.5, st),)
        return (*io(1, 2, 3), call)
    return [Case("scan_stats", ("range_scan_stats",), scan()),
            Case("scan_stats_topk4", ("range_scan_stats",), scan(topk=4)),
            Case("scan_stats_keep_attend_kept", ("range_scan_stats", "range_attend_kept"), kept(0)),
            Case("attend_kept_from_query_64", ("range_scan_stats", "range_attend_kept"), kept(64)),
            Case("scan_stats_at_two_chunks", ("range_scan_stats_at", "range_attend_kept"), scan_at),
            Case("stats_kept", ("range_scan_stats", "range_stats_kept"), stats_kept),
            Case("attend", ("range_attend",), attend),
            Case("attend_diag_then_attend", ("range_attend_diag", "range_attend"), attend_diag)]


def _glue_cases():
    B = 130

    def merge_stats():
        eng = _engine()
        (ra, de) = _encoded(B)
        return (torch.stack([ra[3], de[3]]),), (torch.stack([de[3], de[3]]),), lambda p: (eng.merge_stats(p),)

    def merge_topk():
        eng = _engine()
        lists = []
        for enc in _encoded(B):
            _, tv, ti = eng.scan_stats(enc[1], enc[2], *TAU, topk=4)
            lists.append((tv, ti))
        torch.cuda.synchronize()
        (va, ia), (vb, ib) = lists
        real = (torch.stack([va, vb]), torch.stack([ia, ib + N_BANK]))
        decoy = (torch.stack([vb, vb]), torch.stack([ib, ib + N_BANK]))       # (the merge is symmetric in its parts)
        return real, decoy, lambda v, i: eng.merge_topk(v, i)

    def finalize():
        eng = _engine()
        (ra, de) = _encoded(B)
        real = (torch.stack([_rand((B, 1024), 1), _rand((B, 1024), 2)]), ra[0])
        decoy = (torch.stack([_rand((B, 1024), 3), _rand((B, 1024), 4)]), de[0])
        return real, decoy, lambda p, e64: (eng.finalize(p, e64),)

    def blend():
        eng = _engine()
        real, decoy = (_rand((B, 1024), 5), _rand((B, 1024), 6)), (_rand((B, 1024), 7), _rand((B, 1024), 8))
        return real, decoy, lambda G, H: (eng.blend(G, H, 0.25),)
    return [Case("merge_stats", ("range_merge_stats",), merge_stats), Case("merge_topk", ("range_merge_topk",), merge_topk),
            Case("finalize", ("range_finalize",), finalize), Case("blend", ("range_blend",), blend)]


def _topk_case(B, N, env):
    def build():
        eng = _engine(N=N, env=env) if env or N != N_BANK else _engine()
        real, decoy = ((_engine(N=0).encode(x)[1],) for x in _pair(B))
        torch.cuda.synchronize()
        return real, decoy, lambda e32: eng.topk_stream(e32, 5)
    return Case(f"topk_stream_B{B}_N{N}" + ("_unfused" if env else ""), ("range_topk_stream",), build)


def _topk_more_cases():
    def last():
        eng = _engine()
        real, decoy = _pair(130)

        def call(x):
            out = eng.forward(x, PLUS, 0.5)
            return (out, *eng.topk_last(130, 4))
        return (real,), (decoy,), call

    def timed():
        eng = _engine()
        real, decoy = ((_engine(N=0).encode(x)[1],) for x in _pair(8))
        torch.cuda.synchronize()

        def call(e32):
            eng.stream_read_timed(False, 1, 2)               # (a time only: nothing to compare)
            tv, ti, _ = eng.topk_stream_timed(e32, 5, repeats=2)
            return tv, ti
        return real, decoy, call
    return [Case("topk_last_behind_forward", ("range_forward", "range_topk_last"), last),
            Case("topk_stream_timed", ("range_topk_stream_timed", "range_stream_read_timed"), timed, blocks=True)]


def _forward_case(tag, B, model, beta, **engine_kw):
    def build():
        eng = _engine(**engine_kw)
        real, decoy = _pair(B)
        return (real,), (decoy,), lambda x: (eng.forward(x, model, beta),)
    return Case(f"forward_{tag}_B{B}_model{model}", ("range_forward",), build)


FORWARD_ROUTES = (("one_pass", 5, {}), ("one_launch_per_pass", 130, dict(env=(("RANGE_FWD_OVERLAP", "0"),))),
                  ("chunks_of_1", 130, dict(env=CHUNK1)), ("chunks_of_2", 337, dict(env=CHUNK2)), ("stream_k", 130, {}),
                  ("sharp", 130, dict(taus=(100.0, 40.0))), ("bf16x3", 130, dict(pv="bf16x3")))


def _forward_host_case(B, model, beta):
    def build():
        eng = _engine()
        real, decoy = _pair(B)
        return (real,), (decoy,), lambda x: (torch.from_numpy(eng.forward_host(x, model, beta)),)
    return Case(f"forward_host_B{B}_model{model}", ("range_forward_host",), build, blocks=True)


def _flag_case():
    """range_async_error_flag reads no caller input: what orders is its WRITE.  The slot it writes is first filled from
    the input on the caller's stream; a write that ran ahead of that stream is overwritten by the fill."""
    def build():
        eng = _engine(N=0)
        real, decoy = (torch.full((1,), 7.0, dtype=torch.float64, device=DEV),), (torch.full((1,), 3.0, dtype=torch.float64, device=DEV),)

        def call(x):
            slot = x.clone()
            eng.async_error_flag(out=slot)
            return (torch.cat([slot, x]),)                   # [0.0 - nothing gave up -, the input]
        return real, decoy, call
    return Case("async_error_flag", ("range_async_error_flag",), build)


@functools.lru_cache(maxsize=None)
def _csp():
    import csp_head_refs as H
    import csp_refs as R
    from range_amd import csp
    enc_golden, head_golden = (np.load(os.path.join(GOLDEN, f)) for f in ("csp_encoders.npz", "csp_head.npz"))
    head = H.case_head(enc_golden, head_golden, "theory")
    net = R.case_network(enc_golden, head["enc_case"])
    eng = _native.HipEngine(DEV)
    kind = {"gridcell": posenc.KIND_GRID, "theory": posenc.KIND_THEORY}[net["spa_enc_type"]]
    eng.set_csp(kind, net["freq_list"], [w.shape[0] for w in net["weights"]], net["weights"], net["biases"], net["ln_gamma"],
                net["ln_beta"], csp.ACTIVATIONS[net["act"]], net["skip"], net["use_layn"])
    eng.set_csp_head(head["W"])
    return eng


def _csp_cases():
    B = 150

    def locs():
        from tools import synth
        return tuple(torch.from_numpy(synth.make_queries(B, seed=s, lat_max=89.9)).to(DEV) for s in (96, 97))

    def extras():
        eng = _csp()
        C_ = eng.csp_classes
        g = torch.Generator().manual_seed(5)
        labels = [torch.randint(0, C_, (B,), generator=g, dtype=torch.int32).to(DEV) for _ in range(2)]
        img = [torch.rand((B, C_), generator=g, dtype=torch.float32).to(DEV) for _ in range(2)]
        feats = [eng.csp_encode(x) for x in locs()]
        torch.cuda.synchronize()
        return labels, img, feats

    def encode():
        eng = _csp()
        width = eng.lib.range_csp_width(eng._h)

        def call(x):
            plain = eng._empty((B, width), torch.float32)
            _check(eng.lib, eng.lib.range_csp_encode(eng._h, x.data_ptr(), B, plain.data_ptr(), eng._stream()))
            return plain, eng.csp_encode(x, max_grid=2)
        real, decoy = locs()
        return (real,), (decoy,), call

    def head():
        eng = _csp()
        ids = torch.tensor([7, 0, 32, 7], dtype=torch.int32, device=DEV)
        _, _, feats = extras()

        def call(f):
            plain = eng._empty((B, 4), torch.float32)
            _check(eng.lib, eng.lib.range_csp_head(eng._h, f.data_ptr(), B, ids.data_ptr(), 4, _native.CSP_HEAD_LOGITS,
                                                   plain.data_ptr(), eng._stream()))
            return plain, eng.csp_head(f), eng.csp_head(f, mode=_native.CSP_HEAD_SUM, max_grid=3)
        return (feats[0],), (feats[1],), call

    def predict():
        eng = _csp()
        real, decoy = locs()
        return (real,), (decoy,), lambda x: (eng.csp_predict(x), eng.csp_predict(x, mode=_native.CSP_HEAD_SUM))

    def rank():
        eng = _csp()
        labels, img, feats = extras()

        def call(f, lab, im):
            plain = tuple(eng._empty((B,), torch.int32) for _ in range(3))
            _check(eng.lib, eng.lib.range_csp_rank(eng._h, f.data_ptr(), B, im.data_ptr(), _native.CSP_IMG_F32, lab.data_ptr(),
                                                   *[t.data_ptr() for t in plain], eng._stream()))
            # (one tensor per call: tied_after alone is zero for either batch)
            return torch.stack(plain), torch.stack(eng.csp_rank(f, lab, im, max_grid=2)), torch.stack(eng.csp_rank(f, lab))
        return (feats[0], labels[0], img[0]), (feats[1], labels[1], img[1]), call

    def predict_rank():
        eng = _csp()
        labels, img, _ = extras()
        real, decoy = locs()
        return (real, labels[0], img[0]), (decoy, labels[1], img[1]), lambda x, lab, im: (torch.stack(eng.csp_predict_rank(x, lab, im)),)
    return [Case("csp_encode", ("range_csp_encode", "range_csp_encode_grid"), encode),
            Case("csp_head", ("range_csp_head", "range_csp_head_grid"), head),
            Case("csp_predict", ("range_csp_predict",), predict),
            Case("csp_rank", ("range_csp_rank", "range_csp_rank_grid"), rank),
            Case("csp_predict_rank", ("range_csp_predict_rank",), predict_rank)]


def _nearest_case(max_chunks):
    def build():
        eng = _engine(N=0)
        rad = lambda B, seed: torch.deg2rad(_q(B, seed))      # noqa: E731
        real, decoy = (rad(70, 11), rad(5000, 12)), (rad(70, 13), rad(5000, 14))
        torch.cuda.synchronize()
        return real, decoy, lambda q, s: eng.nearest_support(q, s, max_chunks=max_chunks)
    return Case("nearest_support_" + ("one_chunk" if max_chunks == 1 else "split"), ("range_nearest_support",), build)


CASES = ([_encode_case(128, B, raw) for B in (40, 600, 3000, 8192 + 77) for raw in (False, True)]
         + [_encode_case(768, 33, raw) for raw in (False, True)]
         + _features_cases() + _pass_cases() + _glue_cases()
         + [_topk_case(B, N, env) for B, N in ((8, N_BANK), (300, 1029)) for env in ((), UNFUSED)]
         + _topk_more_cases()
         + [_forward_case(tag, B, model, beta, **kw) for tag, B, kw in FORWARD_ROUTES for model, beta in MODELS]
         + [_forward_host_case(70, RANGE, 1.0), _forward_host_case(70, PLUS, 0.5), _forward_host_case(4096 + 64, PLUS, 0.5)]
         + [_flag_case()] + _csp_cases() + [_nearest_case(1), _nearest_case(0)])


# ---------------------------------------------------------------------------------------------- the tests
@pytest.fixture(scope="module", autouse=True)
def _release_contexts():
    """The shared contexts and batches live for this module only."""
    yield
    for cached in (_engine, _encoded, _csp):
        cached.cache_clear()


@gpu
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_call_orders_on_a_busy_stream(case):
    real, decoy, call = case.build()
    delay = SO.run_staged(case.name, DEV, real, decoy, call, blocks=case.blocks)
    print(f"{case.name}: delay {delay:.0f} ms, {SO.sleep_cycles_per_ms(DEV):.0f} cycles / ms")


@gpu
def test_the_harness_sees_a_call_on_a_stream_that_is_not_ordered():
    exposed = SO.control_exposes_stale_read(DEV)
    print("stale read exposed on:", ", ".join(exposed) or "no stream")
    assert exposed, "a stand-in call on four streams not ordered behind the busy one read the real batch every time"


COLD = (("forward_chunks_of_1", dict(env=CHUNK1), 130, lambda eng: lambda x: (eng.forward(x, PLUS, 0.5),)),
        ("topk_stream_B8", {}, 8, lambda eng: lambda x: eng.topk_stream(eng.encode(x)[1], 5)),
        ("topk_stream_B300_N1029", dict(N=1029), 300, lambda eng: lambda x: eng.topk_stream(eng.encode(x)[1], 5)),
        ("encode_B40", dict(N=0), 40, lambda eng: lambda x: eng.encode(x)))


@gpu
@pytest.mark.parametrize("name,engine_kw,B,make_call", COLD, ids=[c[0] for c in COLD])
def test_cold_start_on_a_busy_stream(name, engine_kw, B, make_call):
    """The first call a context ever sees is the staged one: the lazy fp16 key copy, the memset of the exact-count
    words, the first memset of the encoder's phase counters and every workspace's first growth sit on the caller's
    stream (growth may synchronise: only the bits are asserted)."""
    real, decoy = _pair(B)
    warm = make_call(_engine(**engine_kw))
    want, other = (tuple(t.clone() for t in warm(x)) for x in (real, decoy))
    torch.cuda.synchronize()
    fresh = _new_engine(**engine_kw)
    SO.run_staged("cold_" + name, DEV, (real,), (decoy,), make_call(fresh), cold=True, want=want, other=other)
    fresh.check_async_error()
    fresh.close()


@gpu
def test_two_contexts_interleaved_on_two_streams():
    """Two contexts, each with a bank of its own, each on a busy stream of its own; chunked forwards and fused top-k
    calls of both interleaved, nothing synchronised until the end: each result is that of the serial run."""
    B, k = 130, 5
    engines = [_new_engine(env=CHUNK1, seed=31), _new_engine(env=CHUNK1, seed=32)]
    real, decoy = _pair(B)
    e8 = [_engine(N=0).encode(x[:8].contiguous())[1] for x in (real, decoy)]      # the top-k calls' queries, encoded already

    def calls(eng, x, x8):
        out = eng.forward(x, PLUS, 0.5)
        tv, ti = eng.topk_stream(x8, k)
        return [out.clone(), tv.clone(), ti.clone()]
    serial = [[calls(eng, x, x8) for x, x8 in zip((real, decoy), e8)] for eng in engines]
    torch.cuda.synchronize()
    assert not torch.equal(serial[0][0][0], serial[1][0][0]) and not torch.equal(serial[0][0][0], serial[0][1][0])
    cycles = int(60.0 * SO.sleep_cycles_per_ms(DEV))
    streams = [torch.cuda.Stream(DEV) for _ in engines]
    gates = [torch.cuda.Event() for _ in engines]
    bufs = [(decoy.clone(), e8[1].clone()) for _ in engines]
    for S in streams:                                   # (the streams' allocator pools, as run_staged does)
        with torch.cuda.stream(S):
            spare = [torch.empty_like(t) for _ in range(6) for t in serial[0][0]] + [torch.empty(1 << 22, dtype=torch.uint8, device=DEV)]
            del spare
    torch.cuda.synchronize()
    for S, gate, (x, x8) in zip(streams, gates, bufs):
        with torch.cuda.stream(S):
            torch.cuda._sleep(cycles)
            gate.record(S)
            x.copy_(real, non_blocking=True)
            x8.copy_(e8[0], non_blocking=True)
    got = [[], []]
    for rnd in range(2):
        if rnd == 1:
            for S, (x, x8) in zip(streams, bufs):
                with torch.cuda.stream(S):
                    x.copy_(decoy, non_blocking=True)
                    x8.copy_(e8[1], non_blocking=True)
        # the forwards of both contexts, then their top-k calls: the calls of one context alternate with the other's
        outs = []
        for eng, S, (x, x8) in zip(engines, streams, bufs):
            with torch.cuda.stream(S):
                outs.append(eng.forward(x, PLUS, 0.5).clone())
        for i, (eng, S, (x, x8)) in enumerate(zip(engines, streams, bufs)):
            with torch.cuda.stream(S):
                tv, ti = eng.topk_stream(x8, k)
                got[i].append([outs[i], tv.clone(), ti.clone()])
    still_running = [not g.query() for g in gates]
    for S in streams:
        S.synchronize()
    torch.cuda.synchronize()
    assert all(still_running), "the delays had ended when everything was enqueued: a call blocked the host"
    for i in range(2):
        for rnd in range(2):
            for j, (g, w) in enumerate(zip(got[i][rnd], serial[i][rnd])):
                assert torch.equal(g, w), f"context {i}, round {rnd}, output {j}"
    for eng in engines:
        eng.check_async_error()
        eng.close()


def test_every_stream_taking_entry_point_has_a_case():
    """Needs no GPU: the five public headers against the case tables of both stream-order modules."""
    import test_gpu_stream_order_side as side
    found = SO.stream_entry_points()
    assert {h: len(v) for h, v in found.items()} == {"range_hip.h": 31, "range_neighbors.h": 10, "range_probe.h": 9,
                                                     "range_map.h": 4, "range_cluster.h": 3}
    declared = set(NO_STAGED_CASE)
    for case in list(CASES) + list(side.CASES):
        declared.update(case.covers)
    names = {n for v in found.values() for n in v}
    assert len(names) == 57
    missing, unknown = sorted(names - declared), sorted(declared - names)
    assert not missing, f"entry points with a range_stream_t parameter and no stream-order case: {missing}"
    assert not unknown, f"the case tables name entry points the headers do not declare: {unknown}"
    # a name listed as without a case must not also have one
    assert not set(NO_STAGED_CASE) & {n for case in list(CASES) + list(side.CASES) for n in case.covers}
    print(f"{len(names)} stream-taking entry points: {len(names) - len(NO_STAGED_CASE)} with a case, "
          f"{len(NO_STAGED_CASE)} without ({', '.join(NO_STAGED_CASE)})")
