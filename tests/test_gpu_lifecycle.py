"""The retrieval engine and the model on a context that has already done something else (`-m gpu`).

Almost every other GPU test creates an engine, installs one encoder and one bank and calls one route.  The
product keeps ONE context for its whole life: its device buffers only grow and are never cleared, and a few
validity words (engine_ctx.h: kept_B / kept_total / kept_blocks, ws_queries, tg_key_scale, vplanes_groups, the
sh-table pointers, ...) decide whose contents may be read.  Here every scenario runs on a context with a history -
a poisoned larger bank (tests/lifecycle.py), a larger batch, another encoder, a refused setter - and every result
is compared bit for bit with the exact expectation of tools/exact_bank.py, or, where no exact expectation exists
(encoder outputs), with a fresh context that only ever saw the final state plus the oracle at the bound of
test_gpu_parity.test_encoder_vs_oracle.  Every comparison is ``torch.equal`` / ``_assert_equal`` / ``_assert_rows``,
a refusal with its code, or that bound.
"""
import os
import re

import numpy as np
import pytest
import torch

import exact_dense_cases as D
import lifecycle as L
from exact_helpers import DEV, H_ENC, L_ENC, _assert_equal, _assert_rows, _dev, _env, _fwd_want, _model
from oracle import range_oracle as O
from range_amd import _native, sh_table
from tools import exact_bank as X
from tools import synth

pytestmark = pytest.mark.gpu
TAU, TAU2, BETA = L.TAU, L.TAU2, L.BETA
PLUS = _native.MODEL_RANGE_PLUS
T48, T64 = X.dense_tau(48), X.dense_tau(64)
INVALID, STATE = -1, -3

_ENGINES = {}


def _engine(tag, **env):
    """The context ``tag`` of this module, created under ``env`` on first use."""
    key = (tag, tuple(sorted(env.items())))
    if key not in _ENGINES:
        with _env(**env):
            _ENGINES[key] = _native.HipEngine(DEV)
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _release_engines():
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()
    torch.cuda.empty_cache()


def _refused(code, fn, *a, **kw):
    with pytest.raises(_native.RangeNativeError, match=re.escape(f"librange_hip error {code}:")):
        fn(*a, **kw)


def _const_encoder(eng, vec):
    """An encoder whose e-hat is ``vec`` for every query (last layer: weight 0, bias ``vec``; exact_helpers._model)."""
    w = synth.make_encoder_weights(L_ENC, H_ENC, 256, 2, 5)
    w["last_layer.weight"][:] = 0.0
    w["last_layer.bias"][:] = vec
    eng.set_encoder(L_ENC, H_ENC, 2, 256, _native.SH_CLOSED_FORM,
                    [w["layers.0.weight"], w["layers.1.weight"], w["last_layer.weight"]],
                    [w["layers.0.bias"], w["layers.1.bias"], w["last_layer.bias"]])


def _lonlat(q):
    return torch.from_numpy(X.lonlat_of(q.geo)).to(DEV)


def _check_stats(st, bank, q, what, tau=TAU):
    _assert_equal(st, _dev(X.expect_stats(bank, q, tau, tau)), f"{what}: statistics")


def _check_topk(tv, ti, bank, q, k, off, what):
    wv, wi = X.topk_expect(bank, q, k)
    assert int(ti.min()) >= off and int(ti.max()) < bank.n + off, f"{what}: a row outside the bank"
    _assert_equal(ti, _dev(wi + off), f"{what}: indices")
    _assert_equal(tv, _dev(wv), f"{what}: values")


def _install(engines, arrays, off=0):
    for e in engines:
        e.set_bank(*arrays, row_offset=off)


def _check_forward(eng, bank, q, B, what, beta=BETA, host=False):
    q = X.Queries(q.sem[:B], q.geo[:B], q.e32[:B], q.xq[:B])
    want = _fwd_want(bank, q, beta, True)
    x = _lonlat(q)
    out = eng.forward_host(x, PLUS, beta) if host else eng.forward(x, PLUS, beta)
    _assert_rows(out, want, what)
    return out


def _check_routes(eng, nokeep, n, off, what):
    """Every route of ``eng`` - and the in-scan top-k lists of ``nokeep``, a context that cannot keep logits -
    on the exact bank of ``n`` rows both hold, at row offset ``off``."""
    bank, q, k = L.exact(n), L.route_queries(n), L.topk_k(n)
    B = len(q.sem)
    e32, xq = _dev(q.e32), _dev(q.xq)
    want = _dev(X.expect(bank, q, BETA))
    _check_stats(eng.scan_stats(e32, xq, TAU, TAU), bank, q, f"{what} scan_stats")
    st, tv, ti = eng.scan_stats(e32, xq, TAU, TAU, topk=k, keep_logits=True)
    _check_stats(st, bank, q, f"{what} scan_stats(topk)")
    _check_topk(tv, ti, bank, q, k, off, f"{what} scan_stats(topk) from kept logits")
    st, tv, ti = nokeep.scan_stats(e32, xq, TAU, TAU, topk=k, keep_logits=True)
    assert nokeep.kept_queries() == 0
    _check_stats(st, bank, q, f"{what} scan_stats(topk), in-scan lists")
    _check_topk(tv, ti, bank, q, k, off, f"{what} scan_stats(topk), in-scan lists")
    _assert_equal(nokeep.attend(e32, xq, TAU, TAU, BETA, st), want, f"{what} attend (nothing kept)")
    st = eng.scan_stats(e32, xq, TAU, TAU, keep_logits=True)
    _check_stats(st, bank, q, f"{what} scan_stats(keep_logits)")
    assert eng.kept_queries() == B
    _assert_equal(eng.attend(e32, xq, TAU, TAU, BETA, st), want, f"{what} attend")
    _assert_equal(eng.attend_kept(0, xq, TAU, TAU, BETA, st), want, f"{what} attend_kept")
    a, b = 64, 165
    _assert_equal(eng.attend_kept(a, xq[a:b], TAU, TAU, BETA, st[a:b].contiguous()), want[a:b], f"{what} attend_kept [{a},{b})")
    _check_stats(eng.stats_kept(0, xq, [(TAU2, TAU2)])[0], bank, q, f"{what} stats_kept", tau=TAU2)
    for Bt in L.TOPK_B:
        tv, ti = eng.topk_stream(e32[:Bt], k)
        _check_topk(tv, ti, bank, X.Queries(q.sem[:Bt], q.geo[:Bt], None, None), k, off, f"{what} topk_stream B={Bt}")
    # the forward routes: an encoder that returns the first class's direction, both heads at 43
    _const_encoder(eng, bank.class_vectors([L.FORWARD_CLASS])[0])
    eng.set_temperatures(TAU, TAU)
    for Bf in L.FORWARD_B:
        fq = L.forward_queries(n, Bf)
        _check_forward(eng, bank, fq, Bf, f"{what} forward B={Bf}")
        if Bf == 33:
            tv, ti = eng.topk_last(Bf, k)
            _check_topk(tv, ti, bank, fq, k, off, f"{what} topk_last")
            _check_forward(eng, bank, fq, Bf, f"{what} forward_host B={Bf}", host=True)
            assert eng.kept_queries() == Bf
            eng.scan_stats(_dev(fq.e32), _dev(fq.xq), TAU, TAU)             # (no keep_logits: forgets the forward's)
            assert eng.kept_queries() == 0
    eng.set_temperatures(0.0, 0.0)


# -- a. the bank shrinks and grows ---------------------------------------------------------------------------
class _Walk:
    """The banks one pair of contexts (default; RANGE_KEEP_LOGITS=0) has held, in order: a test asks for the history
    it needs and the walk installs what is missing, so every test also runs alone."""

    def __init__(self, kind, off):
        tag = f"walk-{kind}-{off}"
        self.engines = [_engine(tag), _engine(tag, RANGE_KEEP_LOGITS=0)]
        self.kind, self.off = kind, off
        self.poison = L.poison_bank(L.PRED_N, kind)

    def install_poison(self):
        _install(self.engines, self.poison, self.off)

    def install_exact(self, n):
        _install(self.engines, L.exact(n).rows(0, n), self.off)

    def fill(self):
        """A poisoned predecessor that every route has run on (workspaces, key copies, planes hold its rows)."""
        q = L.route_queries(L.SUCCESSORS[0])
        e32, xq = _dev(q.e32), _dev(q.xq)
        for e in self.engines:
            st = e.scan_stats(e32, xq, TAU, TAU, topk=16, keep_logits=True)[0]
            e.attend(e32, xq, TAU, TAU, BETA, st)                          # (slabs of overflowing / NaN sums: not looked at)
            e.topk_stream(e32, 16)
            e.topk_stream(e32[:16], 16)


_WALKS = {}


def _walk(kind, off):
    if (kind, off) not in _WALKS:
        _WALKS[(kind, off)] = _Walk(kind, off)
    return _WALKS[(kind, off)]


@pytest.mark.parametrize("n", L.SUCCESSORS)
@pytest.mark.parametrize("kind", L.KINDS)
def test_bank_shrinks(kind, n):
    """poison (12 500 rows, used by a scan and both top-k routes) -> the exact bank of ``n`` rows: every route exact."""
    w = _walk(kind, 0)
    w.install_poison()
    w.fill()
    w.install_exact(n)
    _check_routes(*w.engines, n, 0, f"{kind} -> {n}:")


@pytest.mark.parametrize("kind", L.KINDS)
def test_bank_grows_back(kind):
    """17 -> 12 500 -> 50 001 rows behind a poisoned predecessor: the last size takes bank splits where the others took
    the stream-K walk, and reallocates every bank buffer."""
    w = _walk(kind, 0)
    w.install_poison()
    for n in L.GROWTH:
        w.install_exact(n)
        _check_routes(*w.engines, n, 0, f"{kind} ... -> {n}:")


@pytest.mark.parametrize("kind", L.KINDS)
def test_bank_shrinks_at_a_row_offset(kind):
    """The shrink again with row offset 77 on the poison and on every successor."""
    w = _walk(kind, 77)
    for n in L.SUCCESSORS:
        w.install_poison()
        w.fill()
        w.install_exact(n)
        _check_routes(*w.engines, n, 77, f"{kind} -> {n} at row offset 77:")


# -- b. workspaces filled by a larger call -------------------------------------------------------------------
def _ws_routes(eng, B, big, what, check=True):
    """scan (kept, top-k), both passes 2, stats_kept, top-k stream on the 12 500-row bank with queries of the ``big``
    or the small calls' classes; ``check`` False: only fill the workspaces."""
    bank, q = L.exact(L.WS_N), L.ws_queries(B, big)
    e32, xq = _dev(q.e32), _dev(q.xq)
    st, tv, ti = eng.scan_stats(e32, xq, TAU, TAU, topk=16, keep_logits=True)
    st = eng.scan_stats(e32, xq, TAU, TAU, keep_logits=True)
    outs = [eng.attend_kept(0, xq, TAU, TAU, BETA, st), eng.attend(e32, xq, TAU, TAU, BETA, st)]
    sk = eng.stats_kept(0, xq, [(TAU2, TAU2), (TAU, TAU)])
    ts = eng.topk_stream(e32, 16)
    if not check:
        return
    want = _dev(X.expect(bank, q, BETA))
    _check_stats(st, bank, q, f"{what} scan_stats")
    _check_topk(tv, ti, bank, q, 16, 0, f"{what} scan_stats(topk)")
    _assert_equal(outs[0], want, f"{what} attend_kept")
    _assert_equal(outs[1], want, f"{what} attend")
    _check_stats(sk[0], bank, q, f"{what} stats_kept", tau=TAU2)
    _check_stats(sk[1], bank, q, f"{what} stats_kept at the scan's temperature")
    _check_topk(*ts, bank, q, 16, 0, f"{what} topk_stream")


def _ws_forward(eng, big, B, what):
    bank, c = L.exact(L.WS_N), L.ws_forward_class(big)
    _const_encoder(eng, bank.class_vectors([c])[0])
    eng.set_temperatures(TAU, TAU)
    return _check_forward(eng, bank, L.ws_forward_queries(B, big), B, what)


@pytest.mark.parametrize("env", [{}, {"RANGE_P2_STREAMK": 0}], ids=["streamk", "splits"])
def test_workspaces_filled_by_a_larger_call(env):
    """B = 4 097 first (kept logits, every slab, the candidate lists, the statistics parts), then 1, 17, 33 and 65
    queries of OTHER classes, then 257: a stale tile, slab or list carries the wrong class's values."""
    eng = _engine("ws", **env)
    eng.set_bank(*L.exact(L.WS_N).rows(0, L.WS_N))
    _ws_routes(eng, L.WS_BIG_B, True, f"{env} B={L.WS_BIG_B}")
    _ws_forward(eng, True, L.WS_BIG_B, f"{env} forward B={L.WS_BIG_B}")
    for B in L.WS_SMALL_B + (L.WS_MID_B,):
        _ws_routes(eng, B, False, f"{env} B={B} behind B={L.WS_BIG_B}")
        _ws_forward(eng, False, B, f"{env} forward B={B} behind B={L.WS_BIG_B}")


@pytest.mark.parametrize("env", [{"RANGE_FWD_OVERLAP": 2}, {"RANGE_FWD_OVERLAP": 2, "RANGE_P2_STREAMK": 0}],
                         ids=["streamk", "splits"])
def test_forward_overlap_workspaces(env):
    """Chunks on the auxiliary stream: B = 700, 130, 700 - exact, and the third the first bit for bit."""
    eng = _engine("overlap", **env)
    eng.set_bank(*L.exact(L.WS_N).rows(0, L.WS_N))
    outs = [_ws_forward(eng, i != 1, B, f"{env} forward B={B} (call {i})") for i, B in enumerate(L.WS_OVERLAP_B)]
    assert torch.equal(outs[0], outs[2])


# -- c. set_keys and set_bank alternate -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", L.KINDS)
def test_set_keys_and_set_bank_alternate(kind):
    n = 4099
    bank, q = L.exact(n), L.route_queries(n)
    eng, nokeep = _engine("alternate"), _engine("alternate", RANGE_KEEP_LOGITS=0)
    _install([eng, nokeep], L.poison_bank(L.PRED_N, kind))
    e32, xq = _dev(q.e32), _dev(q.xq)
    eng.topk_stream(e32, 16)
    eng.set_keys(bank.keys)
    for Bt in L.TOPK_B:
        tv, ti = eng.topk_stream(e32[:Bt], 16)
        _check_topk(tv, ti, bank, X.Queries(q.sem[:Bt], q.geo[:Bt], None, None), 16, 0, f"keys only: topk_stream B={Bt}")
    _const_encoder(eng, bank.class_vectors([L.FORWARD_CLASS])[0])
    st = torch.zeros((len(q.sem), 4), device=DEV)
    _refused(STATE, eng.scan_stats, e32, xq, TAU, TAU)
    _refused(STATE, eng.attend, e32, xq, TAU, TAU, BETA, st)
    _refused(STATE, eng.forward, _lonlat(q), PLUS, BETA)
    _refused(STATE, eng.forward, _lonlat(q)[:5], PLUS, BETA)
    _install([eng, nokeep], bank.rows(0, n))
    _check_routes(eng, nokeep, n, 0, f"{kind} -> keys -> {n}:")


@pytest.mark.parametrize("name,B,beta", [("n108", 17, 0.25), ("n4099", 65, 0.75)])
def test_planes_follow_set_keys_and_set_bank(name, B, beta):
    """pv_mode bf16x3 over poison -> set_keys -> the dense bank (its bf16x3 answer is exact: test_gpu_exact_dense.
    test_bf16x3_dense): set_keys released the planes, the set_bank behind it rebuilt them from ITS values."""
    bank = D.bank(name)
    q = X.queries(bank, B, seed=B, perturb=D.perturbed(name))
    X.assert_bank_margin(bank, q, beta, T48, T48)
    e32, xq, want = _dev(q.e32), _dev(q.xq), _dev(X.expect(bank, q, beta))
    eng = _engine("planes")
    eng.set_pv_mode("bf16x3")
    try:
        eng.set_bank(*L.poison_bank(L.PRED_N, "huge"))
        eng.set_keys(bank.keys)
        eng.set_pv_mode("bf16x3")                   # (nothing to build on a keys-only bank; the mode stays)
        assert eng.pv_mode == "bf16x3"
        eng.set_bank(bank.keys, bank.values, bank.xyz)
        st = eng.scan_stats(e32, xq, T48, T48, keep_logits=True)
        _assert_equal(st, _dev(X.expect_stats(bank, q, T48, T48)), "scan_stats")
        _assert_equal(eng.attend_kept(0, xq, T48, T48, beta, st), want, "attend_kept bf16x3 behind poison and set_keys")
    finally:
        eng.set_pv_mode("exact")
    _assert_equal(eng.attend_kept(0, xq, T48, T48, beta, st), want, "attend_kept exact")


# -- d. kept-logit validity ------------------------------------------------------------------------------------
def test_kept_logits_are_never_answered_from_old_tiles():
    n, other = 4099, 12500
    bank, q = L.exact(n), L.route_queries(n)
    B = len(q.sem)
    e32, xq, want = _dev(q.e32), _dev(q.xq), _dev(X.expect(bank, q, BETA))
    eng = _engine("kept")
    eng.set_bank(*bank.rows(0, n))
    st = eng.scan_stats(e32, xq, TAU, TAU, keep_logits=True)
    _assert_equal(eng.attend_kept(0, xq, TAU, TAU, BETA, st), want, "attend_kept")

    def refused(what):
        assert eng.kept_queries() == 0, what
        _refused(STATE, eng.attend_kept, 0, xq, TAU, TAU, BETA, st)
        _refused(STATE, eng.stats_kept, 0, xq, [(TAU2, TAU2)])

    eng.set_bank(*L.exact(other).rows(0, other))
    refused("set_bank")
    eng.set_bank(*bank.rows(0, n))
    eng.scan_stats(e32, xq, TAU, TAU, keep_logits=True)
    eng.scan_stats(e32, xq, TAU, TAU)
    refused("a scan without keep_logits")
    eng.scan_stats(e32, xq, TAU, TAU, keep_logits=True)
    eng.scan_stats_at(e32[:64], xq[:64], TAU, TAU, 128, B)
    refused("scan_stats_at that does not extend the scan")
    eng.scan_stats_at(e32[:64], xq[:64], TAU, TAU, 0, B)
    assert eng.kept_queries() == 64
    eng.scan_stats_at(e32[64:128], xq[64:128], TAU, TAU, 64, B + 64)
    refused("scan_stats_at with another total_queries")
    # a valid chain: chunks extended in order, a stats_kept, attend_kept - the single scan's bits
    cuts = [0, 64, 192, B]
    sts = [eng.scan_stats_at(e32[a:b], xq[a:b], TAU, TAU, a, B) for a, b in zip(cuts[:-1], cuts[1:])]
    assert eng.kept_queries() == B
    _assert_equal(torch.cat(sts), st, "scan_stats_at chunks")
    _check_stats(eng.stats_kept(0, xq, [(TAU2, TAU2)])[0], bank, q, "stats_kept behind the chunks", tau=TAU2)
    _assert_equal(eng.attend_kept(0, xq, TAU, TAU, BETA, torch.cat(sts)), want, "attend_kept behind the chunks")
    _refused(INVALID, eng.attend_kept, 64, xq, TAU, TAU, BETA, st)          # [64, 64 + B) exceeds the B kept
    _assert_equal(eng.attend_kept(0, xq, TAU, TAU, BETA, st), want, "attend_kept behind a refusal")
    # a context that cannot keep
    nokeep = _engine("kept", RANGE_KEEP_LOGITS=0)
    nokeep.set_bank(*bank.rows(0, n))
    st2 = nokeep.scan_stats(e32, xq, TAU, TAU, keep_logits=True)
    _assert_equal(st2, st, "scan_stats under RANGE_KEEP_LOGITS=0")
    assert nokeep.kept_queries() == 0
    _refused(STATE, nokeep.attend_kept, 0, xq, TAU, TAU, BETA, st)


def test_attend_kept_on_the_rows_a_forward_kept():
    n, B = 4099, 257
    bank = L.exact(n)
    eng = _engine("kept")
    eng.set_bank(*bank.rows(0, n))
    _const_encoder(eng, bank.class_vectors([L.FORWARD_CLASS])[0])
    eng.set_temperatures(TAU, TAU)
    try:
        fq = L.forward_queries(n, B)
        out = _check_forward(eng, bank, fq, B, "forward")
        assert eng.kept_queries() == B
        xq = _dev(fq.xq)
        st = _dev(X.expect_stats(bank, fq, TAU, TAU))
        got = eng.attend_kept(0, xq, TAU, TAU, BETA, st)
        assert torch.equal(got.double(), out[:, :1024])
        a = 64
        got = eng.attend_kept(a, xq[a:], TAU, TAU, BETA, st[a:].contiguous())
        assert torch.equal(got.double(), out[a:, :1024])
    finally:
        eng.set_temperatures(0.0, 0.0)


def test_what_set_bank_and_set_encoder_keep():
    """INTEGRATION.md's table: range_topk_last's claim - the e-hat of the last forward - outlives range_set_encoder and
    range_set_bank (then scanned against the NEW keys) and is taken by range_encode_raw; the kept logits outlive
    range_set_encoder and range_set_pv_mode, not range_set_bank."""
    n, other, B, k = 4099, 12500, 257, 16
    bank = L.exact(n)
    eng = _engine("keeps")
    eng.set_bank(*bank.rows(0, n))
    _const_encoder(eng, bank.class_vectors([L.FORWARD_CLASS])[0])
    eng.set_temperatures(TAU, TAU)
    try:
        fq = L.forward_queries(n, B)
        e32, xq = _dev(fq.e32), _dev(fq.xq)
        out = _check_forward(eng, bank, fq, B, "forward")
        st = _dev(X.expect_stats(bank, fq, TAU, TAU))
        kept = eng.attend_kept(0, xq, TAU, TAU, BETA, st)
        assert torch.equal(kept.double(), out[:, :1024])
        tv, ti = eng.topk_last(B, k)
        _check_topk(tv, ti, bank, fq, k, 0, "topk_last")
        # another encoder: the kept logits and the claim belong to the queries already embedded
        _set_encoder(eng, ENCODERS[1])
        assert eng.kept_queries() == B
        _assert_equal(eng.attend_kept(0, xq, TAU, TAU, BETA, st), kept, "attend_kept behind set_encoder")
        tv2, ti2 = eng.topk_last(B, k)
        assert torch.equal(tv2, tv) and torch.equal(ti2, ti)
        # another bank: the kept logits go, the claim stays and meets the new keys
        big = L.exact(other)
        eng.set_bank(*big.rows(0, other))
        assert eng.kept_queries() == 0
        _refused(STATE, eng.attend_kept, 0, xq, TAU, TAU, BETA, st)
        tv3, ti3 = eng.topk_last(B, k)
        wv, wi = eng.topk_stream(e32, k)
        assert torch.equal(tv3, wv) and torch.equal(ti3, wi) and int(ti3.max()) < other
        # range_encode_raw takes the claim for ITS queries
        x = _dev(synth.make_queries(33, seed=9))
        _, q32, _ = eng.encode(x)
        eng.encode_raw(x)
        _refused(STATE, eng.topk_last, B, k)
        tv4, ti4 = eng.topk_last(33, k)
        wv, wi = eng.topk_stream(q32, k)
        assert torch.equal(tv4, wv) and torch.equal(ti4, wi)
    finally:
        eng.set_temperatures(0.0, 0.0)


# -- e. modes and temperatures flip ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,beta", [("n108", 17, 0.25), ("n4099", 65, 0.75)])
def test_pv_mode_flips(name, B, beta):
    bank = D.bank(name)
    q = X.queries(bank, B, seed=B, perturb=D.perturbed(name))
    X.assert_bank_margin(bank, q, beta, T48, T48)
    e32, xq, want = _dev(q.e32), _dev(q.xq), _dev(X.expect(bank, q, beta))
    eng = _engine("modes")
    eng.set_bank(bank.keys, bank.values, bank.xyz)
    st = eng.scan_stats(e32, xq, T48, T48, keep_logits=True)
    try:
        for i, mode in enumerate(("exact", "bf16x3", "exact", "bf16x3")):
            eng.set_pv_mode(mode)
            assert eng.pv_mode == mode
            _assert_equal(eng.attend_kept(0, xq, T48, T48, beta, st), want, f"attend_kept, switch {i} to {mode}")
    finally:
        eng.set_pv_mode("exact")


def test_temperatures_flip():
    """set_temperatures default -> 48 (the running-maximum pass 1) -> 0 (the defaults again) -> 12 -> 48 with forwards
    behind each.  Exact: the defaults (12, 40) for the geographic head alone (beta = 0), (48, 40) for both heads.  What
    shows that a temperature was restored is the forward at beta = 1/2 under the defaults: at tau 12 the other
    classes' mass (4 308 rows at e^-12 beside 8 192) is in l_sem, so the result is no exact number and differs in bits
    from the one at 48 - and it must come back bit for bit behind set_temperatures(0, 0) and (12, 0).  Then the same for
    the geographic temperature: (0, 5) moves the result, (0, 0) and the defaults spelled out (12, 40) restore it."""
    n = L.WS_N
    bank = L.exact(n)
    eng = _engine("temps")
    eng.set_bank(*bank.rows(0, n))
    _const_encoder(eng, bank.class_vectors([L.FORWARD_CLASS])[0])
    for B in (33, 700):
        q = L.forward_queries(n, B)
        x = _lonlat(q)
        exact, blend = {}, {}
        for step, ts in enumerate((0.0, L.TAU_SHARP, 0.0, 12.0, L.TAU_SHARP)):
            eng.set_temperatures(ts, 0.0)
            what = f"forward B={B} behind set_temperatures({ts}, 0), step {step}"
            exact[step] = _check_forward(eng, bank, q, B, what, beta=BETA if ts == L.TAU_SHARP else 0.0)
            blend[step] = eng.forward(x, PLUS, BETA)
        for step in (1, 4):                                  # sharp: the blend is the exact forward itself
            assert torch.equal(blend[step], exact[step])
        assert not torch.equal(blend[0][:, :1024], blend[1][:, :1024]), "tau 12 and tau 48 cannot be told apart"
        for step in (2, 3):
            _assert_equal(blend[step], blend[0], f"B={B} step {step}: the semantic temperature was not restored")
            assert torch.equal(exact[step], exact[0])
        assert torch.equal(exact[1], exact[4])
        # the geographic temperature
        eng.set_temperatures(0.0, 0.0)
        eng.set_temperatures(0.0, 5.0)
        moved = eng.forward(x, PLUS, BETA)
        assert not torch.equal(moved[:, :1024], blend[0][:, :1024]), "tau_geo 5 and 40 cannot be told apart"
        for pair in ((0.0, 0.0), (12.0, 40.0), (0.0, 40.0)):
            eng.set_temperatures(*pair)
            _assert_equal(eng.forward(x, PLUS, BETA), blend[0], f"B={B} set_temperatures{pair}: the defaults were not restored")
        eng.set_temperatures(0.0, 5.0)
        _assert_equal(eng.forward(x, PLUS, BETA), moved, f"B={B} set_temperatures(0, 5) again")
        _refused(INVALID, eng.set_temperatures, 1001.0, 0.0)         # refused: the pair stays (0, 5)
        _assert_equal(eng.forward(x, PLUS, BETA), moved, f"B={B} behind a refused set_temperatures")
        eng.set_temperatures(0.0, 0.0)


def test_temperatures_flip_dense():
    """The arithmetic side of the same flips: a dense bank at k = 48 (constant shift), one at k = 64 (sharp), the
    first again - the first and the third forward equal bit for bit."""
    eng = _engine("temps-dense")
    outs = []
    try:
        for name, tau, beta in L.DENSE_TEMPS:
            bank = D.bank(name)
            c = L.dense_forward_class(name)
            eng.set_bank(bank.keys, bank.values, bank.xyz)
            _const_encoder(eng, bank.class_vectors([c])[0])
            eng.set_temperatures(tau, tau)
            for B in L.DENSE_TEMPS_B:
                q = X.forward_queries(bank, c, B, B)
                X.assert_bank_margin(bank, q, beta, tau, tau)
                outs.append(_check_forward(eng, bank, q, B, f"{name} forward B={B} at k={bank.k}", beta=beta))
    finally:
        eng.set_temperatures(0.0, 0.0)
    assert torch.equal(outs[0], outs[4]) and torch.equal(outs[1], outs[5])


# -- f. the encoder replaced -------------------------------------------------------------------------------------
# (L, hidden, layers, mode, seed, with the faithful table)
ENCODERS = [(40, 512, 2, "analytic", 1234, True), (10, 64, 2, "closed-form", 5, False), (16, 1000, 2, "analytic", 6, False),
            (7, 192, 1, "analytic", 8, False), (40, 512, 2, "analytic", 1234, False)]
ENC_B = (1, 16, 17, 513, 4097)
ENC_N = 4099
_ENC_DONE = []                                      # the encoders the module's context has held, in order


def _enc_queries():
    """The pole-to-pole locations of test_gpu_parity.test_encoder_reference_mode_over_all_latitudes (300 of them, its
    bounds against the faithful oracle hold on these), repeated up to the largest batch."""
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "latitude_L40_H512_n2.npz"))
    return np.ascontiguousarray(np.resize(z["lonlat"], (max(ENC_B), 2)))


def _set_encoder(eng, spec):
    Lp, H, layers, mode, seed, table = spec
    w = synth.make_encoder_weights(Lp, H, 256, layers, seed)
    ws = [w[f"layers.{i}.weight"] for i in range(layers)] + [w["last_layer.weight"]]
    bs = [w[f"layers.{i}.bias"] for i in range(layers)] + [w["last_layer.bias"]]
    eng.set_encoder(Lp, H, layers, 256, _native.SH_ANALYTIC if mode == "analytic" else _native.SH_CLOSED_FORM, ws, bs,
                    sh_table=sh_table.generate_table(Lp) if table else None)
    return w


def _encoder_outputs(eng, x):
    outs = {f"encode B={B}": eng.encode(x[:B].contiguous()) for B in ENC_B}
    outs["encode_raw B=33"] = (eng.encode_raw(x[:33].contiguous()),)
    for B in (5, 33, 257):
        outs[f"forward B={B}"] = (eng.forward(x[:B].contiguous(), PLUS, BETA),)
    return outs


@pytest.mark.parametrize("step", range(len(ENCODERS)))
def test_encoder_replaced(step):
    """One context takes the five encoders in turn (an installed bank stays): after each, encode at every launch
    geometry, encode_raw and a forward equal a fresh context's bit for bit, and e-hat meets the oracle - the exact
    recurrence's at 2e-12 (test_encoder_vs_oracle), the faithful polynomials' for the first step at the bounds of
    test_encoder_reference_mode_over_all_latitudes.  The last step has the first one's network WITHOUT the table."""
    q = _enc_queries()
    x = _dev(q)
    used = _engine("encoders")
    bank = L.exact(ENC_N)
    if not used.n_rows:
        used.set_bank(*bank.rows(0, ENC_N))
    for s in range(len(_ENC_DONE), step):           # the history, when this step runs alone
        _set_encoder(used, ENCODERS[s])
        _encoder_outputs(used, x)
        _ENC_DONE.append(s)
    _ENC_DONE.append(step)
    w = _set_encoder(used, ENCODERS[step])
    fresh = _native.HipEngine(DEV)
    try:
        _set_encoder(fresh, ENCODERS[step])
        fresh.set_bank(*bank.rows(0, ENC_N))
        got, want = _encoder_outputs(used, x), _encoder_outputs(fresh, x)
    finally:
        fresh.close()
    for what in want:
        for g, t in zip(got[what], want[what]):
            _assert_equal(g, t, f"step {step}: {what} against a fresh context")
    Lp, H, layers, mode, seed, table = ENCODERS[step]
    al = np.abs(q[:, 1])
    ref = O.encode(q, w, Lp, features=O.sh_features_faithful(q, O.load_ylm_table(), Lp)) if table else O.encode(q, w, Lp, mode)
    for B in ENC_B:
        e64 = got[f"encode B={B}"][0].cpu().numpy()
        if table:
            d = np.abs(e64 - ref[:B]).max(axis=1)
            assert np.where(al[:B] <= 45, d, 0.0).max() < 1e-7 and d.max() < 5.5e-4, f"step {step}: encode B={B} (faithful oracle)"
        else:
            np.testing.assert_allclose(e64, ref[:B], rtol=0, atol=2e-12, err_msg=f"step {step}: encode B={B}")


# -- g. refusals change nothing --------------------------------------------------------------------------------
def test_refusals_change_nothing():
    n = 4099
    bank, q = L.exact(n), L.route_queries(n)
    eng = _engine("refusals")
    eng.set_bank(*bank.rows(0, n))
    Lp, H = 10, 64
    w = _set_encoder(eng, (Lp, H, 2, "analytic", 5, True))
    x = _dev(synth.make_queries(300, seed=9))
    e32 = _dev(q.e32)
    lib, h = eng.lib, eng._h

    def state():
        outs = [eng.forward(x[:B].contiguous(), PLUS, BETA) for B in (5, 33, 300)]
        tv, ti = eng.topk_stream(e32, 16)
        _check_topk(tv, ti, bank, q, 16, 0, "topk_stream")
        return outs + [tv, ti, eng.encode(x)[0]]

    before = state()

    def unchanged(what):
        for a, b in zip(state(), before):
            assert torch.equal(a, b), f"results moved behind a refused {what}"

    def enc(hidden, embed):
        ww = synth.make_encoder_weights(Lp, hidden, embed, 2, 5)
        return ([ww["layers.0.weight"], ww["layers.1.weight"], ww["last_layer.weight"]],
                [ww["layers.0.bias"], ww["layers.1.bias"], ww["last_layer.bias"]])

    _refused(INVALID, eng.set_encoder, Lp, 1088, 2, 256, _native.SH_ANALYTIC, *enc(1088, 256))
    unchanged("set_encoder(hidden 1088)")
    _refused(INVALID, eng.set_encoder, Lp, H, 2, 128, _native.SH_ANALYTIC, *enc(H, 128))
    unchanged("set_encoder(embed_dim 128)")

    def sh_table_rc(Lt):
        t = sh_table.generate_table(Lt)
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)   # noqa: E731
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)     # noqa: E731
        arrs = [f64(t.front), f64(t.a0), f64(t.a2), i32(t.p2), i32(t.kx), i32(t.off), i32(t.cnt)]
        coef, powr = f64(t.coef), i32(t.pow)
        return lib.range_set_sh_table(h, Lt, *[a.ctypes.data for a in arrs], coef.shape[0], coef.ctypes.data, powr.ctypes.data)

    assert sh_table_rc(9) == INVALID
    unchanged("set_sh_table(L = 9)")
    z = np.zeros((16, 1024), np.float32)
    assert lib.range_set_bank(h, z.ctypes.data, z.ctypes.data, z.ctypes.data, 0, 0) == INVALID
    assert lib.range_set_keys(h, z.ctypes.data, 0, 0) == INVALID
    unchanged("set_bank(n_rows = 0)")
    assert lib.range_set_pv_mode(h, 7) == INVALID and eng.pv_mode == "exact"
    unchanged("set_pv_mode(7)")
    _refused(INVALID, eng.set_temperatures, 1001.0, 0.0)
    unchanged("set_temperatures(1001, 0)")
    eng.scan_stats(e32, _dev(q.xq), TAU, TAU, keep_logits=True)
    st = torch.zeros((len(q.sem), 4), device=DEV)
    _refused(INVALID, eng.attend_kept, 64, _dev(q.xq), TAU, TAU, BETA, st)
    unchanged("attend_kept beyond the kept count")
    for B in (5, 33, 300):                       # the one-pass route, two passes
        _refused(INVALID, eng.forward, x[:B].contiguous(), PLUS, 2.0)
        _refused(INVALID, eng.forward_host, x[:B].contiguous(), PLUS, 2.0)
    unchanged("forward(beta = 2)")
    # a closed-form encoder takes no table, and goes on as it was
    _set_encoder(eng, (Lp, H, 2, "closed-form", 5, False))
    before = state()
    assert sh_table_rc(Lp) == INVALID
    unchanged("set_sh_table on a closed-form encoder")
    np.testing.assert_allclose(before[-1].cpu().numpy(), O.encode(x.cpu().numpy(), w, Lp, "closed-form"), rtol=0, atol=2e-12)


# -- h. model level ----------------------------------------------------------------------------------------------
def test_model_lifecycle(tmp_path):
    """One load_model instance (constant-e-hat checkpoint, prepared bank of 4 099 rows, both heads at 43) serves
    batches of every size up and down, with the temperature, return_topk, sweep and the two result contracts
    changing in between: every call the exact expectation.  Then RANGE+ and RANGE interleaved in one process.
    (The expectation is the same at 43 and at 48: the calls at ``args.temp = 48`` show that the sharp route of a used
    context is exact, not that the attribute was read - test_temperatures_flip tells temperatures apart.)"""
    bank, c = L.exact(L.MODEL_N), L.FORWARD_CLASS
    (tmp_path / "plus").mkdir()
    (tmp_path / "range").mkdir()
    m = _model(tmp_path / "plus", bank, c, "RANGE+", BETA, prepared=True, temp=TAU, geo_temp=TAU)
    r = _model(tmp_path / "range", bank, c, "RANGE", None, prepared=True, temp=TAU)

    def call(B, i, model=m, beta=BETA, geo=True, **kw):
        q = X.forward_queries(bank, c, B, B)
        x = torch.from_numpy(X.lonlat_of(q.geo)).to(DEV)
        out = model(x, return_device=bool(i % 2), **kw)
        if kw:
            out, tv, ti = out
            _check_topk(tv, ti, bank, q, kw["return_topk"], 0, f"B={B} return_topk")
        _assert_rows(out, _fwd_want(bank, q, beta, geo), f"B={B} call {i} {kw}")
        return q, x

    sizes = L.MODEL_B + L.MODEL_B[::-1]
    for i, B in enumerate(sizes):
        q, x = call(B, i)
        if i % 5 == 1:
            m.args.temp = L.TAU_SHARP
            call(B, i + 1)
            m.args.temp = TAU
        if i % 5 == 2:
            call(B, i, return_topk=16)
        if i % 5 == 3:
            sw = m.sweep(x, list(L.MODEL_BETAS), return_device=True, temps=[TAU, L.TAU_SHARP])
            for ti in range(2):
                for bi, beta in enumerate(L.MODEL_BETAS):
                    _assert_rows(sw[ti, 0, bi], _fwd_want(bank, q, beta, True), f"B={B} sweep temp {ti} beta {beta}")
            sw = m.sweep(x, list(L.MODEL_BETAS))
            for bi, beta in enumerate(L.MODEL_BETAS):
                _assert_rows(sw[bi], _fwd_want(bank, q, beta, True), f"B={B} beta sweep {beta}")
    for i, B in enumerate((33, 4097, 5, 257, 17)):
        call(B, i)
        call(B, i + 1, model=r, beta=1.0, geo=False)
        call(B, i, return_topk=16)
        call(B, i, model=r, beta=1.0, geo=False, return_topk=16)
