"""GPU tests of the round-2 paths over ragged shapes: the host-array contract
(range_forward_host), the small-batch two-kernel encoder, the reference-faithful spherical
harmonics at several degrees, the persistent stream top-k on small / ragged banks."""
import os

import numpy as np
import pytest
import torch

from oracle import range_oracle as O
from range_amd import _native, sh_table
from tools import synth
from range_amd.bank import prepare_bank

pytestmark = pytest.mark.gpu


def _weights(L, H, layers, seed):
    w = synth.make_encoder_weights(L, H, 256, layers, seed)
    ws = [w[f"layers.{i}.weight"] for i in range(layers)] + [w["last_layer.weight"]]
    bs = [w[f"layers.{i}.bias"] for i in range(layers)] + [w["last_layer.bias"]]
    return w, ws, bs


@pytest.mark.parametrize("B", [1, 63, 64, 1000, 4095, 4096, 5001, 9000])
def test_forward_host_equals_device_result(B):
    """The host contract: same values as the device-resident result (bit-identical below the
    two-part threshold, split-order rounding above), caller's array rows filled exactly once."""
    N, L, H = 5000, 10, 64
    w, ws, bs = _weights(L, H, 2, 5)
    bank = prepare_bank(*synth.make_bank(N, 3))
    eng = _native.HipEngine("cuda:0")
    eng.set_encoder(L, H, 2, 256, _native.SH_ANALYTIC, ws, bs, sh_table=sh_table.generate_table(L))
    eng.set_bank(bank.keys, bank.values, bank.xyz)
    x = torch.from_numpy(synth.make_queries(B, seed=B, lat_max=90.0)).cuda()
    dev = eng.forward(x, _native.MODEL_RANGE_PLUS, 0.3).cpu().numpy()
    out = np.full((B + 2, 1280), -7.0)
    got = eng.forward_host(x, _native.MODEL_RANGE_PLUS, 0.3, out=out[1:-1])
    assert got.base is out or got is out[1:-1] or np.shares_memory(got, out)
    assert (out[0] == -7.0).all() and (out[-1] == -7.0).all()          # nothing beyond the rows given
    if B < 4096:
        assert np.array_equal(out[1:-1], dev)
    else:
        np.testing.assert_allclose(out[1:-1], dev, rtol=1e-5, atol=2e-6)
        assert np.array_equal(out[1:-1, 1024:], dev[:, 1024:])
    fresh = eng.forward_host(x, _native.MODEL_RANGE, 1.0)               # a pool array, RANGE model
    assert fresh.shape == (B, 1280) and fresh.dtype == np.float64 and fresh.flags.c_contiguous
    np.testing.assert_allclose(fresh, eng.forward(x, _native.MODEL_RANGE, 1.0).cpu().numpy(), rtol=1e-5, atol=2e-6)
    with pytest.raises(ValueError):
        eng.forward_host(x, _native.MODEL_RANGE, 1.0, out=np.zeros((B, 1280), np.float32))


@pytest.mark.parametrize("L,H,layers,mode", [(40, 512, 2, "analytic"), (40, 256, 2, "analytic"), (16, 128, 3, "analytic"),
                                             (10, 64, 2, "closed-form"), (33, 320, 2, "analytic"), (7, 192, 1, "analytic"),
                                             (40, 384, 2, "analytic")])
def test_small_batch_encoder_split_matches_one_kernel(L, H, layers, mode, monkeypatch):
    """Batches of up to 2048 queries run the encoder as (first layer per column part and K range) +
    [second layer per column part, from 32 tiles on] + (rest):
    same embeddings as the one-kernel encoder to float64 summation-order noise, for every width
    the split exists for (and unchanged behaviour for those it does not), in both SH evaluations."""
    w, ws, bs = _weights(L, H, layers, 11)
    sh = _native.SH_ANALYTIC if mode == "analytic" else _native.SH_CLOSED_FORM
    for table in ([None, sh_table.generate_table(L)] if mode == "analytic" else [None]):
        monkeypatch.setenv("RANGE_ENC_SPLIT", "0")
        one = _native.HipEngine("cuda:0")
        monkeypatch.delenv("RANGE_ENC_SPLIT")
        two = _native.HipEngine("cuda:0")
        for e in (one, two):
            e.set_encoder(L, H, layers, 256, sh, ws, bs, sh_table=table)
        for B in (1, 15, 16, 17, 250, 600, 1024, 2048, 2049, 3000):
            x = torch.from_numpy(synth.make_queries(B, seed=B + L, lat_max=90.0)).cuda()
            a64, a32, axq = one.encode(x)
            b64, b32, bxq = two.encode(x)
            assert float((a64 - b64).abs().max()) < 5e-13
            assert torch.equal(axq, bxq)
            raw1, raw2 = one.encode_raw(x), two.encode_raw(x)
            assert float((raw1 - raw2).abs().max()) < 5e-12 * max(1.0, float(raw1.abs().max()))
        if table is None:
            x = torch.from_numpy(synth.make_queries(300, seed=1, lat_max=89.0)).cuda()
            np.testing.assert_allclose(two.encode(x)[0].cpu().numpy(), O.encode(x.cpu().numpy(), w, L, mode),
                                       rtol=0, atol=2e-12)


@pytest.mark.parametrize("L", [1, 2, 5, 10, 16, 25, 33, 40])
def test_reference_sh_tables_of_other_degrees(L):
    """The generated-polynomial evaluation for any degree L <= 40 (the table of L is a prefix of
    the table of 40): the kernel agrees with the CPU evaluation of the same table, and - the
    polynomials being well-conditioned for small L - with the exact basis too."""
    H = 64
    w, ws, bs = _weights(L, H, 2, 3)
    table = sh_table.generate_table(L)
    eng = _native.HipEngine("cuda:0")
    eng.set_encoder(L, H, 2, 256, _native.SH_ANALYTIC, ws, bs, sh_table=table)
    q = synth.make_queries(700, seed=L, lat_max=90.0)
    e = eng.encode(torch.from_numpy(q).cuda())[0].cpu().numpy()
    ref = O.encode(q, w, L, features=O.sh_features_faithful(q, O.load_ylm_table(), L))   # (bitwise the reference's features)
    band = np.abs(q[:, 1]) <= 45
    assert np.abs(e - ref)[band].max() < 1e-7 and np.abs(e - ref).max() < (1e-9 if L <= 16 else 2e-3)
    if L <= 16:
        np.testing.assert_allclose(e, O.encode(q, w, L), rtol=0, atol=1e-9)


@pytest.mark.parametrize("N,B,k", [(1, 1, 1), (15, 16, 4), (16, 17, 16), (17, 31, 16), (4095, 32, 16), (4097, 33, 7),
                                   (16385, 64, 16), (100_003, 20, 16), (70_000, 160, 16), (1029, 96, 3)])
def test_stream_topk_ragged_banks(N, B, k, monkeypatch):
    """Persistent stream kernel on banks smaller than the grid, ragged last tiles, more than one
    supergroup of query groups: indices and values equal to the float64 oracle's - and, the two key
    forms sharing one scan body, the float32-key scan's equal to the default's bit for bit."""
    rng = np.random.default_rng(N + B)
    keys = rng.standard_normal((N, 256)).astype(np.float32)
    keys /= np.linalg.norm(keys, axis=1, keepdims=True)
    qs = rng.standard_normal((B, 256)).astype(np.float32)
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    eng, f32 = _topk_engines(monkeypatch, keys, np.zeros((N, 1024), np.float32), np.zeros((N, 3), np.float32), 1000)   # row offset
    e = torch.from_numpy(qs).cuda()
    tv, ti = eng.topk_stream(e, k)
    fv, fi = f32.topk_stream(e, k)
    assert torch.equal(ti, fi) and torch.equal(tv, fv)
    s64 = qs.astype(np.float64) @ keys.astype(np.float64).T
    kk = min(k, N)
    rv, ri = O.topk64(s64, kk)
    tv, ti = tv.cpu().numpy(), ti.cpu().numpy()
    np.testing.assert_allclose(tv[:, :kk], rv, rtol=0, atol=4e-7)
    bad = np.nonzero((ti[:, :kk] - 1000 != ri).any(axis=1))[0]
    for r in bad:      # f32 near-ties only
        assert np.all(np.abs(s64[r, ti[r, :kk] - 1000] - rv[r]) <= 4 * np.spacing(np.float32(1.0)))
    assert len(bad) <= max(1, B // 50)
    if N < k:
        assert (ti[:, N:] == -1).all()


def _topk_engines(monkeypatch, keys, vals, xyz, row_offset=0):
    """(engine with the default bf16-key prefilter, engine streaming the float32 keys)"""
    pre = _native.HipEngine("cuda:0")
    monkeypatch.setenv("RANGE_TOPKS_KEYS", "f32")
    f32 = _native.HipEngine("cuda:0")
    monkeypatch.delenv("RANGE_TOPKS_KEYS")
    for e in (pre, f32):
        e.set_bank(keys, vals, xyz, row_offset)
    return pre, f32


def test_topk_stream_bf16_prefilter_is_exact(monkeypatch):
    """range_topk_stream scans a bf16 copy of the keys and re-ranks the candidates within its error
    bound with the float32 chain: values and indices must be those of the float32 scan bit for bit,
    also where the bf16 rounding scrambles the order (a crowd of rows within 1e-4 of the k-th
    place), for un-normalised queries and keys (the bound scales with the norms), for every k, and
    where everything ties (fallback to the brute-force path)."""
    rng = np.random.default_rng(21)
    N, d = 30011, 256
    keys = rng.standard_normal((N, d)).astype(np.float32)
    keys /= np.linalg.norm(keys, axis=1, keepdims=True)
    q = rng.standard_normal((40, d)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    # a crowd around the 16th place of queries 0..7: 60 rows whose similarity to query b is
    # 0.5 + i * 2e-6 (differences far below the bf16 error of 2e-3, above float32 resolution)
    for b in range(8):
        rows = rng.choice(N, 60, replace=False)
        for i, r in enumerate(rows):
            u = rng.standard_normal(d).astype(np.float64)
            u -= u.dot(q[b].astype(np.float64)) * q[b]
            u /= np.linalg.norm(u)
            s = 0.5 + i * 2e-6
            keys[r] = (s * q[b] + np.sqrt(1 - s * s) * u).astype(np.float32)
    vals = np.zeros((N, 1024), np.float32)
    xyz = np.zeros((N, 3), np.float32)
    pre, f32 = _topk_engines(monkeypatch, keys, vals, xyz)
    for qs in (q, q[:16], q[:5], q * np.float32(3.7)):
        for k in (16, 7, 1):
            e = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
            av, ai = pre.topk_stream(e, k)
            bv, bi = f32.topk_stream(e, k)
            assert torch.equal(ai, bi) and torch.equal(av, bv)
    assert pre.topk_stream_exact_count() == 0          # the crowd fits the candidate lists: no fallback
    # the float32 scan itself against the float64 oracle (indices; values to float32 rounding)
    s64 = q.astype(np.float64) @ keys.astype(np.float64).T
    rv, ri = O.topk64(s64, 16)
    av, ai = pre.topk_stream(torch.from_numpy(q).cuda(), 16)
    np.testing.assert_allclose(av.cpu().numpy(), rv, rtol=0, atol=3e-7)
    same = (ai.cpu().numpy() == ri).all(axis=1)
    assert same[8:].all()                               # (inside the crowd float32 itself may swap neighbours 2e-6 apart)
    # keys of other norms: rows scaled by 0.25 .. 4
    scale = rng.uniform(0.25, 4.0, size=(N, 1)).astype(np.float32)
    pre2, f322 = _topk_engines(monkeypatch, keys * scale, vals, xyz)
    e = torch.from_numpy(q).cuda()
    av, ai = pre2.topk_stream(e, 16)
    bv, bi = f322.topk_stream(e, 16)
    assert torch.equal(ai, bi) and torch.equal(av, bv)
    # everything ties: 5000 copies of one row (more candidates than any list or buffer holds)
    same_keys = np.repeat(keys[:1], 5000, axis=0)
    pre3, f323 = _topk_engines(monkeypatch, same_keys, vals[:5000], xyz[:5000])
    av, ai = pre3.topk_stream(e[:3], 16)
    bv, bi = f323.topk_stream(e[:3], 16)
    assert torch.equal(ai, bi) and torch.equal(av, bv)
    assert ai.cpu().numpy().tolist() == [list(range(16))] * 3     # ties: lower rows first
    assert pre3.topk_stream_exact_count() == 3


@pytest.mark.parametrize("level", ["lanes", "waves"])
def test_topk_stream_drop_seen_by_every_merge_level(level):
    """The candidate lists are merged lane -> wave -> workgroup, each merge over shuffles between the
    4 lanes (j, g) of a query, and what a merge drops must reach the exactness check whichever of
    the 4 lanes saw it go.  'lanes': five of a query's best rows sit in lane groups 2 and 3 of ONE
    wave's tile (3 + 2: no lane list overflows, the pair merge of lanes (2,3) does when lists are 4
    deep).  'waves': ten of its best rows sit in waves 2 and 3 of ONE workgroup (5 + 5, one per
    lane list: the pair merge of waves (2,3) drops two of them).  Either way the result must be the
    oracle's - through the lists if they held everything, through the brute-force path otherwise."""
    rng = np.random.default_rng(5)
    N, d, k = 20000, 256, 16
    keys = rng.standard_normal((N, d)).astype(np.float32)
    keys /= np.linalg.norm(keys, axis=1, keepdims=True)
    q = rng.standard_normal((3, d)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)

    def plant(row, b, s):
        u = rng.standard_normal(d)
        u -= u.dot(q[b].astype(np.float64)) * q[b]
        u /= np.linalg.norm(u)
        keys[row] = (s * q[b] + np.sqrt(1 - s * s) * u).astype(np.float32)

    # rows of a 16-row tile held by lane group g (engine_prims.h: pi_row): g=0 {0,1,8,9}, g=1 {2,3,10,11},
    # g=2 {4,5,12,13}, g=3 {6,7,14,15}; wave w of workgroup 0 streams tile w * 256 first (256 workgroups)
    if level == "lanes":
        spots = [(0, 16 * 7 + r) for r in (4, 5, 12, 6, 7)]                      # tile 7: lanes g=2 (3 rows), g=3 (2)
    else:
        spots = [(0, 16 * (256 * w) + r) for w in (2, 3) for r in (0, 2, 4, 6, 8)]   # waves 2, 3 of workgroup 0
    for i, (b, row) in enumerate(spots):
        plant(row, b, 0.9 + 1e-3 * i)
    for mode in ("bf16", "f32"):
        if mode == "f32":
            os.environ["RANGE_TOPKS_KEYS"] = "f32"
        try:
            eng = _native.HipEngine("cuda:0")
        finally:
            os.environ.pop("RANGE_TOPKS_KEYS", None)
        eng.set_keys(keys)
        tv, ti = eng.topk_stream(torch.from_numpy(q).cuda(), k)
        s64 = q.astype(np.float64) @ keys.astype(np.float64).T
        rv, ri = O.topk64(s64, k)
        assert np.array_equal(ti.cpu().numpy(), ri), mode
        np.testing.assert_allclose(tv.cpu().numpy(), rv, rtol=0, atol=1e-6)     # f32 dot of 256 terms near 0.9


def test_keys_only_bank_serves_topk_and_nothing_else():
    """range_set_keys: the keys column alone (host array or device tensor) answers topk_stream like
    the full bank does; calls that need the values fail with RANGE_ERR_STATE."""
    rng = np.random.default_rng(9)
    N = 5003
    keys = rng.standard_normal((N, 256)).astype(np.float32)
    keys /= np.linalg.norm(keys, axis=1, keepdims=True)
    q = torch.from_numpy(keys[rng.integers(0, N, 40)] + 0.1 * rng.standard_normal((40, 256)).astype(np.float32)).cuda()
    full = _native.HipEngine("cuda:0")
    full.set_bank(keys, np.zeros((N, 1024), np.float32), np.zeros((N, 3), np.float32), 77)
    fv, fi = full.topk_stream(q, 16)
    for src in (keys, torch.from_numpy(keys).cuda()):
        eng = _native.HipEngine("cuda:0")
        eng.set_keys(src, 77)
        tv, ti = eng.topk_stream(q, 16)
        assert torch.equal(ti, fi) and torch.equal(tv, fv)
        with pytest.raises(_native.RangeNativeError, match="keys-only"):
            eng.scan_stats(q, torch.zeros((40, 4), device="cuda"), 12.0, 0.0)


def test_unnormalised_bank_is_refused_by_the_softmax():
    """The constant-shift softmax statistics need unit keys (range/range.py:85-89 normalises them);
    a bank that skipped it is refused by scan_stats / attend instead of overflowing (advice r2)."""
    rng = np.random.default_rng(2)
    N = 300
    keys = rng.standard_normal((N, 256)).astype(np.float32)          # norms ~16
    eng = _native.HipEngine("cuda:0")
    eng.set_bank(keys, np.zeros((N, 1024), np.float32), np.zeros((N, 3), np.float32))
    q = torch.nn.functional.normalize(torch.randn(8, 256), dim=1).cuda()
    with pytest.raises(_native.RangeNativeError, match="not L2-normalised"):
        eng.scan_stats(q, torch.zeros((8, 4), device="cuda"), 12.0, 0.0)
    tv, ti = eng.topk_stream(q, 4)                                     # the top-k takes any norm
    s64 = q.cpu().numpy().astype(np.float64) @ keys.astype(np.float64).T
    assert np.array_equal(ti.cpu().numpy(), O.topk64(s64, 4)[1])


@pytest.mark.parametrize("L,H,layers,mode,Bs", [
    (10, 768, 2, "analytic", (5, 300, 5000)),
    (10, 1024, 2, "closed-form", (1, 16, 700, 4500)),
    (40, 1024, 2, "analytic", (40, 2100)),
    (16, 1024, 3, "analytic", (33,)),
])
def test_encoder_wide_hidden_layers(L, H, layers, mode, Bs):
    """`capacity` of the real checkpoint is unknown: hidden widths beyond 512 - 768
    and 1024 - run 16-query workgroups whose activations are packed densely in LDS (16 x H float64).
    Every batch geometry: one kernel, the small-batch split kernels, many rounds; both SH evaluations
    (the exact recurrence against the float64 oracle; the reference's polynomials against their CPU
    evaluation through the same Siren)."""
    w, ws, bs = _weights(L, H, layers, 12)
    smode = _native.SH_ANALYTIC if mode == "analytic" else _native.SH_CLOSED_FORM
    exact = _native.HipEngine("cuda:0")
    exact.set_encoder(L, H, layers, 256, smode, ws, bs)
    engines = [(exact, None)]
    if mode == "analytic":
        tab = sh_table.generate_table(L)
        faithful = _native.HipEngine("cuda:0")
        faithful.set_encoder(L, H, layers, 256, smode, ws, bs, sh_table=tab)
        engines.append((faithful, tab))
    for B in Bs:
        q = synth.make_queries(B, seed=B, lat_max=40.0)
        x = torch.from_numpy(q).cuda()
        for eng, tab in engines:
            e64, e32, xq = eng.encode(x)
            ref = (O.encode(q, w, L, mode) if tab is None else
                   O.encode(q, w, L, features=O.sh_features_faithful(q, O.load_ylm_table(), L)))
            np.testing.assert_allclose(e64.cpu().numpy(), ref, rtol=0, atol=4e-12 if tab is None else 2e-7)
            np.testing.assert_array_equal(e32.cpu().numpy(), e64.cpu().numpy().astype(np.float32))
            raw = eng.encode_raw(x).cpu().numpy()
            np.testing.assert_allclose(raw / np.linalg.norm(raw, axis=1, keepdims=True), e64.cpu().numpy(), rtol=0, atol=1e-13)
    with pytest.raises(_native.RangeNativeError, match="unsupported"):
        bad = _native.HipEngine("cuda:0")
        wb, wsb, bsb = _weights(10, 1088, 2, 1)
        bad.set_encoder(10, 1088, 2, 256, _native.SH_ANALYTIC, wsb, bsb)


@pytest.mark.parametrize("H", [100, 576, 640, 704, 832, 896, 960, 1000])
def test_hidden_widths_between_the_kernels_run_zero_padded(H):
    """`capacity` of the real checkpoint is unknown: ANY hidden width up to 1024 loads.  Widths no
    kernel exists for run as the next one that has (multiples of 64 up to 512, 768, 1024) with
    zero-padded weights - a padded unit is sin(0) = 0 feeding zero weights, every product it adds an
    exact +0.0 - and equal the float64 oracle of the UNPADDED network like every other width."""
    L = 12
    w, ws, bs = _weights(L, H, 2, 30 + H)
    eng = _native.HipEngine("cuda:0")
    eng.set_encoder(L, H, 2, 256, _native.SH_CLOSED_FORM, ws, bs)
    for B in (7, 300, 5000):
        q = synth.make_queries(B, seed=B + H, lat_max=89.0)
        e64, e32, xq = eng.encode(torch.from_numpy(q).cuda())
        np.testing.assert_allclose(e64.cpu().numpy(), O.encode(q, w, L, "closed-form"), rtol=0, atol=4e-12)
        np.testing.assert_array_equal(e32.cpu().numpy(), e64.cpu().numpy().astype(np.float32))


@pytest.mark.parametrize("N", [9, 1000, 20011])
def test_small_batches_take_one_pass_over_the_bank(N, monkeypatch):
    """Up to 32 queries run attend_small_kernel (one or two tiles of 16 queries per workgroup; every CU streams its share of keys, locations and
    values ONCE and accumulates the un-normalised products of both heads) + small_finalize_kernel:
    against the float64 oracle and the reference's float32 op order, RANGE and RANGE+, several beta,
    banks that do not fill a 16-row block or have fewer blocks than CUs; the two-pass kernels
    (RANGE_SMALL_FORWARD=0) agree to float32 rounding; 33 queries take the two-pass route."""
    L, H = 10, 64
    w, ws, bs = _weights(L, H, 2, 5)
    locs, vals, keys = synth.make_bank(N, 3)
    vals = vals.copy()
    vals[:, 0] = 1.0                       # a constant column: reproduced iff the weights sum to one
    bank = prepare_bank(locs, vals, keys)
    obank = O.prep_bank(locs, vals, keys)
    eng = _native.HipEngine("cuda:0")
    monkeypatch.setenv("RANGE_SMALL_FORWARD", "0")
    two = _native.HipEngine("cuda:0")
    monkeypatch.delenv("RANGE_SMALL_FORWARD")
    for e in (eng, two):
        e.set_encoder(L, H, 2, 256, _native.SH_ANALYTIC, ws, bs)
        e.set_bank(bank.keys, bank.values, bank.xyz)
    for B in (1, 5, 16, 17, 29, 32, 33):
        q = synth.make_queries(B, seed=N + B, lat_max=80.0)
        x = torch.from_numpy(q).cuda()
        for model, name, beta in ((_native.MODEL_RANGE_PLUS, "RANGE+", 0.5), (_native.MODEL_RANGE_PLUS, "RANGE+", 0.0),
                                  (_native.MODEL_RANGE_PLUS, "RANGE+", 1.0), (_native.MODEL_RANGE, "RANGE", 1.0)):
            eng.profile_enable(True)
            out = eng.forward(x, model, beta).cpu().numpy()
            assert eng.profile_read(_native.PROF_SCAN_STATS)[1] == (0 if B <= 32 else 1)   # which route ran: no pass 1
            eng.profile_enable(False)
            ref64 = O.retrieve64(out[:, 1024:], q, obank, name, beta)
            np.testing.assert_allclose(out[:, :1024], ref64, rtol=0, atol=2e-5)
            np.testing.assert_allclose(out, O.retrieve(out[:, 1024:], q, obank, name, beta), rtol=0, atol=1e-4)
            assert np.abs(out[:, 0] - 1.0).max() < 2e-6
            np.testing.assert_allclose(out[:, 1024:], O.encode(q, w, L), rtol=0, atol=2e-12)
            other = two.forward(x, model, beta).cpu().numpy()
            np.testing.assert_allclose(out, other, rtol=0, atol=3e-6)
            host = eng.forward_host(x, model, beta)                            # the numpy contract, same route
            assert np.array_equal(host, out)


def test_in_launch_handoffs_under_repetition(monkeypatch):
    """The two kernels that hand data between workgroups INSIDE a launch - the top-k stream kernel
    (candidate lists -> the merging workgroups; self-resetting sharded counters) and the one-tile
    encoder (five phases meeting at wrap-around counters) - run hundreds of times back to back with
    changing batch sizes and queries, each result compared with the same computation done as
    separate launches (RANGE_TOPKS_FUSED=0 / RANGE_ENC_FUSED=0): a counter left non-zero, a stale
    line or a lost increment shows as a wrong row or a hang (bounded spins: it would show as -1 / NaN
    rows and an error from topk_stream_exact_count)."""
    rng = np.random.default_rng(77)
    N = 40_000
    keys = rng.standard_normal((N, 256)).astype(np.float32)
    keys /= np.linalg.norm(keys, axis=1, keepdims=True)
    L, H = 10, 128
    w, ws, bs = _weights(L, H, 2, 3)
    fused = _native.HipEngine("cuda:0")
    monkeypatch.setenv("RANGE_TOPKS_FUSED", "0")
    monkeypatch.setenv("RANGE_ENC_FUSED", "0")
    apart = _native.HipEngine("cuda:0")
    monkeypatch.delenv("RANGE_TOPKS_FUSED")
    monkeypatch.delenv("RANGE_ENC_FUSED")
    for e in (fused, apart):
        e.set_keys(keys)
        e.set_encoder(L, H, 2, 256, _native.SH_ANALYTIC, ws, bs)
    g = torch.Generator(device="cuda").manual_seed(5)
    sizes = (1, 16, 40, 200, 256, 300, 7, 64)
    for it in range(240):
        B = sizes[it % len(sizes)]
        q = torch.nn.functional.normalize(torch.randn((B, 256), generator=g, device="cuda"), dim=1).contiguous()
        k = (16, 5, 1)[it % 3]
        av, ai = fused.topk_stream(q, k)
        bv, bi = apart.topk_stream(q, k)
        assert torch.equal(ai, bi) and torch.equal(av, bv), (it, B, k)
        nq = 1 + (it * 23) % 530                      # 1 .. 530 queries: one to 32 tiles in one launch, and beyond
        x = torch.stack([torch.rand(nq, generator=g, device="cuda", dtype=torch.float64) * 360 - 180,
                         torch.rand(nq, generator=g, device="cuda", dtype=torch.float64) * 170 - 85], dim=1).contiguous()
        e1 = fused.encode(x)
        e2 = apart.encode(x)
        assert float((e1[0] - e2[0]).abs().max()) < 1e-12 and torch.equal(e1[2], e2[2]), (it, nq)
    assert fused.topk_stream_exact_count() == apart.topk_stream_exact_count()


@pytest.mark.parametrize("L,H", [(10, 128), (12, 192), (40, 256), (20, 320), (40, 512), (16, 448)])
def test_one_tile_encoder_over_widths(L, H):
    """encoder_tile_kernel (one persistent launch for up to 8 tiles of 16 queries) over hidden widths
    whose phases need different numbers of workgroups (activation 2..8, second layer 2..8, last layer 4)."""
    w, ws, bs = _weights(L, H, 2, 21)
    eng = _native.HipEngine("cuda:0")
    eng.set_encoder(L, H, 2, 256, _native.SH_CLOSED_FORM, ws, bs)
    for B in (1, 9, 16, 17, 50, 128, 300, 512):
        q = synth.make_queries(B, seed=B + H, lat_max=85.0)
        e64, e32, xq = eng.encode(torch.from_numpy(q).cuda())
        np.testing.assert_allclose(e64.cpu().numpy(), O.encode(q, w, L, "closed-form"), rtol=0, atol=2e-12)
        np.testing.assert_allclose(xq.cpu().numpy()[:, :3], O.query_xyz(q), rtol=0, atol=1.2e-7)


def test_a_given_up_in_kernel_wait_poisons_that_call_and_falls_back():
    """The persistent launches' waits between workgroups are bounded; one that gives up (test hook:
    the NEXT persistent launch behaves as if its wait had expired - the kernel's real give-up path)
    (i) leaves NaN in THAT call's output rows (never stale memory), (ii) is reported by the next look
    - entry of the next call, the synchronous numpy contract before it returns, check_async_error
    behind a caller's own synchronisation - and (iii) switches the context to the separate-launch
    path: the same call re-issued succeeds and equals the oracle (include/range_hip.h at range_encode)."""
    L, H, N = 20, 256, 500          # (a shape whose small batches take the one-launch encoder)
    w, ws, bs = _weights(L, H, 2, 5)
    eng = _native.HipEngine("cuda:0")
    eng.set_encoder(L, H, 2, 256, _native.SH_ANALYTIC, ws, bs)
    locs, vals, keys = synth.make_bank(N, 3)
    bank = prepare_bank(locs, vals, keys)
    obank = O.prep_bank(locs, vals, keys)
    eng.set_bank(bank.keys, bank.values, bank.xyz)
    q = synth.make_queries(40, seed=1)
    x = torch.from_numpy(q).cuda()
    ref = O.forward(q, w, L, obank, "RANGE+", 0.5)
    good = eng.forward(x, _native.MODEL_RANGE_PLUS, 0.5).cpu().numpy()
    np.testing.assert_allclose(good, ref, rtol=0, atol=2e-5)
    eng.check_async_error()                                  # nothing to report
    # ---- the device-resident path: the failed call returns OK (nothing has synchronised yet) ...
    eng.debug_fail_next_persistent_launch()
    e64, e32, xq = eng.encode(x)
    torch.cuda.synchronize()
    # ... but every row it could not finish is NaN, in every output
    assert bool(torch.isnan(e64).all()) and bool(torch.isnan(e32).all()) and bool(torch.isnan(xq).all())
    with pytest.raises(_native.RangeNativeError, match="gave up waiting"):
        eng.check_async_error()
    eng.check_async_error()                                  # reported once
    # the same call re-issued: the separate-launch path from now on, the oracle's rows
    e64b, _, _ = eng.encode(x)
    np.testing.assert_allclose(e64b.cpu().numpy(), ref[:, 1024:], rtol=0, atol=2e-12)
    np.testing.assert_allclose(eng.forward(x, _native.MODEL_RANGE_PLUS, 0.5).cpu().numpy(), ref, rtol=0, atol=2e-5)
    # ---- the fused top-k tail: NaN values / index -1 for that call, reported, then the two-launch form
    eng2 = _native.HipEngine("cuda:0")
    eng2.set_encoder(L, H, 2, 256, _native.SH_ANALYTIC, ws, bs)
    eng2.set_bank(bank.keys, bank.values, bank.xyz)
    _, e32g, _ = eng2.encode(x)
    e32g = e32g[:8].contiguous()                             # (one query per stream workgroup: the fused form; 500 rows = 8 workgroups)
    tv0, ti0 = eng2.topk_stream(e32g, 8)
    rv, ri = O.topk64(O.logits64(ref[:8, 1024:], q[:8], obank)[0], 8)
    assert np.array_equal(ti0.cpu().numpy(), ri)
    eng2.debug_fail_next_persistent_launch()
    tv, ti = eng2.topk_stream(e32g, 8)
    torch.cuda.synchronize()
    assert bool(torch.isnan(tv).all()) and bool((ti == -1).all())
    with pytest.raises(_native.RangeNativeError, match="top-k launch"):
        eng2.topk_stream(e32g, 8)                            # entry of the next call
    for _ in range(3):                                       # the fall-back, and the counters of later calls are sound
        tv2, ti2 = eng2.topk_stream(e32g, 8)
        assert torch.equal(ti2, ti0) and torch.equal(tv2, tv0)
    # ---- the numpy contract: the call in flight refuses itself before handing out rows
    eng3 = _native.HipEngine("cuda:0")
    eng3.set_encoder(L, H, 2, 256, _native.SH_ANALYTIC, ws, bs)
    eng3.set_bank(bank.keys, bank.values, bank.xyz)
    eng3.debug_fail_next_persistent_launch()
    with pytest.raises(_native.RangeNativeError, match="gave up waiting"):
        eng3.forward_host(x, _native.MODEL_RANGE_PLUS, 0.5)
    np.testing.assert_allclose(eng3.forward_host(x, _native.MODEL_RANGE_PLUS, 0.5), ref, rtol=0, atol=2e-5)


def test_fused_topk_counters_survive_many_calls_and_batch_sizes():
    """The fused tail's arrival counters only count up and the host tracks their base: calls of
    different batch sizes (different numbers of merging workgroups), back to back, never disagree
    with the two-launch form."""
    rng = np.random.default_rng(5)
    keys = rng.standard_normal((20011, 256)).astype(np.float32)
    keys /= np.linalg.norm(keys, axis=1, keepdims=True)
    eng = _native.HipEngine("cuda:0")
    eng.set_keys(keys)
    os.environ["RANGE_TOPKS_FUSED"] = "0"
    try:
        ref_eng = _native.HipEngine("cuda:0")
    finally:
        os.environ.pop("RANGE_TOPKS_FUSED", None)
    ref_eng.set_keys(keys)
    for i, B in enumerate((1, 16, 7, 64, 255, 3, 33, 256, 16, 16, 16, 100)):
        e = torch.from_numpy(rng.standard_normal((B, 256)).astype(np.float32)).cuda()
        e = torch.nn.functional.normalize(e, dim=1).contiguous()
        tv, ti = eng.topk_stream(e, 16)
        rv, ri = ref_eng.topk_stream(e, 16)
        assert torch.equal(ti, ri) and torch.equal(tv, rv), (i, B)
    eng.check_async_error()


def test_topk_stream_on_a_dram_sized_bank():
    """The scan at the size its roofline entry is quoted on (N = 10^6 keys, 512 MB as bf16: streamed
    from DRAM, 61 rounds of tiles per wave): indices equal a float64 top-k for 1 .. 5 passes and over
    supergroups, call after call (the fused tail's ticket counters only count up)."""
    N = 1_000_000
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(N)
    keys = torch.randn((N, 256), generator=g, device=dev, dtype=torch.float32)
    cent = torch.randn((32, 256), generator=g, device=dev, dtype=torch.float32)
    keys += 3.0 * cent[torch.randint(0, 32, (N,), generator=g, device=dev)]
    keys = torch.nn.functional.normalize(keys, dim=1).contiguous()
    eng = _native.HipEngine(dev)
    eng.set_keys(keys)
    for rep, B in enumerate((16, 1, 40, 32, 130, 64, 16, 256)):
        e = torch.nn.functional.normalize(
            keys[torch.randint(0, N, (B,), generator=g, device=dev)] + 0.5 * torch.randn((B, 256), generator=g, device=dev),
            dim=1).contiguous()
        tv, ti = eng.topk_stream(e, 16)
        rv, ri = torch.topk(e.double() @ keys.double().T, 16, dim=1)
        # (float32 near-ties may swap against float64: at most one query of a batch)
        assert int((ti != ri).any(dim=1).sum()) <= 1, (rep, B)
        assert float((tv - rv.float()).abs().max()) < 3e-7
    eng.check_async_error()


def test_scan_stats_at_chunks_share_one_workspace():
    """range_scan_stats_at (pass 1 in chunks of one scan, range_amd/dist.py): chunks called in order keep
    their logits at their offsets of ONE workspace - pass 2 on them equals pass 2 behind a single
    range_scan_stats bit for bit when every chunk uses the same bank splits, and a query's statistics do
    not depend on the chunking; out of order, or past what the first chunk could keep, nothing is kept
    but the statistics are still right; bad offsets are refused."""
    L, H, N, B = 10, 64, 5003, 448
    w, ws, bs = _weights(L, H, 2, 9)
    locs, vals, keys = synth.make_bank(N, 4)
    bank = prepare_bank(locs, vals, keys)
    eng = _native.HipEngine("cuda:0")
    eng.set_encoder(L, H, 2, 256, _native.SH_ANALYTIC, ws, bs)
    eng.set_bank(bank.keys, bank.values, bank.xyz)
    x = torch.from_numpy(synth.make_queries(B, seed=2)).cuda()
    e64, e32, xq = eng.encode(x)
    S = eng.p1_splits(192)
    assert S >= 1
    # one call over everything, with the chunks' split count
    st_all = eng.scan_stats_at(e32, xq, 12.0, 40.0, 0, B, n_splits=S)
    assert eng.kept_queries() == B
    # three chunks (192 + 128 + 128 queries); pass 2 runs per chunk in both cases (its own split count
    # follows its launch's geometry, so it is compared chunk by chunk)
    cuts = [(0, 192), (192, 320), (320, 448)]
    ref = torch.cat([eng.attend_kept(lo, xq[lo:hi].contiguous(), 12.0, 40.0, 0.5, st_all[lo:hi].contiguous()) for lo, hi in cuts])
    sts = [eng.scan_stats_at(e32[lo:hi].contiguous(), xq[lo:hi].contiguous(), 12.0, 40.0, lo, B, n_splits=S)
           for lo, hi in cuts]
    assert eng.kept_queries() == B
    st = torch.cat(sts)
    assert torch.equal(st, st_all)                                         # a query's statistics: chunking-free
    out = torch.cat([eng.attend_kept(lo, xq[lo:hi].contiguous(), 12.0, 40.0, 0.5, st[lo:hi].contiguous()) for lo, hi in cuts])
    assert torch.equal(out, ref)
    # ... and equal to recomputing the logits (range_attend), as ever
    rec = torch.cat([eng.attend(e32[lo:hi].contiguous(), xq[lo:hi].contiguous(), 12.0, 40.0, 0.5, st_all[lo:hi].contiguous())
                     for lo, hi in cuts])
    assert torch.equal(rec, ref)
    # out of order: a later chunk without the first - statistics right, nothing kept
    eng.scan_stats(e32[:64].contiguous(), xq[:64].contiguous(), 12.0, 40.0)                  # (forgets the scan)
    s2 = eng.scan_stats_at(e32[192:320].contiguous(), xq[192:320].contiguous(), 12.0, 40.0, 192, B, n_splits=S)
    assert eng.kept_queries() == 0 and torch.equal(s2, st_all[192:320])
    with pytest.raises(_native.RangeNativeError, match="kept"):
        eng.attend_kept(192, xq[192:320].contiguous(), 12.0, 40.0, 0.5, s2)
    # a scan restarted with another total is a new scan
    eng.scan_stats_at(e32[:192].contiguous(), xq[:192].contiguous(), 12.0, 40.0, 0, 192, n_splits=S)
    assert eng.kept_queries() == 192
    eng.scan_stats_at(e32[192:320].contiguous(), xq[192:320].contiguous(), 12.0, 40.0, 192, B, n_splits=S)
    assert eng.kept_queries() == 0
    for first, total in ((32, B), (-64, B), (384, 400)):                   # not a tile boundary / negative / past the scan
        with pytest.raises(_native.RangeNativeError):
            eng.scan_stats_at(e32[:64].contiguous(), xq[:64].contiguous(), 12.0, 40.0, first, total)
    # a context that never keeps (RANGE_KEEP_LOGITS=0): statistics only
    os.environ["RANGE_KEEP_LOGITS"] = "0"
    try:
        nk = _native.HipEngine("cuda:0")
    finally:
        os.environ.pop("RANGE_KEEP_LOGITS", None)
    nk.set_encoder(L, H, 2, 256, _native.SH_ANALYTIC, ws, bs)
    nk.set_bank(bank.keys, bank.values, bank.xyz)
    s3 = nk.scan_stats_at(e32, xq, 12.0, 40.0, 0, B, n_splits=S)
    assert nk.kept_queries() == 0 and torch.equal(s3, st_all)
