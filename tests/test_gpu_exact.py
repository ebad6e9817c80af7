"""Bit-exact row accounting of every retrieval route, at the bank and batch sizes where the launch
geometry varies (bank splits, the stream-K walk and its columns, chunked scans, kept-logit
sub-ranges, shards, the host contract's part cuts, the one-pass path, 10^6 rows).

The banks (tools/exact_bank.py) have answers that are exactly float32 numbers: one-hot keys and
axis locations make every similarity 1, 0 or -1, queried classes have power-of-two sizes and the
values are 1 or 2, so the in-class weights are short binary fractions and the out-of-class mass
rounds away at every addition.  A correct kernel returns the expectation bit for bit whatever its
summation order; a dropped, doubled or misplaced row, block, part or query changes the result by at
least one in-class term.  Every check here is ``torch.equal``.
"""
import functools

import numpy as np
import pytest
import torch

from exact_helpers import DEV, _assert_equal, _assert_rows, _dev, _env, _fwd_queries, _fwd_want, _model
from range_amd import _native
from tools import exact_bank as X

pytestmark = pytest.mark.gpu
TAU = X.TAU


@functools.lru_cache(maxsize=None)
def _bank(n, seed=0, sem_cap=1 << 14):
    return X.build(n, seed=seed, sem_cap=sem_cap)


_ENGINES = {}


def _engine(n, seed=0, sem_cap=1 << 14, lo=0, hi=None, **env):
    """An engine holding rows [lo, hi) of the bank (row_offset lo), created under ``env``."""
    key = (n, seed, sem_cap, lo, hi, tuple(sorted(env.items())))
    if key not in _ENGINES:
        b = _bank(n, seed, sem_cap)
        with _env(**env):
            eng = _native.HipEngine(DEV)
        eng.set_bank(*b.rows(lo, n if hi is None else hi), row_offset=lo)
        _ENGINES[key] = eng
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _release_engines():
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()
    torch.cuda.empty_cache()


def _check_stats(st, bank, q, geo, what):
    want = _dev(X.expect_stats(bank, q))
    _assert_equal(st[:, :2], want[:, :2], f"{what}: m_sem, l_sem")
    if geo:
        _assert_equal(st[:, 2:], want[:, 2:], f"{what}: m_geo, l_geo")


def _setup(n, B, beta, geo, seed=0, sem_cap=1 << 14):
    bank = _bank(n, seed, sem_cap)
    q = X.queries(bank, B, seed=B)
    X.assert_bank_margin(bank, q, beta, TAU, TAU if geo else 0.0)
    if B >= bank.n_classes:
        assert X.covered(bank, q)
    want = _dev(X.expect(bank, q, beta, geo))
    return bank, q, _dev(q.e32), _dev(q.xq), want


# -- premise ------------------------------------------------------------------------------------
def test_premise_statistics_exact():
    """The construction's premise on the hardware: m = f32(43 log2 e) and l = the class size,
    bit for bit (v_exp_f32 of 0 is 1, the out-of-class terms round away)."""
    bank, q, e32, xq, _ = _setup(4099, 64, 0.5, True)
    st = _engine(4099).scan_stats(e32, xq, TAU, TAU)
    _check_stats(st, bank, q, True, "scan_stats")


# -- engine level: statistics, pass 2 recompute / kept / sub-ranges ------------------------------
# (N, B, beta, geo head): stream-K for N <= 50 000, bank splits above; B across tile edges
ENGINE_CASES = [
    (1, 1, 0.5, True), (15, 16, 0.5, True), (17, 17, 0.25, True), (4099, 32, 0.75, True),
    (4099, 33, 1.0, True), (12500, 64, 0.0, True), (12500, 65, 0.5, True), (16385, 257, 0.25, True),
    (16385, 1250, 1.0, False), (50000, 4096, 0.75, True), (50000, 4097, 0.5, True),
    (50001, 10000, 0.25, True), (100000, 10000, 0.5, True), (100003, 16385, 0.75, True),
]


@pytest.mark.parametrize("n,B,beta,geo", ENGINE_CASES)
def test_engine_exact(n, B, beta, geo):
    bank, q, e32, xq, want = _setup(n, B, beta, geo)
    eng = _engine(n)
    tg = TAU if geo else 0.0
    st = eng.scan_stats(e32, xq, TAU, tg, keep_logits=True)
    _check_stats(st, bank, q, geo, "scan_stats")
    assert eng.kept_queries() == B
    _assert_equal(eng.attend_kept(0, xq, TAU, tg, beta, st), want, "attend_kept")
    if (n, B) == (100000, 10000):
        assert eng.last_geometry() == (157, 13)      # the benchmark's pass-2 launch
    _assert_equal(eng.attend(e32, xq, TAU, tg, beta, st), want, "attend")
    if B > 128:                                       # a sub-range of the kept scan
        a = 64 * (B // 3 // 64 + 1)
        b = min(B, a + 64 * (B // 5 // 64) + 37)
        _assert_equal(eng.attend_kept(a, xq[a:b], TAU, tg, beta, st[a:b].contiguous()), want[a:b],
                      f"attend_kept [{a},{b})")


@pytest.mark.parametrize("n,B,beta", [(4099, 33, 0.5), (12500, 257, 0.25), (50000, 4097, 0.75)])
def test_split_scheme_exact(n, B, beta):
    """RANGE_P2_STREAMK=0: the split scheme on banks the stream-K walk would take."""
    bank, q, e32, xq, want = _setup(n, B, beta, True)
    eng = _engine(n, RANGE_P2_STREAMK=0)
    st = eng.scan_stats(e32, xq, TAU, TAU, keep_logits=True)
    _check_stats(st, bank, q, True, "scan_stats")
    _assert_equal(eng.attend_kept(0, xq, TAU, TAU, beta, st), want, "attend_kept (splits)")
    _assert_equal(eng.attend(e32, xq, TAU, TAU, beta, st), want, "attend (splits)")


@pytest.mark.parametrize("n,B,beta", [(16385, 1250, 0.5), (100003, 300, 0.25)])
def test_no_kept_logits_exact(n, B, beta):
    bank, q, e32, xq, want = _setup(n, B, beta, True)
    eng = _engine(n, RANGE_KEEP_LOGITS=0)
    st = eng.scan_stats(e32, xq, TAU, TAU, keep_logits=True)
    assert eng.kept_queries() == 0
    _check_stats(st, bank, q, True, "scan_stats")
    _assert_equal(eng.attend(e32, xq, TAU, TAU, beta, st), want, "attend (nothing kept)")


@pytest.mark.parametrize("n,B,beta", [(50000, 4096, 1.0), (100000, 1000, 0.0), (12500, 300, 1.0)])
def test_bf16x3_exact(n, B, beta):
    """pv_mode bf16x3 on kept logits: single power-of-two weights sit in the high plane exactly."""
    bank, q, e32, xq, want = _setup(n, B, beta, True, seed=1)
    eng = _engine(n, seed=1)                          # (an engine of its own: the mode is per context)
    eng.set_pv_mode("bf16x3")
    try:
        st = eng.scan_stats(e32, xq, TAU, TAU, keep_logits=True)
        assert eng.kept_queries() == B
        _assert_equal(eng.attend_kept(0, xq, TAU, TAU, beta, st), want, "attend_kept bf16x3")
    finally:
        eng.set_pv_mode("exact")


@pytest.mark.parametrize("n", [12500, 50001])
@pytest.mark.parametrize("n_splits", [1, 7, 0])
def test_chunked_scan_exact(n, n_splits):
    B, cuts = 1000, [0, 320, 640, 1000]
    bank, q, e32, xq, want = _setup(n, B, 0.5, True)
    eng = _engine(n)
    sts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        st = eng.scan_stats_at(e32[a:b], xq[a:b], TAU, TAU, a, B, n_splits)
        assert eng.kept_queries() == b
        sts.append(st)
    st = torch.cat(sts)
    _check_stats(st, bank, q, True, f"scan_stats_at (n_splits={n_splits})")
    for a, b in zip(cuts[:-1], cuts[1:]):
        _assert_equal(eng.attend_kept(a, xq[a:b], TAU, TAU, 0.5, st[a:b].contiguous()), want[a:b],
                      f"attend_kept chunk [{a},{b}) n_splits={n_splits}")


@pytest.mark.parametrize("n,cuts,B", [(12500, [0, 5001, 12500], 700), (50001, [0, 16383, 33339, 50001], 4097)])
def test_shards_exact(n, cuts, B):
    """Row-sharded bank (row_offset at non-multiples of 16): merge_stats, per-shard attend,
    finalize; and the top-k side channel through merge_topk."""
    bank, q, e32, xq, want = _setup(n, B, 0.75, True)
    engs = [_engine(n, lo=a, hi=b) for a, b in zip(cuts[:-1], cuts[1:])]
    k = 16
    outs = [e.scan_stats(e32, xq, TAU, TAU, topk=k) for e in engs]
    st = engs[0].merge_stats(torch.stack([o[0] for o in outs]).contiguous())
    _check_stats(st, bank, q, True, "merge_stats")
    parts = torch.stack([e.attend(e32, xq, TAU, TAU, 0.75, st) for e in engs]).contiguous()
    e64 = e32.double()
    out = engs[0].finalize(parts, e64)
    _assert_equal(out[:, :1024], want.double(), "finalize of shard partials")
    assert torch.equal(out[:, 1024:], e64)
    tv, ti = engs[0].merge_topk(torch.stack([o[1] for o in outs]).contiguous(),
                                torch.stack([o[2] for o in outs]).contiguous())
    wv, wi = X.topk_expect(bank, q, k)
    _assert_equal(ti, _dev(wi), "merge_topk indices")
    _assert_equal(tv, _dev(wv), "merge_topk values")


def test_position_independence():
    """Every query of one class returns the same bits, at every position of a stream-K batch and
    alone."""
    n, B = 50000, 4097
    bank = _bank(n)
    q = X.queries(bank, B, seed=5)
    q.sem[:], q.geo[:] = q.sem[0], q.geo[0]
    q.e32[:], q.xq[:] = q.e32[0], q.xq[0]
    eng = _engine(n)
    e32, xq = _dev(q.e32), _dev(q.xq)
    st = eng.scan_stats(e32, xq, TAU, TAU, keep_logits=True)
    out = eng.attend_kept(0, xq, TAU, TAU, 0.5, st)
    assert torch.equal(out, out[:1].expand_as(out))
    st1 = eng.scan_stats(e32[:1], xq[:1], TAU, TAU)
    assert torch.equal(eng.attend(e32[:1], xq[:1], TAU, TAU, 0.5, st1), out[:1])
    _assert_equal(out, _dev(X.expect(bank, q, 0.5)), "one class everywhere")


def test_million_rows_exact():
    """10^6 rows, 4 096 queries: kept-logit tile offsets past 2^31 floats."""
    n, B = 1_000_000, 4096
    eb, keys, values, xyz = X.build_device(n, DEV, seed=3)
    eng = _native.HipEngine(DEV)
    try:
        eng.set_bank(keys.cpu().numpy(), values.cpu().numpy(), xyz.cpu().numpy())
        del keys, values, xyz
        q = X.queries(eb, B, seed=11)
        X.assert_bank_margin(eb, q, 0.5)
        assert X.covered(eb, q)
        e32, xq = _dev(q.e32), _dev(q.xq)
        st = eng.scan_stats(e32, xq, TAU, TAU, keep_logits=True)
        assert eng.kept_queries() == B
        _check_stats(st, eb, q, True, "scan_stats 1e6")
        want = _dev(X.expect(eb, q, 0.5))
        _assert_equal(eng.attend_kept(0, xq, TAU, TAU, 0.5, st), want, "attend_kept 1e6")
        a = 64 * 40
        _assert_equal(eng.attend_kept(a, xq[a:], TAU, TAU, 0.5, st[a:].contiguous()), want[a:], "attend_kept 1e6 tail")
    finally:
        eng.close()
        torch.cuda.empty_cache()


# -- top-k under exact ties ---------------------------------------------------------------------
@pytest.mark.parametrize("B", [200, 600])
@pytest.mark.parametrize("k", [16, 5])
def test_topk_ties_exact(B, k):
    """Classes of 16 rows (and of 2 and 1: filled up with the lowest orthogonal rows): the k best
    rows of a query are its class's lowest rows.  topk_stream (<= 256 queries fused, GEMM path
    above), selection from kept logits, in-scan lists (RANGE_KEEP_LOGITS=0)."""
    n = 4099
    bank = _bank(n, 2, 16)
    q = X.queries(bank, B, seed=B + k)
    wv, wi = map(_dev, X.topk_expect(bank, q, k))
    e32, xq = _dev(q.e32), _dev(q.xq)
    tv, ti = _engine(n, 2, 16).topk_stream(e32, k)
    _assert_equal(ti, wi, "topk_stream indices")
    _assert_equal(tv, wv, "topk_stream values")
    for env in ({}, {"RANGE_KEEP_LOGITS": 0}):
        eng = _engine(n, 2, 16, **env)
        _, tv, ti = eng.scan_stats(e32, xq, TAU, TAU, topk=k, keep_logits=True)
        _assert_equal(ti, wi, f"scan_stats top-k indices {env}")
        _assert_equal(tv, wv, f"scan_stats top-k values {env}")


def test_topk_brute_force_fallback_exact():
    """Classes of 16 384 tied rows overflow the short per-lane lists: the brute-force path."""
    n, B, k = 50000, 40, 16
    bank = _bank(n)
    q = X.queries(bank, B, seed=9)
    eng = _engine(n)
    before = eng.topk_stream_exact_count()
    tv, ti = eng.topk_stream(_dev(q.e32), k)
    wv, wi = X.topk_expect(bank, q, k)
    _assert_equal(ti, _dev(wi), "topk_stream indices (fallback)")
    _assert_equal(tv, _dev(wv), "topk_stream values (fallback)")
    assert eng.topk_stream_exact_count() > before


# -- forward level: production temperatures, constant-e-hat encoder ------------------------------
@pytest.mark.parametrize("B", [17, 700, 4100])
def test_forward_geo_head_only(tmp_path, B):
    """RANGE+ beta = 0 on a ragged bank: the geographic head alone (tau 40), one-pass path (B <= 32),
    two passes, the host contract's part cuts (B >= 4 096)."""
    bank = _bank(12500, 4)
    c = 0
    m = _model(tmp_path, bank, c, "RANGE+", 0.0)
    q, ll = _fwd_queries(bank, c, B, B)
    X.assert_margin(bank.n, int(bank.sem_size[c]), int(bank.geo_size[0]), 0.0, 12.0, 40.0, g_out=0.0)
    want = _fwd_want(bank, q, 0.0, True)
    x = torch.from_numpy(ll).to(DEV)
    _assert_rows(m(x), want, "forward_host")
    _assert_rows(m(x, return_device=True), want, "forward")


def test_forward_range_opposite_keys(tmp_path):
    """RANGE (tau 15): the class at e_c, every other key at -e_c (weight e^-30)."""
    n, P = 100000, 1 << 14
    bank = X.build(n, seed=6, sem_sizes=[P, n - P], sem_dirs=[17, 17 + 256])
    X.assert_margin(n, P, 1, 1.0, 15.0, 0.0, s_out=-1.0)
    m = _model(tmp_path, bank, 0, "RANGE", None)
    for B in (5, 300, 4100):
        q, ll = _fwd_queries(bank, 0, B, B)
        want = _fwd_want(bank, q, 1.0, False)
        x = torch.from_numpy(ll).to(DEV)
        _assert_rows(m(x), want, f"RANGE forward_host B={B}")
        _assert_rows(m(x, return_device=True), want, f"RANGE forward B={B}")
    out, tv, ti = m(x[:300], return_device=True, return_topk=16)
    _assert_rows(out, want[:300], "RANGE forward with return_topk")
    wv, wi = X.topk_expect(bank, X.Queries(q.sem[:300], q.geo[:300], None, None), 16)
    _assert_equal(ti, _dev(wi), "return_topk indices")
    _assert_equal(tv, _dev(wv), "return_topk values")


def test_forward_blend_uniform_semantic(tmp_path):
    """RANGE+ beta in {1/4, 1/2, 3/4} on 2^17 rows all at e_c (semantic weights 2^-17): one pass,
    two passes, 16 384-query chunks with part cuts, and sweep (attend_kept, blend, finalize)."""
    n = 1 << 17
    bank = X.build(n, seed=7, sem_sizes=[n], sem_dirs=[300])
    for beta in (0.25, 0.5, 0.75):
        X.assert_margin(n, n, 1 << 14, beta, 12.0, 40.0)
    m = _model(tmp_path, bank, 0, "RANGE+", 0.5)
    for B, beta in ((20, 0.25), (2000, 0.5), (16400, 0.75)):
        m.args.beta = beta
        q, ll = _fwd_queries(bank, 0, B, B)
        x = torch.from_numpy(ll).to(DEV)
        want = _fwd_want(bank, q, beta, True)
        _assert_rows(m(x), want, f"RANGE+ beta={beta} forward_host B={B}")
        if B <= 2000:
            _assert_rows(m(x, return_device=True), want, f"RANGE+ beta={beta} forward B={B}")
    q, ll = _fwd_queries(bank, 0, 1000, 1)
    sw = m.sweep(torch.from_numpy(ll).to(DEV), [0.25, 0.5, 0.75], return_device=True)
    for j, beta in enumerate((0.25, 0.5, 0.75)):
        _assert_rows(sw[j], _fwd_want(bank, q, beta, True), f"sweep beta={beta}")
