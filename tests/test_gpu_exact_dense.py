"""Bit-exact arithmetic of every retrieval route: the second family of exact banks
(tools/exact_bank.py: build_dense), whose operands an arithmetic defect cannot leave alone.

tests/test_gpu_exact.py pins the accounting with one-hot keys, values 1 or 2 and weights 1.  Here the
keys are +-1/16 in all 256 columns with 13-bit mantissa perturbations (every one of the 256 products of
a similarity is non-zero; neither bf16 nor tf32 holds the entries), the values are 1 + j / 2^17 (18
significant bits) and the in-class weights are graded powers of two (1 and 2^-3 at k = 48, l = 2; 2^-6 in the banks "g"), with
tau the float32 for which k = (float)(tau log2 e) is an integer.  Every product and every partial sum of
a correct float32 pipeline is still a float32 number in any order, so the result is the float64
expectation bit for bit (shown on the CPU for every bank used here, with the defects this file is meant
to catch planted: tests/test_exact_dense_cpu.py).  Every check is ``torch.equal``.
"""
import numpy as np
import pytest
import torch

import exact_dense_cases as D
from exact_helpers import DEV, _assert_equal, _assert_rows, _dev, _env, _fwd_queries, _fwd_want, _model
from range_amd import _native
from tools import exact_bank as X

pytestmark = pytest.mark.gpu
T32, T48, T64 = X.dense_tau(32), X.dense_tau(48), X.dense_tau(64)

_ENGINES = {}


def _engine(name, lo=0, hi=None, **env):
    """An engine holding rows [lo, hi) of the bank (row_offset lo), created under ``env``."""
    key = (name, lo, hi, tuple(sorted(env.items())))
    if key not in _ENGINES:
        b = D.bank(name)
        with _env(**env):
            eng = _native.HipEngine(DEV)
        eng.set_bank(*b.rows(lo, b.n if hi is None else hi), row_offset=lo)
        _ENGINES[key] = eng
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _release_engines():
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()
    torch.cuda.empty_cache()


def _setup(name, B, beta, geo=True, classes=None):
    """Bank, queries (perturbed where the bank's keys are), margin check, device operands, expectation."""
    bank, tau = D.bank(name), D.tau(name)
    assert beta in D.betas(name)
    q = X.queries(bank, B, seed=B, classes=classes, perturb=D.perturbed(name))
    X.assert_bank_margin(bank, q, beta, tau, tau if geo else 0.0)
    if B >= bank.n_classes and classes is None:
        assert X.covered(bank, q)
    return bank, q, _dev(q.e32), _dev(q.xq), _dev(X.expect(bank, q, beta, geo))


def _check_stats(st, bank, q, ts, tg, what, sharp=False):
    want = _dev(X.expect_stats(bank, q, ts, tg if tg > 0 else ts, sharp=sharp))
    _assert_equal(st[:, :2], want[:, :2], f"{what}: m_sem, l_sem")
    if tg > 0:
        _assert_equal(st[:, 2:], want[:, 2:], f"{what}: m_geo, l_geo")


# -- premise ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B", [("n108", 64), ("n4099", 33)])
def test_premise_graded_statistics(name, B):
    """v_exp_f32 at the negative integer -3 is 2^-3 exactly: m = 48 and l = 1 + 8 * 2^-3 = 2 bit for
    bit (d = 0 classes: their size).  Outcome on the device: profiles/NOTES.md."""
    bank, q, e32, xq, _ = _setup(name, B, 0.5)
    st = _engine(name).scan_stats(e32, xq, T48, T48)
    assert (X.expect_stats(bank, q, T48, T48)[bank.sem_size[q.sem] == 9, :2] == (48.0, 2.0)).all()
    _check_stats(st, bank, q, T48, T48, "scan_stats")


def test_premise_other_integer_exponents():
    """Arguments -2 (k = 32) and, through the running-maximum pass 1, -4 (k = 64) on the same bank."""
    bank = D.bank("n17")
    q = X.queries(bank, 33, seed=33, perturb=True)
    e32, xq = _dev(q.e32), _dev(q.xq)
    for tau in (T32, T64):
        X.assert_bank_margin(bank, q, 0.5, tau, tau, stats_only=True)
        _check_stats(_engine("n17").scan_stats(e32, xq, tau, tau), bank, q, tau, tau, f"scan_stats tau={tau:.2f}", sharp=tau > X.TAU)


# -- engine level --------------------------------------------------------------------------------
# (bank, B, beta, geo head): N across the 16-row block, B across the 16-query wave, the 64-query tile
ENGINE_CASES = [
    ("n9", 1, 0.5, True), ("n16", 16, 0.25, True), ("n17", 17, 0.75, True), ("n108", 33, 1.0, False),
    ("n108", 64, 0.5, True), ("n1537", 65, 0.25, True), ("n1537", 17, 0.0, True), ("n4099", 257, 0.75, True),
    ("n4099_plain", 64, 0.25, True), ("g108", 17, 1.0, True), ("g1537", 65, 1.0, False),      # (g: a third grade, 2^-6)
    ("n108_geo", 33, 0.25, True), ("n1537_geo", 65, 0.0, True), ("n1537_geo", 257, 0.75, True),      # graded geographic classes
]


@pytest.mark.parametrize("name,B,beta,geo", ENGINE_CASES)
def test_engine_dense(name, B, beta, geo):
    bank, q, e32, xq, want = _setup(name, B, beta, geo)
    eng = _engine(name)
    tg = T48 if geo else 0.0
    st = eng.scan_stats(e32, xq, T48, tg, keep_logits=True)
    _check_stats(st, bank, q, T48, tg, "scan_stats")
    assert eng.kept_queries() == B
    _assert_equal(eng.attend_kept(0, xq, T48, tg, beta, st), want, "attend_kept")
    _assert_equal(eng.attend(e32, xq, T48, tg, beta, st), want, "attend")
    if B > 64:                                          # a sub-range of the kept scan, from query 64
        b = min(B, 64 + 101)
        _assert_equal(eng.attend_kept(64, xq[64:b], T48, tg, beta, st[64:b].contiguous()), want[64:b],
                      f"attend_kept [64,{b})")


@pytest.mark.parametrize("name,B,beta", [("n108", 17, 0.5), ("n4099", 65, 0.25)])
def test_split_scheme_dense(name, B, beta):
    bank, q, e32, xq, want = _setup(name, B, beta)
    eng = _engine(name, RANGE_P2_STREAMK=0)
    st = eng.scan_stats(e32, xq, T48, T48, keep_logits=True)
    _check_stats(st, bank, q, T48, T48, "scan_stats")
    _assert_equal(eng.attend_kept(0, xq, T48, T48, beta, st), want, "attend_kept (splits)")
    _assert_equal(eng.attend(e32, xq, T48, T48, beta, st), want, "attend (splits)")


@pytest.mark.parametrize("name,B,beta", [("n1537", 33, 0.75), ("n4099", 257, 0.5)])
def test_no_kept_logits_dense(name, B, beta):
    bank, q, e32, xq, want = _setup(name, B, beta)
    eng = _engine(name, RANGE_KEEP_LOGITS=0)
    st = eng.scan_stats(e32, xq, T48, T48, keep_logits=True)
    assert eng.kept_queries() == 0
    _check_stats(st, bank, q, T48, T48, "scan_stats")
    _assert_equal(eng.attend(e32, xq, T48, T48, beta, st), want, "attend (nothing kept)")


@pytest.mark.parametrize("n_splits", [1, 3, 0])
def test_chunked_scan_dense(n_splits):
    name, B, cuts = "n4099", 257, [0, 64, 192, 257]
    bank, q, e32, xq, want = _setup(name, B, 0.25)
    eng = _engine(name)
    sts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        sts.append(eng.scan_stats_at(e32[a:b], xq[a:b], T48, T48, a, B, n_splits))
        assert eng.kept_queries() == b
    st = torch.cat(sts)
    _check_stats(st, bank, q, T48, T48, f"scan_stats_at (n_splits={n_splits})")
    for a, b in zip(cuts[:-1], cuts[1:]):
        _assert_equal(eng.attend_kept(a, xq[a:b], T48, T48, 0.25, st[a:b].contiguous()), want[a:b],
                      f"attend_kept chunk [{a},{b}) n_splits={n_splits}")


@pytest.mark.parametrize("name", sorted(D.STATS_PAIRS))
def test_stats_kept_dense(name):
    """One kept scan, the statistics at temperatures on both sides of 43: l = 1 + 8 * 2^(-k/16) = 3, 2,
    1.5 - against the expectation, and against scan_stats at the pair's temperatures.  (The emulator on
    the same bank, queries and pairs: test_exact_dense_cpu.test_statistics_at_other_temperatures.)"""
    bank, q = D.bank(name), D.stats_queries(name)
    pairs = [D.pair_taus(p) for p in D.STATS_PAIRS[name]]
    e32, xq = _dev(q.e32), _dev(q.xq)
    eng = _engine(name)
    eng.scan_stats(e32, xq, T48, T48, keep_logits=True)
    got = eng.stats_kept(0, xq, pairs)
    sub = eng.stats_kept(64, xq[64:], pairs)
    for j, (ts, tg) in enumerate(pairs):
        X.assert_bank_margin(bank, q, 0.5, ts, tg, stats_only=True)
        sharp = max(ts, tg) > X.TAU
        _check_stats(got[j], bank, q, ts, tg, f"stats_kept ({ts:.2f}, {tg:.2f})", sharp=sharp)
        _assert_equal(got[j], eng.scan_stats(e32, xq, ts, tg), f"stats_kept vs scan_stats ({ts:.2f}, {tg:.2f})")
        _assert_equal(sub[j], got[j][64:], f"stats_kept from query 64 ({ts:.2f}, {tg:.2f})")


@pytest.mark.parametrize("name,cuts,B", [("n108", [0, 37, 108], 33), ("n4099", [0, 1001, 2503, 4099], 65)])
def test_shards_dense(name, cuts, B):
    """Row shards at offsets that are no multiple of 16 (graded classes straddle them): merge_stats,
    per-shard attend, finalize; the top-k side channel through merge_topk."""
    bank, q, e32, xq, want = _setup(name, B, 0.75)
    engs = [_engine(name, lo=a, hi=b) for a, b in zip(cuts[:-1], cuts[1:])]
    k = 16
    outs = [e.scan_stats(e32, xq, T48, T48, topk=k) for e in engs]
    st = engs[0].merge_stats(torch.stack([o[0] for o in outs]).contiguous())
    _check_stats(st, bank, q, T48, T48, "merge_stats")
    parts = torch.stack([e.attend(e32, xq, T48, T48, 0.75, st) for e in engs]).contiguous()
    e64 = e32.double()
    out = engs[0].finalize(parts, e64)
    _assert_equal(out[:, :1024], want.double(), "finalize of shard partials")
    assert torch.equal(out[:, 1024:], e64)
    tv, ti = engs[0].merge_topk(torch.stack([o[1] for o in outs]).contiguous(),
                                torch.stack([o[2] for o in outs]).contiguous())
    wv, wi = X.topk_expect(bank, q, k)
    _assert_equal(ti, _dev(wi), "merge_topk indices")
    _assert_equal(tv, _dev(wv), "merge_topk values")


@pytest.mark.parametrize("beta", [0.25, 0.5, 0.75])
def test_blend_dense(beta):
    """blend of the two heads' retrievals (G: beta = 0, H: beta = 1): (1 - beta) G + beta H is the blended
    expectation - both products and the sum are float32 numbers."""
    bank, q, e32, xq, want = _setup("n1537", 65, beta)
    eng = _engine("n1537")
    st = eng.scan_stats(e32, xq, T48, T48)
    G = eng.attend(e32, xq, T48, T48, 0.0, st)
    H = eng.attend(e32, xq, T48, T48, 1.0, st)
    _assert_equal(G, _dev(X.expect(bank, q, 0.0)), "geographic head alone")
    _assert_equal(H, _dev(X.expect(bank, q, 1.0)), "semantic head alone")
    _assert_equal(eng.blend(G, H, beta), want, f"blend beta={beta}")


# -- the sharp route: tau = 44.36 (k = 64), pass 1 with a running maximum ---------------------------
@pytest.mark.parametrize("name,B,beta", [("s108", 33, 0.5), ("s108_notop", 17, 1.0), ("s108_notop", 65, 0.5),
                                         ("s108_last", 64, 0.5), ("s1537_last", 65, 0.5)])
def test_sharp_dense(name, B, beta):
    """m is the largest in-bank exponent - 64, or 60 for a class without a d = 0 row, whose l is then 16
    weights of 1 - and rescaling an earlier partial by an integer power of two keeps everything exact
    (``*_last``: every d = 0 row sits behind all graded rows)."""
    bank = D.bank(name)
    classes = np.arange(min(bank.n_classes, 24)) if bank.n_classes > B else None     # (the classes without a d = 0 row come first)
    bank, q, e32, xq, want = _setup(name, B, beta, classes=classes)
    if name in D.NO_TOP:
        assert (q.sem < D.NO_TOP[name]).any() and (X.expect_stats(bank, q, T64, T64, sharp=True)[q.sem < D.NO_TOP[name], :2] == (60.0, 16.0)).all()
    eng = _engine(name)
    st = eng.scan_stats(e32, xq, T64, T64, keep_logits=True)
    _check_stats(st, bank, q, T64, T64, "scan_stats (sharp)", sharp=True)
    _assert_equal(eng.attend_kept(0, xq, T64, T64, beta, st), want, "attend_kept (sharp)")
    _assert_equal(eng.attend(e32, xq, T64, T64, beta, st), want, "attend (sharp)")
    st3 = eng.scan_stats_at(e32, xq, T64, T64, 0, B, 3)
    _check_stats(st3, bank, q, T64, T64, "scan_stats_at, three splits (sharp)", sharp=True)
    # the semantic head sharp, the geographic one at k = 48 - and without a geographic head
    _check_stats(eng.scan_stats(e32, xq, T64, T48), bank, q, T64, T48, "scan_stats (64, 48)", sharp=True)
    _check_stats(eng.scan_stats(e32, xq, T64, 0.0), bank, q, T64, 0.0, "scan_stats (64, -)", sharp=True)


# -- the one-pass path and the host contract, through load_model with its tunable temperatures ------
@pytest.mark.parametrize("model,beta", [("RANGE+", 0.25), ("RANGE+", 0.75), ("RANGE", None)])
@pytest.mark.parametrize("name,prepared", D.FORWARD_BANKS)
def test_forward_dense(tmp_path, name, prepared, model, beta):
    """load_model(temp=, geo_temp=) at k = 48 with the plain query h_c / 16 of a constant-bias encoder (its
    float64 normalisation is exact): attend_small_kernel + small_finalize_kernel for B <= 32 - a Q K^T
    loop of their own, not pass 1's - and two passes above.  The keys carry their mantissa perturbation
    (and the locations their grades) where the bank is a prepared bank file, whose arrays the engine
    uploads as written; the .npz variant has plain keys, which its reader's float32 normalisation
    divides by exactly 1.  With the plain query a key rounded to bf16 or cut to tf32 still changes the
    similarity (test_exact_dense_cpu.test_forward_configuration)."""
    c = D.forward_class(name)
    bank = D.bank(name)
    assert bank.sem_size[c] == 9 and prepared == D.perturbed(name)
    geo = model == "RANGE+"
    m = _model(tmp_path, bank, c, model, beta, prepared=prepared, temp=T48, **({"geo_temp": T48} if geo else {}))
    for B in D.FORWARD_B:
        q, ll = _fwd_queries(bank, c, B, B)
        X.assert_bank_margin(bank, q, 1.0 if beta is None else beta, T48, T48 if geo else 0.0)
        want = _fwd_want(bank, q, 1.0 if beta is None else beta, geo)
        x = torch.from_numpy(ll).to(DEV)
        _assert_rows(m(x), want, f"{model} forward_host B={B}")
        _assert_rows(m(x, return_device=True), want, f"{model} forward B={B}")


# -- pv_mode bf16x3 -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,beta", [("n108", 17, 0.25), ("n4099", 65, 0.75)])
def test_bf16x3_dense(name, B, beta):
    """attend_bf16x3.h splits both operands into three bf16 planes (8 + 8 + 8 bits) and drops the products
    w_m V_l, w_l V_m, w_l V_l.  Here the planes hold V exactly (18 bits: V_h + V_m + V_l = V) and every
    weight ca 2^-3j + cb 2^0 is a multiple of 1/64 below 1 - one plane (w_m = w_l = 0) - so the dropped
    products are zero, every kept product is exact (8 x 8 bits) and every partial sum is on the same grid
    as in the float32 kernel: equality holds, and is asserted.  With V cut to two planes in the BANK
    (not in the kernel) the same call must come out different."""
    bank, q, e32, xq, want = _setup(name, B, beta)
    ca, cb = beta / 2.0 * np.array([1.0, 0.125, 0.0]), (1.0 - beta) / bank.geo_size[:3].max() * np.array([0.0, 1.0])
    w = (ca[:, None] + cb[None, :]).ravel()
    assert np.array_equal(X._keep_bits(w.astype(np.float32), 8), w.astype(np.float32))
    hi = X._round_bf16(bank.values)
    cut = hi + X._round_bf16(bank.values - hi)               # the first two of split3's planes
    assert (cut != bank.values).mean() > 0.2 and np.array_equal(cut + X._round_bf16(bank.values - cut), bank.values)
    eng2 = _native.HipEngine(DEV)
    try:
        for eng, v in ((_engine(name), None), (eng2, cut)):
            if v is not None:
                eng.set_bank(bank.keys, v, bank.xyz)
            eng.set_pv_mode("bf16x3")
            try:
                st = eng.scan_stats(e32, xq, T48, T48, keep_logits=True)
                out = eng.attend_kept(0, xq, T48, T48, beta, st)
            finally:
                eng.set_pv_mode("exact")
            if v is None:
                _assert_equal(out, want, "attend_kept bf16x3")
            else:
                assert (out != want).any(dim=1).all(), "two planes of V gave the three-plane result"
    finally:
        eng2.close()


# -- top-k: similarities 1, 15/16 in eight-way ties, then the other classes' rows -------------------
@pytest.mark.parametrize("name", ["n4099", "n4099_plain"])
@pytest.mark.parametrize("B,k", [(33, 16), (200, 5), (257, 16)])
def test_topk_dense(name, B, k):
    """Indices and values of topk_stream (fused up to 256 queries, the GEMM-shaped batch path at 257) and
    of scan_stats(topk=) with and without kept logits; ties go to the lower row.  The plain keys are what
    the half-precision copies of the keys hold exactly; the perturbed ones they do not."""
    bank = D.bank(name)
    q = X.queries(bank, B, seed=B + k, perturb=D.perturbed(name))
    wv, wi = map(_dev, X.topk_expect(bank, q, k))
    e32, xq = _dev(q.e32), _dev(q.xq)
    tv, ti = _engine(name).topk_stream(e32, k)
    _assert_equal(ti, wi, "topk_stream indices")
    _assert_equal(tv, wv, "topk_stream values")
    for env in ({}, {"RANGE_KEEP_LOGITS": 0}):
        _, tv, ti = _engine(name, **env).scan_stats(e32, xq, T48, T48, topk=k, keep_logits=True)
        _assert_equal(ti, wi, f"scan_stats top-k indices {env}")
        _assert_equal(tv, wv, f"scan_stats top-k values {env}")
