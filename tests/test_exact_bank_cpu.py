"""CPU self-checks of tools/exact_bank.py: the banks are what tests/test_gpu_exact.py relies on
(partition, sizes, signatures, margins), and the "exact" answer really is the retrieval's value:
it equals a float64 softmax of the oracle's similarities."""
import numpy as np
import pytest

from oracle import range_oracle as O
from tools import exact_bank as X


@pytest.mark.parametrize("n", [1, 15, 17, 4099, 12500, 16385, 50000, 50001, 100003, 1_000_000])
def test_partition(n):
    for cap in (16, 1 << 14):
        s = X.pow2_partition(n, cap)
        assert sum(s) == n and all(v & (v - 1) == 0 and v <= cap for v in s)
        assert s == sorted(s, reverse=True) and len(set(s[s.count(cap):])) == len(s) - s.count(cap)


@pytest.mark.parametrize("n,cap", [(1, 1 << 14), (17, 1 << 14), (4099, 16), (12500, 1 << 14)])
def test_bank_layout(n, cap):
    b = X.build(n, seed=3, sem_cap=cap)
    assert b.keys.dtype == b.values.dtype == b.xyz.dtype == np.float32
    # signed one-hot keys, every zero +0.0
    assert (np.abs(b.keys).sum(1) == 1).all() and not np.signbit(b.keys[b.keys == 0]).any()
    d = b.sem_dir[b.sem]
    assert np.array_equal(b.keys[np.arange(n), d % 256], np.where(d >= 256, -1.0, 1.0).astype(np.float32))
    assert np.array_equal(np.bincount(b.sem, minlength=b.n_classes), b.sem_size)
    assert np.array_equal(np.bincount(b.geo, minlength=6), b.geo_size)
    assert all(s & (s - 1) == 0 for s in b.geo_size[:3] if s) and b.geo_size[0] > 0
    assert np.array_equal(b.xyz, X.AXES[b.geo]) and not np.signbit(b.xyz[b.xyz == 0]).any()
    # values: column 0 constant, 1-20 the row index, all in {1, 2}
    assert set(np.unique(b.values)) <= {1.0, 2.0} and (b.values[:, 0] == 1).all()
    idx = ((b.values[:, 1:21] - 1).astype(np.int64) << np.arange(20)).sum(1)
    assert np.array_equal(idx, np.arange(n) % (1 << 20))
    assert len({r.tobytes() for r in b.values}) == n     # every row carries its own signature
    ref = np.zeros_like(b.sem_sum)
    np.add.at(ref, b.sem, b.values.astype(np.float64))
    assert np.array_equal(ref, b.sem_sum)
    if n >= 4096:   # a 16-row block mixes classes
        blocks = b.sem[: n // 16 * 16].reshape(-1, 16)
        assert np.mean([len(set(r)) for r in blocks]) > 1.5


def test_device_builder_matches_host():
    torch = pytest.importorskip("torch")
    eb, k, v, x = X.build_device(5000, "cpu", seed=4)
    b = X.build(5000, seed=4)
    assert np.array_equal(k.numpy(), b.keys) and np.array_equal(v.numpy(), b.values)
    assert np.array_equal(x.numpy(), b.xyz) and np.array_equal(eb.sem_sum, b.sem_sum)
    assert np.array_equal(eb.geo_sum, b.geo_sum) and torch.is_tensor(k)


def test_queries_cover_every_row():
    b = X.build(50001, seed=0)
    q = X.queries(b, 64, seed=1)
    assert X.covered(b, q) and set(q.geo) == {0, 1, 2}
    assert (b.sem_size[q.sem] > 0).all() and (b.geo_size[q.geo] > 0).all()


# the configurations of tests/test_gpu_exact.py
ENGINE = [(1, 1, 0.5), (15, 16, 0.5), (17, 17, 0.25), (4099, 33, 1.0), (12500, 64, 0.0), (16385, 257, 0.25),
          (50000, 4097, 0.5), (50001, 10000, 0.25), (100000, 10000, 0.5), (100003, 16385, 0.75)]


@pytest.mark.parametrize("n,B,beta", ENGINE)
def test_engine_margins(n, B, beta):
    sizes, _, _, gs, _ = X._plan(n, 0, 1 << 14, 1 << 14, None)    # (the plan alone: no values needed)
    for P in set(sizes.tolist()):
        for Q in set(gs[:3].tolist()) - {0}:
            X.assert_margin(n, P, Q, beta, X.TAU, X.TAU)


def test_million_row_margin():
    sizes, _, _, gs, _ = X._plan(1_000_000, 3, 1 << 14, 1 << 14, None)
    for P in set(sizes.tolist()):
        X.assert_margin(1_000_000, P, int(gs[0]), 0.5, X.TAU, X.TAU)


def test_forward_margins():
    X.assert_margin(12500, 8192, 4096, 0.0, 12.0, 40.0)
    X.assert_margin(100000, 1 << 14, 1, 1.0, 15.0, 0.0, s_out=-1.0)
    for beta in (0.25, 0.5, 0.75):
        X.assert_margin(1 << 17, 1 << 17, 1 << 14, beta, 12.0, 40.0)


def test_margin_refuses_what_would_not_round_away():
    with pytest.raises(AssertionError):
        X.assert_margin(100000, 1, 1, 1.0, 15.0, 0.0)                # orthogonal keys at tau 15
    with pytest.raises(AssertionError):
        X.assert_margin(3 << 20, 1 << 14, 1, 1.0, 15.0, 0.0, s_out=-1.0)
    with pytest.raises(AssertionError):
        X.assert_margin(100, 12, 4, 0.5, X.TAU, X.TAU)               # not a power of two


def _softmax64(z):
    z = z - z.max(axis=1, keepdims=True)
    p = np.exp(z)
    return p / p.sum(axis=1, keepdims=True)


@pytest.mark.parametrize("beta", [0.0, 0.25, 0.5, 0.75, 1.0])
def test_exact_equals_float64_softmax(beta):
    """At N ~ 5 000 the exact expectation is the float64 softmax retrieval of the oracle's
    similarities (tau 43 on both heads) to 1e-12 relative."""
    b = X.build(5003, seed=8, sem_cap=1024)
    q = X.queries(b, 40, seed=2)
    s, g = O.logits64(q.e32.astype(np.float64), X.lonlat_of(q.geo), O.Bank(b.keys, b.values, b.xyz))
    V = b.values.astype(np.float64)
    ref = beta * (_softmax64(X.TAU * s) @ V) + (1 - beta) * (_softmax64(X.TAU * g) @ V)
    got = X.expect(b, q, beta).astype(np.float64)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)


def _fwd_case(bank, c, B, model, beta):
    rng = np.random.default_rng(B)
    geo = rng.choice(np.flatnonzero(bank.geo_size[:3] > 0), B)
    e = np.tile(X.direction_vector(int(bank.sem_dir[c])).astype(np.float64), (B, 1))
    q = X.Queries(np.full(B, c), geo, e.astype(np.float32), None)
    obank = O.prep_bank(X.lonlat_of(bank.geo), bank.values, bank.keys)
    ref = O.retrieve64(e, X.lonlat_of(geo), obank, model, beta)
    got = X.expect(bank, q, 1.0 if model == "RANGE" else beta, model == "RANGE+")
    np.testing.assert_allclose(got.astype(np.float64), ref, rtol=1e-9, atol=0)


def test_forward_configurations_equal_oracle():
    """The three production-temperature configurations of the forward tests (at CPU sizes)
    against O.retrieve64 - axis locations through the reference's float32 trigonometry."""
    _fwd_case(X.build(6001, seed=4), 0, 30, "RANGE+", 0.0)
    n, P = 12000, 1 << 12
    _fwd_case(X.build(n, seed=6, sem_sizes=[P, n - P], sem_dirs=[17, 273]), 0, 30, "RANGE", None)
    n = 1 << 13
    for beta in (0.25, 0.5, 0.75):
        _fwd_case(X.build(n, seed=7, sem_sizes=[n], sem_dirs=[300]), 0, 30, "RANGE+", beta)


def test_topk_expectation():
    b = X.build(4099, seed=2, sem_cap=16)
    q = X.queries(b, 300, seed=3)
    tv, ti = X.topk_expect(b, q, 16)
    s = q.e32.astype(np.float64) @ b.keys.astype(np.float64).T
    rv, ri = O.topk64(s, 16)
    assert np.array_equal(ri, ti) and np.array_equal(rv, tv)
