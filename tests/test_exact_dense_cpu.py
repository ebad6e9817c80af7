"""CPU checks of the dense exact banks (tools/exact_bank.py: build_dense): every bank that
tests/test_gpu_exact_dense.py uses goes through the any-order float32 emulator and must give the float64
expectation bit for bit; every planted arithmetic defect must break that equality on at least one of
them (a defect that survives everywhere is a gap in the banks); the generalised margin and top-k
expectations say what they should.  No GPU."""
import numpy as np
import pytest

import exact_dense_cases as D
from oracle import range_oracle as O
from tools import exact_bank as X

ORDERS = [(1, 1), (2, 3), (3, 5), (4, 7)]          # (seed of the summation order, partial sums)


def _queries(name, B=16, seed=3):
    return X.queries(D.bank(name), B, seed=seed, perturb=D.perturbed(name))


def test_integer_temperatures():
    """k = (float)(tau * log2 e) is the integer, and the neighbouring float32 temperatures miss it."""
    for k, t in X.DENSE_TAU.items():
        tau = np.float32(t)
        assert X.k_shift(X.dense_tau(k)) == np.float32(k)
        for other in (np.nextafter(tau, np.float32(0)), np.nextafter(tau, np.float32(100))):
            assert X.k_shift(float(other)) != np.float32(k)


@pytest.mark.parametrize("name", sorted(D.BANKS))
def test_layout(name):
    b = D.bank(name)
    k = D.BANKS[name]["k"]
    assert b.keys.dtype == b.values.dtype == b.xyz.dtype == np.float32 and b.dense and b.k == k
    k64, h = b.keys.astype(np.float64), X._hadamard(b.sem_dir[b.sem])
    # every one of the 256 entries non-zero, norm inside the engine's limit, in-class similarity 1 - d/128
    assert (np.abs(k64) > 2.0 ** -5).all() and np.linalg.norm(k64, axis=1).max() < 1.0005
    assert np.array_equal((k64 * h).sum(1) / 16.0, 1.0 - b.grade / 128.0)
    assert np.array_equal(np.bincount(b.sem, minlength=b.n_classes), b.sem_size)
    # two classes: orthogonal or opposite directions
    gram = X._hadamard(b.sem_dir) @ X._hadamard(b.sem_dir).T
    assert set(np.unique(gram - 256.0 * np.eye(b.n_classes))) <= {0.0, -256.0}
    sig = X._keep_bits(b.keys, 8)
    if D.perturbed(name):    # entries that bf16 (8 bits) and tf32 (11) do not hold, in every row
        assert (b.keys != sig).any(axis=1).all() and (b.keys != X._keep_bits(b.keys, 11)).any(axis=1).all()
    else:
        assert np.array_equal(b.keys, sig) and set(np.unique(np.abs(b.keys))) == {np.float32(1 / 16)}
        assert np.array_equal(np.linalg.norm(b.keys, ord=2, axis=1), np.ones(b.n, np.float32))
    # values: 18 significant bits, in [1, 2), every row and every column its own
    v = b.values.astype(np.float64)
    assert (v >= 1).all() and (v < 2).all() and np.array_equal(v * 2 ** 17, np.round(v * 2 ** 17))
    assert (b.values != X._keep_bits(b.values, 16)).mean() > 0.5
    assert len({r.tobytes() for r in b.values}) == b.n and len({c.tobytes() for c in b.values.T}) == X.VAL_DIM
    # geographic classes small enough for the value grid; l a power of two; the d = 0 rows last where asked
    if D.BANKS[name].get("geo_graded"):
        assert b.geo_size[:3].tolist() == [9, 9, 9] and b.l_geo[:3].tolist() == [2, 2, 2]
        norm = np.linalg.norm(b.xyz.astype(np.float64), axis=1)
        assert sorted(np.unique(norm)) == [15 / 16, 1.0] and all((norm[b.geo == a] == 1).sum() == 1 for a in range(3))
    else:
        assert all(s & (s - 1) == 0 and s <= 8 for s in b.geo_size[:3] if s) and b.geo_size[0] > 0
    assert set(np.log2(b.l_sem) % 1) == {0.0}
    if D.BANKS[name].get("top_last"):
        n0 = int((b.grade == 0).sum())
        assert n0 and (b.grade[-n0:] == 0).all() and (b.grade[:-n0] != 0).all()
    for c in range(D.NO_TOP.get(name, 0)):
        assert (b.grade[b.sem == c] == X.GRADE).all()


@pytest.mark.parametrize("name", sorted(D.BANKS))
def test_any_order_emulator_equals_expectation(name):
    """The condition of use: float32 accumulation of the logits, of l and of w @ V in seeded random
    orders over 1, 3, 5 and 7 partial sums gives the float64 expectation bit for bit."""
    b, q, tau = D.bank(name), _queries(name), D.tau(name)
    sharp = tau > X.TAU
    ws = X.expect_stats(b, q, tau, tau, sharp=sharp)
    for (seed, parts), beta in zip(ORDERS, D.betas(name) * 4):
        X.assert_bank_margin(b, q, beta, tau, tau)
        st, out = X.emulate(b, q, beta, tau, tau, seed=seed, parts=parts, sharp=sharp)
        assert np.array_equal(st, ws), (name, seed, parts)
        assert np.array_equal(out, X.expect(b, q, beta)), (name, seed, parts, beta)
    X.assert_bank_margin(b, q, 1.0, tau, 0.0)
    st, out = X.emulate(b, q, 0.5, tau, 0.0, seed=9, parts=3, sharp=sharp)          # no geographic head
    assert np.array_equal(st[:, :2], ws[:, :2]) and np.array_equal(out, X.expect(b, q, 0.5, geo=False))
    if sharp and b.geo_l is None:              # the semantic head sharp, the geographic one at k = 48
        t48 = X.dense_tau(48)
        X.assert_bank_margin(b, q, 0.5, tau, t48, stats_only=True)
        st, _ = X.emulate(b, q, 0.5, tau, t48, seed=11, parts=5, sharp=True)
        assert np.array_equal(st, X.expect_stats(b, q, tau, t48, sharp=True))


@pytest.mark.parametrize("name,prepared", D.FORWARD_BANKS)
def test_forward_configuration(name, prepared):
    """The load_model tests' configuration: B plain queries h_c / 16 of one class.  The emulator gives the
    expectation; on a bank with perturbed keys (a prepared bank file) keys rounded to bf16 or cut to tf32
    break it although the query has no mantissa bits - on plain keys (the .npz variant) they cannot.  The
    class sits on an odd Hadamard row, so a mispaired 4-chunk shows on either."""
    b, tau, c = D.bank(name), D.tau(name), D.forward_class(name)
    assert b.sem_size[c] == 9 and prepared == D.perturbed(name)
    for B, (seed, parts), beta in zip(D.FORWARD_B, ORDERS + ORDERS[:1], (0.25, 0.75, 1.0, 0.25, 0.75)):
        q = X.forward_queries(b, c, B, B)
        X.assert_bank_margin(b, q, beta, tau, tau)
        st, out = X.emulate(b, q, beta, tau, tau, seed=seed, parts=parts)
        assert np.array_equal(st, X.expect_stats(b, q, tau, tau)) and np.array_equal(out, X.expect(b, q, beta))
    for defect in ("k_bf16", "tf32", "v16", "exp2_trunc4", "drop_col255", "mispair"):
        st, out = X.emulate(b, q, 0.75, tau, tau, seed=5, parts=3, defect=defect)
        same = np.array_equal(st, X.expect_stats(b, q, tau, tau)) and np.array_equal(out, X.expect(b, q, 0.75))
        assert same == (not prepared and defect in ("k_bf16", "tf32")), (name, defect)


DEFECT_BANKS = ["n17", "n108", "n108_plain", "s108_notop"]


@pytest.mark.parametrize("defect", X.DEFECTS)
def test_planted_defect_is_caught(defect):
    caught = []
    for name in DEFECT_BANKS:
        b, q, tau = D.bank(name), _queries(name), D.tau(name)
        sharp = tau > X.TAU
        st, out = X.emulate(b, q, 0.5, tau, tau, seed=5, parts=3, sharp=sharp, defect=defect)
        if not (np.array_equal(st, X.expect_stats(b, q, tau, tau, sharp=sharp)) and np.array_equal(out, X.expect(b, q, 0.5))):
            caught.append(name)
    print(defect, "caught on", caught)
    assert caught, f"{defect} survives on every bank"
    if defect in ("v16", "v8", "v_swap_cols", "grade_wrong_row", "l_missing_grade", "drop_col255"):
        assert caught == DEFECT_BANKS          # (no operand of any bank hides these)


def test_the_one_hot_family_is_blind_to_them():
    """Why the second family exists: on a one-hot bank most of the planted defects change nothing."""
    b = X.build(108, seed=1, sem_cap=8)
    q = X.queries(b, 16, seed=3)
    assert not b.dense
    blind = []
    for defect in X.DEFECTS:
        st, out = X.emulate(b, q, 0.5, X.TAU, X.TAU, seed=5, parts=3, defect=defect)
        if np.array_equal(st, X.expect_stats(b, q)) and np.array_equal(out, X.expect(b, q, 0.5)):
            blind.append(defect)
    assert {"v16", "v8", "k_bf16", "q_bf16", "tf32", "exp2_trunc4", "l_missing_grade"} <= set(blind), blind


@pytest.mark.parametrize("name", sorted(D.STATS_PAIRS))
def test_statistics_at_other_temperatures(name):
    """The bank, queries and (k_sem, k_geo) pairs tests/test_gpu_exact_dense.py sweeps with stats_kept,
    through the emulator: l = 1 + 8 * 2^(-k/16) = 3, 2, 1.5 at k = 32, 48, 64."""
    b, q = D.bank(name), D.stats_queries(name)
    big = b.sem_size[q.sem] == 9
    assert big.any()
    for j, pair in enumerate(D.STATS_PAIRS[name]):
        ts, tg = D.pair_taus(pair)
        sharp = max(ts, tg) > X.TAU
        X.assert_bank_margin(b, q, 0.5, ts, tg, stats_only=True)
        ws = X.expect_stats(b, q, ts, tg if tg > 0 else ts, sharp=sharp)
        assert (ws[big, 1] == 1 + 8 * 2.0 ** (-pair[0] / 16)).all() and (ws[:, 0] == pair[0]).all()
        st, _ = X.emulate(b, q, 0.5, ts, tg, seed=j + 1, parts=(3, 5, 7, 1, 3)[j], sharp=sharp)
        n = 4 if tg > 0 else 2
        assert np.array_equal(st[:, :n], ws[:, :n]), (name, pair)


def test_margin_refuses_a_bank_too_large_for_its_temperature():
    with pytest.raises(AssertionError):                       # 108 rows do not round away at k = 32
        X.assert_bank_margin(D.bank("n108"), _queries("n108"), 0.5, X.dense_tau(32), X.dense_tau(32), stats_only=True)


def test_admitted_blend_weights():
    """X.dense_betas derives them from the bank; assert_margin agrees on every one it admits and refuses
    the others for the grid."""
    want = {"n108": X.BETAS, "n108_geo": X.BETAS, "s108": (0.5, 1.0, 0.0), "s108_notop": (0.5, 1.0, 0.0), "g108": (1.0, 0.0)}
    for name, betas in want.items():
        b, q, tau = D.bank(name), _queries(name), D.tau(name)
        assert D.betas(name) == betas, name
        for beta in X.BETAS:
            if beta in betas:
                X.assert_bank_margin(b, q, beta, tau, tau)
            else:
                with pytest.raises(AssertionError, match="grid"):
                    X.assert_bank_margin(b, q, beta, tau, tau)


def test_third_grade():
    """Weights 2^-3 and 2^-6 in one class of l = 1; the grid refuses a blend there, and l = 2 with 2^-6."""
    b, q, tau = D.bank("g108"), _queries("g108"), D.tau("g108")
    assert sorted(np.unique(b.grade)) == [8, 16] and (X.expect_stats(b, q, tau, tau)[:, :2] == (48.0, 1.0)).all()
    with pytest.raises(AssertionError, match="grid"):
        X.assert_bank_margin(b, q, 0.5, tau, tau)
    with pytest.raises(AssertionError, match="grid"):
        X.assert_margin(108, 65, 8, 1.0, tau, tau, s_out=1 / 8, l_sem=2.0, w_min=2.0 ** -6, v_bits=17)
    st, out = X.emulate(b, q, 1.0, tau, tau, seed=2, parts=5, defect="exp2_trunc4")
    assert not np.array_equal(st, X.expect_stats(b, q, tau, tau))


def test_sharp_expectation():
    b = D.bank("s108_notop")
    q = X.queries(b, 16, seed=3, perturb=True)
    ws = X.expect_stats(b, q, D.tau("s108_notop"), D.tau("s108_notop"), sharp=True)
    no_top = q.sem < 2
    assert no_top.any() and (ws[no_top, 0] == 60).all() and (ws[no_top, 1] == 16).all()
    full = b.sem_size[q.sem] == 17
    assert full.any() and (ws[full, 0] == 64).all() and (ws[full, 1] == 2).all()


def test_margin_covers_grades_and_the_value_grid():
    t48, t64 = X.dense_tau(48), X.dense_tau(64)
    X.assert_margin(4099, 9, 8, 0.25, t48, t48, s_out=1 / 16, l_sem=2.0, w_min=2.0 ** -3, v_bits=17)
    with pytest.raises(AssertionError, match="grid"):       # weight 2^-4 / 2 at beta 1/4 on 2^-17 values: 2^-24
        X.assert_margin(108, 17, 8, 0.25, t64, t64, s_out=1 / 16, l_sem=2.0, w_min=2.0 ** -4, v_bits=17)
    with pytest.raises(AssertionError, match="grid"):       # a geographic class of 32 rows
        X.assert_margin(108, 9, 32, 0.25, t48, t48, s_out=1 / 16, l_sem=2.0, w_min=2.0 ** -3, v_bits=17)
    with pytest.raises(AssertionError, match="margin|absorbed"):   # 10^6 rows at 2^-45 do not round away
        X.assert_margin(1 << 20, 9, 8, 0.25, t48, t48, s_out=1 / 16, l_sem=2.0, w_min=2.0 ** -3, v_bits=17)
    # a graded geographic class: nine rows, l_geo = 2, smallest weight 2^-3 - and not with 2^-4 at beta 1/4
    X.assert_margin(108, 9, 9, 0.25, t48, t48, s_out=1 / 16, l_sem=2.0, w_min=2.0 ** -3, v_bits=17, l_geo=2.0, g_min=2.0 ** -3)
    with pytest.raises(AssertionError, match="grid"):
        X.assert_margin(108, 9, 17, 0.25, t48, t64, s_out=1 / 16, l_sem=2.0, w_min=2.0 ** -3, v_bits=17, l_geo=2.0, g_min=2.0 ** -4)
    with pytest.raises(AssertionError):                     # l = 1.5
        X.assert_margin(108, 9, 8, 0.5, t64, t64, s_out=1 / 16, l_sem=1.5, w_min=2.0 ** -4, v_bits=17)


@pytest.mark.parametrize("name", ["n108", "n108_plain"])
@pytest.mark.parametrize("beta", [0.25, 1.0])
def test_dense_exact_equals_float64_softmax(name, beta):
    """The expectation is the float64 softmax retrieval of the oracle's similarities at the bank's
    temperature, to the out-of-class mass (2^-45 per row)."""
    b, q, tau = D.bank(name), _queries(name), D.tau(name)
    s, g = O.logits64(q.e32.astype(np.float64), X.lonlat_of(q.geo), O.Bank(b.keys, b.values, b.xyz))

    def sm(z):
        p = np.exp(z - z.max(axis=1, keepdims=True))
        return p / p.sum(axis=1, keepdims=True)
    V = b.values.astype(np.float64)
    ref = beta * (sm(tau * s) @ V) + (1 - beta) * (sm(tau * g) @ V)
    np.testing.assert_allclose(X.expect(b, q, beta).astype(np.float64), ref, rtol=1e-9, atol=0)


@pytest.mark.parametrize("name", ["n108", "n4099_plain"])
def test_dense_topk_expectation(name):
    b, q = D.bank(name), _queries(name, 40)
    tv, ti = X.topk_expect(b, q, 16)
    rv, ri = O.topk64(X.similarities64(b, q.e32), 16)
    assert np.array_equal(ri, ti) and np.array_equal(rv, tv)
    big = b.sem_size[q.sem] == 9
    assert big.any() and (tv[big, 0] == 1).all() and (tv[big, 1:9] == np.float32(15 / 16)).all() and (tv[big, 9] < 0.2).all()
    for i in np.flatnonzero(big):                             # the eight-way tie goes to the lower rows
        assert (np.diff(ti[i, 1:9]) > 0).all() and b.sem[ti[i, :9]].tolist() == [q.sem[i]] * 9
