"""CPU checks of tests/probe_refs.py, the comparison code of tests/test_gpu_probe_kernels.py.

Not too tight: plain float64 numpy evaluations of every operation, on the input generators the
GPU tests use, stay below ratio 1.  Not blind: every planted defect - each a mistake a kernel of
this kind can make while the end-to-end goldens still pass - exceeds it."""
import numpy as np
import pytest

import probe_refs as pr
from oracle import probe_oracle as po

from probe_refs import GEMM_SHAPES, SOLVE_SHAPES


def test_long_double_is_extended():
    assert np.finfo(np.longdouble).eps < 2e-19
    assert pr.U == 2.0 ** -53


def test_max_ratio_conventions():
    assert pr.max_ratio([0.0, 1.0], [0.0, 4.0]) == 0.25          # 0/0 counts as 0
    assert pr.max_ratio([0.0, 1e-300], [1.0, 0.0]) == np.inf      # x/0 is infinite
    assert pr.max_ratio([np.nan], [1.0]) == np.inf                # NaN never passes
    assert pr.max_ratio([9.0, 1.0], [1.0, 4.0], mask=np.array([False, True])) == 0.25
    assert pr.max_ratio(np.zeros(0), np.zeros(0)) == 0.0


@pytest.mark.parametrize("ta,tb", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_float64_passes(M, N, K, ta, tb):
    A, B, C0 = pr.gemm_operands(M, N, K, ta, tb)
    prod = (A.T if ta else A) @ (B.T if tb else B)
    ref = pr.gemm_products(A, B, ta, tb)
    assert pr.gemm_ratio(A, B, prod, ta, tb, products=ref) < 1
    # another summation order: K in slabs of 528, as split-K sums them
    opa, opb = (A.T if ta else A), (B.T if tb else B)
    slabs = sum(opa[:, k:k + 528] @ opb[k:k + 528] for k in range(0, K, 528))
    assert pr.gemm_ratio(A, B, slabs, ta, tb, products=ref) < 1
    assert pr.gemm_ratio(A, B, -0.5 * prod + 2.0 * C0, ta, tb, -0.5, 2.0, C0, products=ref) < 1


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES[1:])
def test_gemm_defects_fail(M, N, K):
    A, B, C0 = pr.gemm_operands(M, N, K, False, False)
    ref = pr.gemm_products(A, B)
    assert pr.gemm_ratio(A, B, A[:, :-1] @ B[:-1], products=ref) > 1          # drops the last k
    # ignores beta, or takes it for 1
    assert pr.gemm_ratio(A, B, -0.5 * (A @ B), alpha=-0.5, beta=2.0, C0=C0, products=ref) > 1
    assert pr.gemm_ratio(A, B, -0.5 * (A @ B) + C0, alpha=-0.5, beta=2.0, C0=C0, products=ref) > 1
    # reads A with the natural width instead of the leading dimension of its view
    buf, win = pr.embed(A, 0.5)
    start = win[0].start * buf.shape[1] + win[1].start
    wrong = buf.reshape(-1)[start:start + M * K].reshape(M, K)
    np.testing.assert_array_equal(wrong[0], A[0])
    assert pr.gemm_ratio(A, B, wrong @ B, products=ref) > 1
    # an absolute tolerance scaled to the largest entry is blind to the small rows; the bound is not
    small = np.argmin(np.abs(A @ B).max(axis=1))
    off = A @ B
    off[small] *= 1 + 1e-9
    assert np.abs(off - A @ B).max() < 1e-13 * K ** 0.5 * 8 * max(1.0, np.abs(A @ B).max())
    assert pr.gemm_ratio(A, B, off, products=ref) > 1


def test_gemm_mask_and_lower_tiles():
    m = pr.lower_tile_mask(257)
    assert m[0, 127] and not m[0, 128] and m[128, 0] and m[128, 255] and not m[128, 256]
    assert m[256, 256] and m.sum() == 3 * 128 * 128 + 257
    rng = np.random.default_rng(0)
    Z = pr.scaled_normal(rng, 100, 257)
    got = Z.T @ Z
    got[~m] = np.nan                                   # tiles a lower_only GEMM never writes
    assert pr.gemm_ratio(Z, Z, got, True, False, mask=m) < 1
    assert pr.gemm_ratio(Z, Z, got, True, False) == np.inf


def test_embed_and_sentinels():
    a = np.arange(6.0).reshape(2, 3)
    buf, win = pr.embed(a, pr.SENTINEL)
    assert buf.shape == (4, 6) and buf[win].base is buf
    np.testing.assert_array_equal(buf[win], a)
    assert pr.outside_untouched(buf, win)
    buf[win] = -1.0
    assert pr.outside_untouched(buf, win)
    for i, j in ((0, 2), (1, 1), (1, 5), (3, 4)):      # above, left, right (the ld gap), below
        b = buf.copy()
        b[i, j] = np.nextafter(pr.SENTINEL, 0)
        assert not pr.outside_untouched(b, win)


@pytest.mark.parametrize("n", [1, 63, 64, 127, 128, 129, 4097])
def test_colsum_bound(n):
    rng = np.random.default_rng(n)
    X = pr.scaled_normal(rng, n, 5) + 3.0
    X[n // 2, 1], X[n // 3, 2], X[:, 3] = np.inf, -np.inf, 0.1
    assert pr.colsum_ratio(X, X.sum(axis=0)) < 1
    seq = np.zeros(5)
    for row in X:                                       # strict left-to-right order
        seq = seq + row
    assert pr.colsum_ratio(X, seq) < 1
    if n > 1:
        assert pr.colsum_ratio(X, X[:-1].sum(axis=0)) > 1           # drops the last row
    wrong = X.sum(axis=0)
    wrong[1] = -np.inf
    assert pr.colsum_ratio(X, wrong) == np.inf


@pytest.mark.parametrize("parts,count", [(1, 1), (1, 257), (11, 255), (4, 70000)])
def test_sum_parts_bound(parts, count):
    rng = np.random.default_rng(parts + count)
    x = pr.scaled_normal(rng, parts, count)
    assert pr.sum_parts_ratio(x, x.sum(axis=0)) < 1
    if parts > 1:
        assert pr.sum_parts_ratio(x, x[:-1].sum(axis=0)) > 1


@pytest.mark.parametrize("c,n_alpha", [(1, 1), (3, 3), (2, 5)])
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 1000])
def test_r2_two_pass_passes_one_pass_fails(rows, c, n_alpha):
    rng = np.random.default_rng(rows * 31 + c)
    P, c0, T = pr.r2_case(rng, rows, c, n_alpha)
    Pr = P.reshape(rows, n_alpha, c)
    e = T[:, None, :] - (Pr + c0[None])
    tbar = T.sum(axis=0) / rows
    two_pass = np.stack([(e * e).sum(axis=0),
                         np.broadcast_to(((T - tbar) ** 2).sum(axis=0), (n_alpha, c))], axis=2)
    r_res, r_tot = pr.r2_ratio(P, c0, T, two_pass, n_alpha)
    assert r_res < 1 and r_tot < 1
    if rows == 1:
        assert two_pass[0, 0, 1] == 0.0
        return
    one_pass = two_pass.copy()
    one_pass[:, :, 1] = (T * T).sum(axis=0) - rows * tbar * tbar
    assert pr.r2_ratio(P, c0, T, one_pass, n_alpha)[1] > 1
    # the residual expanded the same way: sum (t - b)^2 - 2 (t - b) p + p^2
    tb = T[:, None, :] - c0[None]
    one_pass[:, :, 0] = (tb * tb).sum(axis=0) - 2 * (tb * Pr).sum(axis=0) + (Pr * Pr).sum(axis=0)
    assert pr.r2_ratio(P, c0, T, one_pass, n_alpha)[0] > 1
    # an intercept taken from another alpha
    if n_alpha > 1:
        e = T[:, None, :] - (Pr + np.roll(c0, 1, axis=0)[None])
        swapped = two_pass.copy()
        swapped[:, :, 0] = (e * e).sum(axis=0)
        assert pr.r2_ratio(P, c0, T, swapped, n_alpha)[0] > 1


def test_r2_constant_targets_are_exact():
    rng = np.random.default_rng(5)
    P, c0, T = pr.r2_case(rng, 300, 2, 3, constant=1536.25)
    tbar = T.sum(axis=0) / 300
    assert ((T - tbar) ** 2).sum() == 0.0
    e = T[:, None, :] - (P.reshape(300, 3, 2) + c0[None])
    got = np.stack([(e * e).sum(axis=0), np.zeros((3, 2))], axis=2)
    assert pr.r2_ratio(P, c0, T, got, 3)[1] == 0.0
    got[1, 1, 1] = 1e-300
    assert pr.r2_ratio(P, c0, T, got, 3)[1] == np.inf


@pytest.mark.parametrize("n_cls", [3, 7, 70])
@pytest.mark.parametrize("mask", pr.MASKS)
def test_accuracy_reference_and_defects(n_cls, mask):
    rows, n_alpha = 1000, 3
    P, c0, code, c, present = pr.accuracy_case(rows, n_cls, mask)
    ref = pr.accuracy_ref(P, c0, code, c, n_alpha, n_cls, present)
    S = P.reshape(rows, n_alpha, c) + c0[None]
    # a row-by-row restatement of the rule, first maximum among the present classes
    slow = np.zeros(n_alpha, dtype=np.int64)
    for i in range(rows):
        for a in range(n_alpha):
            best, pred = -np.inf, -1
            for k in range(c):
                if present[k] and (pred < 0 or S[i, a, k] > best):
                    best, pred = S[i, a, k], k
            slow[a] += pred == code[i]
    np.testing.assert_array_equal(ref, slow)
    assert ref.min() > 0 and all(len(set(c0[:, k])) == n_alpha for k in range(c))
    assert (code == -1).any()
    h = rows // 2
    halves = (pr.accuracy_ref(P[:h], c0, code[:h], c, n_alpha, n_cls, present)
              + pr.accuracy_ref(P[h:], c0, code[h:], c, n_alpha, n_cls, present))
    np.testing.assert_array_equal(halves, ref)
    idx = np.flatnonzero(present)
    if mask != "single":
        # the last maximum wins
        last = idx[len(idx) - 1 - np.argmax(S[:, :, idx][:, :, ::-1], axis=2)]
        assert ((last == code[:, None]).sum(axis=0) != ref).any()
    if mask in ("top_absent", "single"):
        # ignores present
        blind = np.argmax(S, axis=2)
        assert ((blind == code[:, None]).sum(axis=0) != ref).any()


def test_accuracy_two_classes_zero_is_class_0():
    rows, n_alpha = 1000, 3
    P, c0, code, c, _ = pr.accuracy_case(rows, 2, "all")
    S = P.reshape(rows, n_alpha, 1) + c0[None]
    assert (S == 0).sum(axis=0).min() > 50                # exact zeros under every alpha
    ref = pr.accuracy_ref(P, c0, code, 1, n_alpha, 2)
    pos, lab = S[:, :, 0] > 0, code[:, None]
    np.testing.assert_array_equal(ref, ((pos & (lab == 1)) | (~pos & (lab == 0))).sum(axis=0))
    ge = ((S[:, :, 0] >= 0).astype(np.int64) == code[:, None]).sum(axis=0)
    assert (ge != ref).all()                              # the rule >= 0


@pytest.mark.parametrize("n,d,c,k", SOLVE_SHAPES)
def test_solve_restatement_passes(n, d, c, k):
    X, Y, sx, sy, folds, edges = pr.solve_case(n, d, c, k)
    W, c0 = pr.solve_restatement(X - sx, Y - sy, edges, po.ALPHAS, folds=k > 1)
    ratio = pr.solve_ratio(X, Y, sx, sy, folds, k, po.ALPHAS, W, c0)
    print(f"RATIO solve_restatement {(n, d, c, k)} {ratio:.3e}")
    assert ratio < 1


@pytest.mark.parametrize("n,d,c,k,alphas", [(200, 63, 1, 3, (0.0, 1e-3, 1e3)),
                                            (400, 129, 1, 3, (0.7,))])
def test_solve_restatement_other_alphas(n, d, c, k, alphas):
    X, Y, sx, sy, folds, edges = pr.solve_case(n, d, c, k)
    W, c0 = pr.solve_restatement(X - sx, Y - sy, edges, alphas)
    ratio = pr.solve_ratio(X, Y, sx, sy, folds, k, alphas, W, c0)
    print(f"RATIO solve_restatement {(n, d, c, k)} {alphas} {ratio:.3e}")
    assert ratio < 1


@pytest.mark.parametrize("n,d,c,k", [(200, 65, 1, 3), (400, 129, 1, 3), (600, 193, 2, 3),
                                     (300, 70, 129, 3)])
def test_solve_defects_fail(n, d, c, k):
    X, Y, sx, sy, folds, edges = pr.solve_case(n, d, c, k)
    for defect in ({"mean_correction": False}, {"alpha_skips_first_panel": True}):
        W, c0 = pr.solve_restatement(X - sx, Y - sy, edges, po.ALPHAS, **defect)
        assert pr.solve_ratio(X, Y, sx, sy, folds, k, po.ALPHAS, W, c0) > 1
    # the existing tolerance of test_batched_ridge_solve_vs_oracle and the tighter one
    W, c0 = pr.solve_restatement(X - sx, Y - sy, edges, po.ALPHAS)
    nudged = W * (1 + 3e-9)
    assert pr.solve_ratio(X, Y, sx, sy, folds, k, po.ALPHAS, nudged, c0) > 1
    assert pr.solve_ratio(X, Y, sx, sy, folds, k, po.ALPHAS, nudged, c0, 1e-7, 1e-9) < 1
