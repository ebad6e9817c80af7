"""Plain references for the ridge-probe kernels (include/range_probe.h), with derived bounds.

Every ``*_ratio`` helper takes the inputs of one operation and the array ``got`` that the code
under test produced, evaluates the operation in ``numpy.longdouble`` (80-bit here) and returns
``max(err / bound)`` over all elements: a correct float64 evaluation stays below 1 whatever its
summation order, a wrong one does not.  A zero bound with zero error counts as 0, a zero bound with
a non-zero error (or a NaN anywhere) as infinite.  tests/test_probe_refs_cpu.py shows both halves
on the CPU; tests/test_gpu_probe_kernels.py applies the helpers to the HIP kernels.

Bounds (u = 2^-53, Higham, Accuracy and Stability of Numerical Algorithms, ch. 3):

* GEMM  C = alpha op(A) op(B) + beta C0:  (K + 4) u (|alpha| |op A| |op B| + |beta| |C0|).  The
  dot-product bound gamma_K holds for every summation order, so it covers the MFMA order and the
  split-K slabs; + 4 pays for alpha, beta and the final sum.
* column sums: (n + 4) u sum |x|; sums of parts: (parts + 2) u sum |x|.
* R^2 residual: u [(rows + 16) res + 4 sum |e_i| (|t_i| + |p_i| + |b|)], e_i = t_i - (p_i + b):
  two roundings in e_i (relative to the magnitudes that were added), one in the square, gamma_rows
  for the sum.  Total: the same with e_i = t_i - tbar.  The one-pass form sum t^2 - n tbar^2 misses
  this bound by two orders of magnitude on targets of 1e3 + N(0, 1): that is what it is for.
* ridge solve: |got - ref| <= atol + rtol |ref| against oracle.ridge_fit on the training rows, in
  the shifted coordinates of the kernels.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import scipy.linalg

from oracle import probe_oracle as po

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "the references need an extended-precision long double"
U = 2.0 ** -53
TILE = 128              # C tile of dgemm_kernel: lower_only skips whole tiles above the diagonal
PANEL = 64              # Cholesky panel width
SOLVE_RTOL, SOLVE_ATOL = 1e-9, 1e-11
SENTINEL = 1.2345e77    # what the padding of an output view holds


# (M, N, K): ragged tiles, a ragged K stage, both sides of the split-K edge at K = 1024
GEMM_SHAPES = [(1, 1, 1), (127, 129, 15), (128, 128, 16), (129, 127, 17), (257, 65, 1023),
               (130, 70, 1024), (70, 130, 1025), (128, 128, 2049)]
# (n, d, c, k): d around the panel edges 64, 128, 192; c around the 64-column grid edge of the
# triangular solves; n_alpha * c around 64; fewer training rows than features; k = 1 and 10
SOLVE_SHAPES = [(40, 1, 1, 3), (200, 63, 1, 3), (200, 64, 2, 3), (200, 65, 1, 3),
                (400, 127, 1, 3), (400, 128, 3, 3), (400, 129, 1, 3), (600, 193, 2, 3),
                (300, 40, 64, 3), (300, 40, 65, 3), (300, 70, 129, 3), (300, 33, 22, 3),
                (90, 129, 2, 3), (60, 200, 1, 3), (50, 1, 1, 1), (300, 64, 1, 10)]


def _ld(a) -> np.ndarray:
    return np.asarray(a, dtype=LD)


def max_ratio(err, bound, mask=None) -> float:
    """max(err / bound); 0/0 counts as 0, x/0 and NaN as infinite."""
    err, bound = np.broadcast_arrays(_ld(err), _ld(bound))
    if mask is not None:
        err, bound = err[mask], bound[mask]
    if err.size == 0:
        return 0.0
    out = np.zeros(err.shape, dtype=LD)
    pos = bound > 0
    out[pos] = err[pos] / bound[pos]
    out[~pos & (err != 0)] = np.inf
    out[np.isnan(err) | np.isnan(bound)] = np.inf
    return float(out.max())


def _abs_err(got, ref) -> np.ndarray:
    """|got - ref| with equal infinities counting as exact."""
    got, ref = _ld(got), _ld(ref)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref)
    err[np.isinf(ref) & (got == ref)] = 0
    return err


# ---- input generators shared by the CPU and the GPU tests ----------------------------------------
def scaled_normal(rng, rows: int, cols: int) -> np.ndarray:
    """Standard normal, rows and columns scaled by exp(U(-6, 6)): eleven orders of magnitude."""
    return (rng.standard_normal((rows, cols)) * np.exp(rng.uniform(-6, 6, size=(rows, 1)))
            * np.exp(rng.uniform(-6, 6, size=(1, cols))))


def gemm_operands(M, N, K, ta, tb):
    """Stored A (K x M when ta), stored B (N x K when tb) and C0 (M x N)."""
    rng = np.random.default_rng(M * 7 + N * 3 + K + 2 * ta + tb)
    A = scaled_normal(rng, *((K, M) if ta else (M, K)))
    B = scaled_normal(rng, *((N, K) if tb else (K, N)))
    C0 = scaled_normal(rng, M, N)
    return A, B, C0


def embed(a: np.ndarray, fill: float) -> Tuple[np.ndarray, Tuple[slice, slice]]:
    """``a`` inside a larger buffer filled with ``fill``: leading dimension width + 3, two extra
    rows.  Returns the buffer and the window's index; ``buf[win]`` is a row-strided view."""
    rows, width = a.shape
    buf = np.full((rows + 2, width + 3), fill, dtype=np.float64)
    win = (slice(1, 1 + rows), slice(2, 2 + width))
    buf[win] = a
    return buf, win


def outside_untouched(buf_after: np.ndarray, win, fill: float = SENTINEL) -> bool:
    """Every byte outside the window still holds the fill."""
    keep = np.ones(buf_after.shape, dtype=bool)
    keep[win] = False
    want = np.full(1, fill, dtype=np.float64).view(np.int64)[0]
    return bool(np.all(np.ascontiguousarray(buf_after).view(np.int64)[keep] == want))


def lower_tile_mask(n: int) -> np.ndarray:
    """Elements of the 128-tiles on or below the diagonal (diagonal tiles in full)."""
    t = np.arange(n) // TILE
    return t[None, :] <= t[:, None]


def solve_case(n: int, d: int, c: int, k: int):
    """The generator of test_batched_ridge_solve_vs_oracle: X, Y, the shifts and fold edges."""
    rng = np.random.default_rng(n + d)
    X = rng.uniform(0, 1, size=(n, d)) * rng.uniform(0.2, 1.0, size=d)
    Y = X @ rng.standard_normal((d, c)) + 0.1 * rng.standard_normal((n, c)) + 3.0
    shift_x, shift_y = X.mean(axis=0) + 0.01, Y.mean(axis=0) - 0.02     # any origin must work
    folds = po.kfold_ids(n, k) if k > 1 else np.zeros(n, dtype=np.int64)
    edges = np.concatenate([[0], np.cumsum(np.bincount(folds))])
    return X, Y, shift_x, shift_y, folds, edges


def r2_case(rng, rows: int, c: int, n_alpha: int, constant: Optional[float] = None):
    """Targets 1e3 + N(0, 1), predictions P = T - noise - c0 with one c0 per (alpha, target)."""
    T = (np.full((rows, c), constant) if constant is not None
         else 1e3 + rng.standard_normal((rows, c)))
    c0 = 3.0 * (1 + np.arange(n_alpha * c, dtype=np.float64).reshape(n_alpha, c)) \
        + rng.standard_normal((n_alpha, c))
    noise = 0.3 * rng.standard_normal((rows, n_alpha, c))
    P = (T[:, None, :] - noise - c0[None]).reshape(rows, n_alpha * c)
    return P, c0, T


# ---- GEMM ----------------------------------------------------------------------------------------
def gemm_products(A, B, ta: bool = False, tb: bool = False):
    """(op(A) op(B), |op A| |op B|, K) in long double: computed once, shared between checks."""
    opa = _ld(A).T if ta else _ld(A)
    opb = _ld(B).T if tb else _ld(B)
    return opa @ opb, np.abs(opa) @ np.abs(opb), opa.shape[1]


def gemm_ratio(A, B, got, ta: bool = False, tb: bool = False, alpha: float = 1.0,
               beta: float = 0.0, C0=None, mask=None, products=None) -> float:
    prod, absprod, K = products if products is not None else gemm_products(A, B, ta, tb)
    ref = LD(alpha) * prod
    bound = abs(LD(alpha)) * absprod
    if beta != 0.0:
        ref = ref + LD(beta) * _ld(C0)
        bound = bound + abs(LD(beta)) * np.abs(_ld(C0))
    return max_ratio(_abs_err(got, ref), (K + 4) * LD(U) * bound, mask)


# ---- column kernels ------------------------------------------------------------------------------
def colsum_ratio(X, got, extra: int = 4) -> float:
    """Column sums within (n + extra) u sum|x|; a column whose sum is infinite must be equal."""
    X = _ld(X)
    with np.errstate(invalid="ignore"):
        ref = X.sum(axis=0)
        bound = (X.shape[0] + extra) * LD(U) * np.abs(X).sum(axis=0)
    bound[np.isinf(ref)] = 0
    return max_ratio(_abs_err(got, ref), bound)


def sum_parts_ratio(parts, got) -> float:
    p = np.asarray(parts)
    flat = p.reshape(p.shape[0], -1)
    return colsum_ratio(flat, np.asarray(got).reshape(-1), extra=2)


# ---- scores --------------------------------------------------------------------------------------
def r2_ratio(P, c0, T, got, n_alpha: int) -> Tuple[float, float]:
    """(ratio of the residual sums, ratio of the total sums) of got (n_alpha, c, 2)."""
    T = _ld(T)
    rows, c = T.shape
    P = _ld(P).reshape(rows, n_alpha, c)
    b = _ld(c0).reshape(1, n_alpha, c)
    t = T[:, None, :]
    e = t - (P + b)
    ref_res = (e * e).sum(axis=0)
    bound_res = LD(U) * ((rows + 16) * ref_res
                         + 4 * (np.abs(e) * (np.abs(t) + np.abs(P) + np.abs(b))).sum(axis=0))
    tbar = T.sum(axis=0) / rows
    e2 = T - tbar
    ref_tot = (e2 * e2).sum(axis=0)
    bound_tot = LD(U) * ((rows + 16) * ref_tot
                         + 4 * (np.abs(e2) * (np.abs(T) + np.abs(tbar))).sum(axis=0))
    got = np.asarray(got).reshape(n_alpha, c, 2)
    return (max_ratio(_abs_err(got[:, :, 0], ref_res), bound_res),
            max_ratio(_abs_err(got[:, :, 1], np.broadcast_to(ref_tot, (n_alpha, c))),
                      np.broadcast_to(bound_tot, (n_alpha, c))))


def accuracy_pred(P, c0, c: int, n_alpha: int, n_cls: int, present=None) -> np.ndarray:
    """Predicted class (rows, n_alpha): arg-max over the present classes, first maximum wins;
    two classes: score > 0.  The scores are the float64 sums p + c0 the kernel forms."""
    P = np.asarray(P, dtype=np.float64)
    S = P.reshape(P.shape[0], n_alpha, c) + np.asarray(c0, dtype=np.float64).reshape(1, n_alpha, c)
    if n_cls == 2:
        return (S[:, :, 0] > 0).astype(np.int64)
    idx = np.flatnonzero(np.asarray(present))
    return idx[np.argmax(S[:, :, idx], axis=2)]


def accuracy_ref(P, c0, code, c: int, n_alpha: int, n_cls: int, present=None) -> np.ndarray:
    """Exact hit counts (n_alpha,) int64; a code of -1 is never a hit."""
    pred = accuracy_pred(P, c0, c, n_alpha, n_cls, present)
    return (pred == np.asarray(code).reshape(-1, 1)).sum(axis=0).astype(np.int64)


MASKS = ("all", "no0", "top_absent", "single")


def accuracy_case(rows, n_cls, mask, n_alpha=3):
    """Scores from {-2..2}/4, dyadic intercepts that differ per alpha; ``mask`` in all, no0,
    top_absent, single (ignored for two classes).  Returns P, c0, code, c, present."""
    rng = np.random.default_rng(rows * 131 + n_cls * 7 + len(mask))
    c = 1 if n_cls == 2 else n_cls
    P = rng.integers(-2, 3, size=(rows, n_alpha * c)) / 4.0
    # every class sees each of the n_alpha intercepts once, in an order of its own
    c0 = ((np.arange(n_alpha)[:, None] + rng.integers(0, n_alpha, size=(1, c))) % n_alpha
          - n_alpha // 2) / 4.0
    code = rng.integers(-1, n_cls, size=rows).astype(np.int32)
    if n_cls == 2:
        return P, c0, code, c, None
    present = np.ones(n_cls, dtype=np.int32)
    if mask == "no0":
        present[0] = 0
    elif mask == "top_absent":
        present[1::3] = 0
        P.reshape(rows, n_alpha, c)[:, :, 1::3] += 1.0
    elif mask == "single":
        present[:] = 0
        present[n_cls // 2] = 1
    # half of the rows carry the label the first-maximum rule picks for one of the alphas
    pred = accuracy_pred(P, c0, c, n_alpha, n_cls, present)
    pick = rng.random(rows) < 0.5
    code[pick] = pred[pick, rng.integers(0, n_alpha, size=rows)[pick]]
    return P, c0, code, c, present


# ---- ridge solve ---------------------------------------------------------------------------------
def solve_ratio(X, Y, shift_x, shift_y, folds, k: int, alphas: Sequence[float], W, c0,
                rtol: float = SOLVE_RTOL, atol: float = SOLVE_ATOL) -> float:
    """W (groups, d, n_alpha, c), c0 (groups, n_alpha, c) against oracle.ridge_fit on the training
    rows of every fold (k == 1: all rows); intercept in the shifted coordinates
    y - shift_y = (x - shift_x) . W + c0.  Returns max |got - ref| / (atol + rtol |ref|)."""
    worst = 0.0
    for f in range(max(k, 1)):
        tr = folds != f if k > 1 else np.ones(X.shape[0], bool)
        for a, alpha in enumerate(alphas):
            Wr, br = po.ridge_fit(X[tr], Y[tr], alpha)
            cr = br - shift_y + shift_x @ Wr
            worst = max(worst,
                        max_ratio(_abs_err(W[f, :, a, :], Wr), atol + rtol * np.abs(Wr)),
                        max_ratio(_abs_err(c0[f, a], cr), atol + rtol * np.abs(cr)))
    return worst


def solve_restatement(Z, T, edges, alphas: Sequence[float], folds: bool = True,
                      mean_correction: bool = True, alpha_skips_first_panel: bool = False):
    """The kernels' own algorithm in float64 numpy: per-fold Gram statistics, "all rows but fold
    g" as differences, the rank-one mean correction n delta delta^T, Cholesky.  The two flags
    plant the defects the comparison must catch.  Returns W (groups, d, n_alpha, c) and
    c0 (groups, n_alpha, c)."""
    Z, T = np.asarray(Z, dtype=np.float64), np.asarray(T, dtype=np.float64)
    n, d = Z.shape
    c = T.shape[1]
    groups = len(edges) - 1
    Gf = np.stack([Z[edges[g]:edges[g + 1]].T @ Z[edges[g]:edges[g + 1]] for g in range(groups)])
    Bf = np.stack([Z[edges[g]:edges[g + 1]].T @ T[edges[g]:edges[g + 1]] for g in range(groups)])
    sf = np.stack([Z[edges[g]:edges[g + 1]].sum(axis=0) for g in range(groups)])
    tf = np.stack([T[edges[g]:edges[g + 1]].sum(axis=0) for g in range(groups)])
    Gt, Bt, st, tt = Gf.sum(axis=0), Bf.sum(axis=0), sf.sum(axis=0), tf.sum(axis=0)
    W = np.empty((groups, d, len(alphas), c))
    c0 = np.empty((groups, len(alphas), c))
    for g in range(groups):
        if folds:
            ntr = float(n - (edges[g + 1] - edges[g]))
            G, B, s, t = Gt - Gf[g], Bt - Bf[g], st - sf[g], tt - tf[g]
        else:
            ntr, G, B, s, t = float(n), Gt, Bt, st, tt
        delta = s / ntr
        A0 = G - np.outer(delta, s) if mean_correction else G.copy()
        R = B - np.outer(delta, t)
        for a, alpha in enumerate(alphas):
            A = A0.copy()
            diag = np.diag_indices(d)
            if alpha_skips_first_panel:
                A[diag[0][PANEL:], diag[1][PANEL:]] += alpha
            else:
                A[diag] += alpha
            w = scipy.linalg.cho_solve(scipy.linalg.cho_factor(A, lower=True), R)
            W[g, :, a, :] = w
            c0[g, a] = t / ntr - delta @ w
    return W, c0
