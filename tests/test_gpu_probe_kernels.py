"""Per-kernel GPU tests of the ridge probe (range_amd/csrc/probe_kernels.h, probe_hip.hip) at tile,
panel and stride edges, through ProbeEngine.  Every result is compared with a long-double
reference under a derived bound (tests/probe_refs.py; tests/test_probe_refs_cpu.py shows on the
CPU that the bounds pass float64 arithmetic and fail the planted defects).  Operands are
row-strided views into sentinel-filled buffers: inputs sit in NaN, so a read outside the window
poisons the result, and output padding must keep its bytes.  Each test prints ``RATIO <what>
<max err / bound>`` before it asserts.  Run on an MI355X with ``pytest -m gpu``."""
import ctypes as C

import numpy as np
import pytest
import torch

import probe_refs as pr
from oracle import probe_oracle as po
from range_amd._probe_native import ProbeEngine

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def eng():
    return ProbeEngine("cuda:0")


def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to("cuda:0").contiguous()


def _view(a, fill):
    """``a`` as a row-strided device view (ld = width + 3) inside a buffer filled with ``fill``."""
    buf, win = pr.embed(a, fill)
    t = torch.from_numpy(buf).to("cuda:0")
    v = t[win]
    assert v.stride(0) == a.shape[1] + 3 and not (v.is_contiguous() and a.shape[0] > 1)
    return t, v, win


# ---- GEMM ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ta,tb", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("M,N,K", pr.GEMM_SHAPES)
def test_gemm_strided_views(eng, M, N, K, ta, tb):
    A, B, C0 = pr.gemm_operands(M, N, K, ta, tb)
    ref = pr.gemm_products(A, B, ta, tb)
    _, Av, _ = _view(A, NAN)
    _, Bv, _ = _view(B, NAN)
    for alpha, beta, start in ((1.0, 0.0, np.full((M, N), NAN)), (-0.5, 2.0, C0)):
        Cb, Cv, win = _view(start, pr.SENTINEL)
        assert eng.gemm(Av, Bv, ta, tb, alpha=alpha, beta=beta, out=Cv) is Cv
        after = Cb.cpu().numpy()
        assert np.isfinite(after[win]).all()
        ratio = pr.gemm_ratio(A, B, after[win], ta, tb, alpha, beta, C0, products=ref)
        print(f"RATIO gemm {ratio:.3e}")
        assert ratio <= 1
        assert pr.outside_untouched(after, win)


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("rows", [100, 1024, 4000])
@pytest.mark.parametrize("n", [64, 129, 257])
def test_gemm_lower_only(eng, n, rows, beta):
    rng = np.random.default_rng(n * 5 + rows)
    Z = pr.scaled_normal(rng, rows, n)
    C0 = pr.scaled_normal(rng, n, n)
    start = C0 if beta else np.full((n, n), NAN)
    _, Zv, _ = _view(Z, NAN)
    Cb, Cv, win = _view(start, pr.SENTINEL)
    eng.gemm(Zv, Zv, True, False, beta=beta, out=Cv, lower_only=True)
    after = Cb.cpu().numpy()
    got = after[win]
    lower = pr.lower_tile_mask(n)
    ratio = pr.gemm_ratio(Z, Z, got, True, False, 1.0, beta, C0, mask=lower)
    print(f"RATIO lower_only {ratio:.3e}")
    assert ratio <= 1
    # strictly upper 128-tiles and the padding keep their bytes
    np.testing.assert_array_equal(got[~lower].view(np.int64), start[~lower].view(np.int64))
    assert pr.outside_untouched(after, win)


# ---- column kernels ------------------------------------------------------------------------------
def _column_case(n, d):
    rng = np.random.default_rng(n * 1000 + d)
    X = pr.scaled_normal(rng, n, d) + 3.0
    if d >= 3:
        X[n // 2, 0], X[n // 3, 1], X[:, 2] = np.inf, -np.inf, 0.1
    return rng, X


@pytest.mark.parametrize("d", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("n", [1, 63, 64, 127, 128, 129, 4097])
def test_colstats_and_scale_rows_views(eng, n, d):
    rng, X = _column_case(n, d)
    _, Xv, _ = _view(X, NAN)
    mn, mx, sm = (t.cpu().numpy() for t in eng.colstats(Xv))
    np.testing.assert_array_equal(mn, X.min(axis=0))
    np.testing.assert_array_equal(mx, X.max(axis=0))
    ratio = pr.colsum_ratio(X, sm)
    print(f"RATIO colsum {ratio:.3e}")
    assert ratio <= 1
    scale, off = rng.uniform(0.5, 2.0, size=d), rng.standard_normal(d)
    shift = rng.standard_normal(d)
    sc, of, sh = _dev(scale), _dev(off), _dev(shift)
    np.testing.assert_array_equal(eng.scale_rows(Xv, shift=sh).cpu().numpy(), X - shift)
    np.testing.assert_array_equal(eng.scale_rows(Xv, scale=sc, offset=of).cpu().numpy(),
                                  po.minmax_apply(X, scale, off))
    perm = rng.integers(0, n, size=n + 5)               # repeats, longer than n
    want = po.minmax_apply(X[perm], scale, off) - shift
    np.testing.assert_array_equal(
        eng.scale_rows(Xv, _dev(perm, torch.int64), sc, of, sh).cpu().numpy(), want)
    Zb, Zv, win = _view(np.full((n + 5, d), NAN), pr.SENTINEL)
    assert eng.scale_rows(Xv, _dev(perm, torch.int64), sc, of, sh, out=Zv) is Zv
    after = Zb.cpu().numpy()
    np.testing.assert_array_equal(after[win], want)
    assert pr.outside_untouched(after, win)


@pytest.mark.parametrize("n,d", [(1, 1), (63, 65), (129, 64), (4097, 3)])
def test_colstats_null_outputs(eng, n, d):
    """The C ABI's optional outputs (range_probe_gram passes only the sum)."""
    _, X = _column_case(n, d)
    _, Xv, _ = _view(X, NAN)
    want = (X.min(axis=0), X.max(axis=0))
    for skip in range(3):
        outs = [torch.full((d,), pr.SENTINEL, dtype=torch.float64, device="cuda:0")
                for _ in range(3)]
        ptrs = [None if i == skip else C.c_void_p(o.data_ptr()) for i, o in enumerate(outs)]
        rc = eng.lib.range_probe_colstats(eng._h, Xv.data_ptr(), n, d, Xv.stride(0), *ptrs,
                                          torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        mn, mx, sm = (o.cpu().numpy() for o in outs)
        np.testing.assert_array_equal(outs[skip].cpu().numpy(), np.full(d, pr.SENTINEL))
        if skip != 0:
            np.testing.assert_array_equal(mn, want[0])
        if skip != 1:
            np.testing.assert_array_equal(mx, want[1])
        if skip != 2:
            assert pr.colsum_ratio(X, sm) <= 1


@pytest.mark.parametrize("first", [0, 1, 5])
@pytest.mark.parametrize("c", [1, 3, 70])
def test_onehot(eng, c, first):
    rng = np.random.default_rng(c * 10 + first)
    code = rng.integers(-1, first + c + 2, size=301).astype(np.int32)
    assert (code == -1).any() and (code == first).any()
    shift = rng.standard_normal(c)
    T = eng.onehot(_dev(code, torch.int32), c, first, _dev(shift)).cpu().numpy()
    want = np.where(code[:, None] == first + np.arange(c)[None], 1.0, -1.0) - shift
    np.testing.assert_array_equal(T, want)


@pytest.mark.parametrize("parts,count", [(1, 1), (1, 257), (11, 255), (4, 70000)])
def test_sum_parts(eng, parts, count):
    x = pr.scaled_normal(np.random.default_rng(parts + count), parts, count)
    got = eng.sum_parts(_dev(x)).cpu().numpy()
    ratio = pr.sum_parts_ratio(x, got)
    print(f"RATIO sum_parts {ratio:.3e}")
    assert ratio <= 1


# ---- gram ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,c", [(1, 1), (65, 3), (129, 70)])
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 1023, 1025])
def test_gram_strided_views(eng, rows, d, c):
    rng = np.random.default_rng(rows * 7 + d)
    Z, T = pr.scaled_normal(rng, rows, d), pr.scaled_normal(rng, rows, c)
    _, Zv, _ = _view(Z, NAN)
    _, Tv, _ = _view(T, NAN)
    G, B = _dev(np.full((d, d), NAN)), _dev(np.full((d, c), NAN))
    zsum, tsum = _dev(np.full(d, NAN)), _dev(np.full(c, NAN))
    eng.gram(Zv, Tv, G, B, zsum, tsum)
    G = G.cpu().numpy()
    r_g = pr.gemm_ratio(Z, Z, G, True, False, mask=np.tri(d, dtype=bool))
    r_b = pr.gemm_ratio(Z, T, B.cpu().numpy(), True, False)
    r_s = max(pr.colsum_ratio(Z, zsum.cpu().numpy()), pr.colsum_ratio(T, tsum.cpu().numpy()))
    print(f"RATIO gram {max(r_g, r_b):.3e}")
    print(f"RATIO colsum {r_s:.3e}")
    assert r_g <= 1 and r_b <= 1 and r_s <= 1
    assert np.isnan(G[~pr.lower_tile_mask(d)]).all()   # tiles above the diagonal are not written


# ---- solve ---------------------------------------------------------------------------------------
def _solve(eng, n, d, c, k, alphas):
    X, Y, sx, sy, folds, edges = pr.solve_case(n, d, c, k)
    Z, T = _dev(X - sx), _dev(Y - sy)
    kk = max(k, 1)
    Gf, Bf = eng.empty((kk, d, d)), eng.empty((kk, d, c))
    zs, ts = eng.empty((kk, d)), eng.empty((kk, c))
    for f in range(kk):
        eng.gram(Z[edges[f]:edges[f + 1]], T[edges[f]:edges[f + 1]], Gf[f], Bf[f], zs[f], ts[f])
    Gt, Bt, zt, tt = eng.sum_parts(Gf), eng.sum_parts(Bf), eng.sum_parts(zs), eng.sum_parts(ts)
    if k > 1:
        ntr = [float(n - (edges[f + 1] - edges[f])) for f in range(k)]
        W, c0 = eng.solve(Gt, Bt, zt, tt, ntr, alphas, Gf, Bf, zs, ts)
    else:
        W, c0 = eng.solve(Gt, Bt, zt, tt, [float(n)], alphas)
    ratio = pr.solve_ratio(X, Y, sx, sy, folds, k, alphas, W.cpu().numpy(), c0.cpu().numpy())
    print(f"RATIO solve {(n, d, c, k)} {ratio:.3e}")
    return ratio


@pytest.mark.parametrize("n,d,c,k", pr.SOLVE_SHAPES)
def test_solve_panel_edges(eng, n, d, c, k):
    assert _solve(eng, n, d, c, k, po.ALPHAS) <= 1


@pytest.mark.parametrize("n,d,c,k,alphas", [(200, 63, 1, 3, (0.0, 1e-3, 1e3)),
                                            (400, 129, 1, 3, (0.7,))])
def test_solve_other_alphas(eng, n, d, c, k, alphas):
    assert _solve(eng, n, d, c, k, alphas) <= 1


def test_solve_errors_are_returns(eng):
    d, c = 70, 2
    rng = np.random.default_rng(70)
    B, zero_d, zero_c = _dev(rng.standard_normal((d, c))), _dev(np.zeros(d)), _dev(np.zeros(c))
    diag = np.ones(d)
    diag[66] = -1.0
    # alpha 0.5 leaves -0.5 at index 66 (second panel); alpha 2 makes the system definite
    with pytest.raises(RuntimeError, match=r"alpha 0\.5\).*positive definite at pivot 67$"):
        eng.solve(_dev(np.diag(diag)), B, zero_d, zero_c, [10.0], [0.5, 2.0])
    for at in (3, 66):
        G = np.eye(d)
        G[at, at] = NAN
        with pytest.raises(RuntimeError, match=f"positive definite at pivot {at + 1}$"):
            eng.solve(_dev(G), B, zero_d, zero_c, [10.0], [0.5, 2.0])
    # the same engine solves a good system afterwards
    M = rng.standard_normal((200, d))
    G = M.T @ M
    W, c0 = eng.solve(_dev(G), B, zero_d, zero_c, [200.0], [0.5, 2.0])
    W = W.cpu().numpy()
    for a, alpha in enumerate((0.5, 2.0)):
        Wr = np.linalg.solve(G + alpha * np.eye(d), B.cpu().numpy())
        np.testing.assert_allclose(W[0, :, a, :], Wr, rtol=pr.SOLVE_RTOL, atol=pr.SOLVE_ATOL)
    np.testing.assert_array_equal(c0.cpu().numpy(), np.zeros((1, 2, c)))


# ---- scores --------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,n_alpha", [(1, 1), (3, 3), (2, 5)])
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 1000])
def test_r2_sums(eng, rows, c, n_alpha):
    P, c0, T = pr.r2_case(np.random.default_rng(rows * 31 + c), rows, c, n_alpha)
    got = eng.r2_sums(_dev(P), _dev(c0), _dev(T), _dev(T.sum(axis=0)), n_alpha).cpu().numpy()
    r_res, r_tot = pr.r2_ratio(P, c0, T, got, n_alpha)
    print(f"RATIO r2_sums {max(r_res, r_tot):.3e}")
    assert r_res <= 1 and r_tot <= 1
    if rows == 1:
        np.testing.assert_array_equal(got[:, :, 1], 0.0)


@pytest.mark.parametrize("rows", [255, 256, 257])
def test_r2_sums_constant_targets(eng, rows):
    P, c0, T = pr.r2_case(np.random.default_rng(rows), rows, 2, 3, constant=1536.25)
    got = eng.r2_sums(_dev(P), _dev(c0), _dev(T), _dev(T.sum(axis=0)), 3).cpu().numpy()
    np.testing.assert_array_equal(got[:, :, 1], 0.0)
    assert pr.r2_ratio(P, c0, T, got, 3)[0] <= 1


@pytest.mark.parametrize("n_cls", [2, 3, 7, 70])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_accuracy(eng, rows, n_cls):
    n_alpha = 3
    for mask in (pr.MASKS if n_cls > 2 else pr.MASKS[:1]):
        P, c0, code, c, present = pr.accuracy_case(rows, n_cls, mask)
        if n_cls == 2 and rows >= 63:
            assert ((P + c0.reshape(1, -1)) == 0).any(axis=0).all()      # exact zeros: class 0
        want = pr.accuracy_ref(P, c0, code, c, n_alpha, n_cls, present)
        Pd, c0d, cd = _dev(P), _dev(c0), _dev(code, torch.int32)
        pd = None if present is None else _dev(present, torch.int32)
        got = eng.accuracy(Pd, c0d, cd, c, n_alpha, n_cls, pd).cpu().numpy()
        np.testing.assert_array_equal(got, want, err_msg=mask)
        # labels of -1 alone: never a hit
        none = eng.accuracy(Pd, c0d, torch.full_like(cd, -1), c, n_alpha, n_cls, pd)
        np.testing.assert_array_equal(none.cpu().numpy(), np.zeros(n_alpha, dtype=np.int64))
        if rows > 1:
            h = rows // 2
            halves = (eng.accuracy(Pd[:h], c0d, cd[:h], c, n_alpha, n_cls, pd)
                      + eng.accuracy(Pd[h:], c0d, cd[h:], c, n_alpha, n_cls, pd))
            np.testing.assert_array_equal(halves.cpu().numpy(), want, err_msg=mask)


def test_score_entry_points_validate(eng):
    rows, c, n_alpha = 12, 3, 2
    P, c0, T = pr.r2_case(np.random.default_rng(0), rows, c, n_alpha)
    Pd, c0d, Td, ts = _dev(P), _dev(c0), _dev(T), _dev(T.sum(axis=0))
    eng.r2_sums(Pd, c0d, Td, ts, n_alpha)
    code, present = _dev(np.zeros(rows), torch.int32), _dev(np.ones(c), torch.int32)
    eng.accuracy(Pd, c0d, code, c, n_alpha, c, present)
    eng.accuracy(Pd, c0d.reshape(-1), code, c, n_alpha, c, present)
    transposed = _dev(P.T.copy()).t()
    assert tuple(transposed.shape) == (rows, n_alpha * c)
    for bad in (lambda: eng.r2_sums(transposed, c0d, Td, ts, n_alpha),
                lambda: eng.r2_sums(_dev(P.T.copy()), c0d, Td, ts, n_alpha),
                lambda: eng.r2_sums(Pd, c0d, _dev(T, torch.float32), ts, n_alpha),
                lambda: eng.r2_sums(Pd, c0d[:1], Td, ts, n_alpha),
                lambda: eng.r2_sums(Pd, c0d, Td, ts[:2], n_alpha),
                lambda: eng.r2_sums(Pd.cpu(), c0d, Td, ts, n_alpha),
                lambda: eng.accuracy(transposed, c0d, code, c, n_alpha, c, present),
                lambda: eng.accuracy(Pd, c0d[:1], code, c, n_alpha, c, present),
                lambda: eng.accuracy(Pd, c0d, code[:5], c, n_alpha, c, present),
                lambda: eng.accuracy(Pd, c0d, code, c, n_alpha, c, present[:2])):
        with pytest.raises(ValueError):
            bad()


def test_views_the_engine_refuses(eng):
    t = torch.zeros((8, 8), dtype=torch.float64, device="cuda:0")
    for bad in (t.t(), t[:, ::2], t.as_strided((4, 8), (4, 1)),
                t.to(torch.float32), t.cpu(), t[0]):
        with pytest.raises(ValueError):
            eng.colstats(bad)
        with pytest.raises(ValueError):
            eng.gemm(bad, t)
    col = t[:, 3:4]                                      # one column wide: any column stride
    assert not col.is_contiguous()
    np.testing.assert_array_equal(eng.colstats(col)[2].cpu().numpy(), [0.0])
