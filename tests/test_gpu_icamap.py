"""GPU tests of the embedding map (map_kernels.h, include/range_map.h, range_amd/embedding_map.py,
tools/embedding_map.py): every kernel through the C ABI against long-double numpy at the wave, workgroup-share and
capped-grid edges; results bit for bit across calls, streams and grids; ``ica_colors`` on the fixtures scikit-learn
produced (tests/golden/icamap.npz; the restatements are pinned to it by tests/test_icamap_cpu.py); the model driver
and the command-line tool end to end.  Run with ``pytest -m gpu``.

Bounds (set by the design, not by what the kernels give): projection (d + 2) 2^-53 sum|terms| per output; ICA step
(n + 8) 2^-53 sum|terms| per sum - n 2^-53 is the any-order summation bound, 8 an allowance for the device tanh /
exp and the product roundings; histogram counts exactly numpy.histogram's; equalised values within 2^-50 of the
numpy restatement; ``ica_colors`` sources within 100 d_ref of scikit-learn's, d_ref being scikit-learn's own movement
between its two whitening solvers."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import icamap_refs as R
from range_amd import _map_native
from range_amd.embedding_map import ConvergenceWarning, coord_grid, embedding_map, ica_colors

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
L = np.longdouble
SHARE = 1024                       # rows of one ICA-step slab at these sizes (asserted against the plan below)
PROJ_SHARE = 32                    # rows of one projection trip of a workgroup
PAIRS = [(1, 1), (2, 3), (3, 64), (5, 65), (8, 130)]
RUNS = [("synth_600x50", "c3", 3, 1000), ("synth_601x130", "c3", 3, 1000), ("sphere_640x96", "c3", 3, 1000),
        ("sphere_640x96", "c2", 2, 1000), ("sphere_640x96", "c5", 5, 1000)]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "icamap.npz"))


@pytest.fixture(scope="module")
def engine():
    return _map_native.MapEngine(DEV)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def strided(a, pad):
    """A device copy of the 2-d host array whose rows are `pad` elements apart beyond their length (NaN between)."""
    buf = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=torch.float64, device=DEV)
    buf[:, :a.shape[1]] = dev(a)
    return buf[:, :a.shape[1]]


def test_plan_constants():
    p = _map_native.plan(257, 3)
    assert p["chunk"] == SHARE and p["proj_rows"] == PROJ_SHARE and p["slabs"] == 1
    assert _map_native.plan(3 * SHARE + 1, 3, 3)["slabs"] == 4 and _map_native.plan(3 * SHARE + 1, 3, 3)["step_grid"] == 3


# ---- projection ---------------------------------------------------------------------------------------------------
def project_case(engine, n, c, d, pad, max_grid=0, with_mean=True, seed=0):
    rng = np.random.default_rng(1000 * n + 10 * d + c + seed)
    X = rng.standard_normal((n, d)) * rng.uniform(0.5, 3.0, d) + rng.uniform(-2, 2, d)
    mean = rng.uniform(-2, 2, d) if with_mean else None
    K = rng.standard_normal((c, d))
    Xd = strided(X, pad)
    got = engine.project(Xd, dev(K), None if mean is None else dev(mean), max_grid=max_grid).cpu().numpy()
    want, bound = R.project_ld(X, mean, K)
    err = np.abs(got.astype(L) - want)
    assert got.shape == (c, n) and (err <= bound).all(), f"n={n} c={c} d={d}: worst error/bound {(err / bound).max():.3f}"
    return got


@pytest.mark.parametrize("n", [1, 31, 33, 63, 64, 65, 255, 256, 257, SHARE - 1, SHARE + 1])
@pytest.mark.parametrize("c,d", PAIRS)
def test_project_rows(engine, n, c, d):
    project_case(engine, n, c, d, pad=3 if (n + d) % 2 else 2)


@pytest.mark.parametrize("c", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("d", [1, 3, 64, 65, 130])
def test_project_shapes_and_capped_grid(engine, c, d):
    """Every c with every d; 3 workgroups for 3 * 32 + 1 rows: workgroup 0 makes a second trip.  The capped grid,
    a second call and another stream give the same bits; contiguous rows (16-byte loads when d is even)."""
    n = 3 * PROJ_SHARE + 1
    assert _map_native.plan(n, c, 3)["proj_grid"] == 3
    a = project_case(engine, n, c, d, pad=0, max_grid=3)
    b = project_case(engine, n, c, d, pad=0)
    assert np.array_equal(a, b)
    with torch.cuda.stream(torch.cuda.Stream(DEV)):
        e = project_case(engine, n, c, d, pad=0)
    assert np.array_equal(a, e)
    project_case(engine, n, c, d, pad=1, with_mean=False)


# ---- ICA step -----------------------------------------------------------------------------------------------------
def step_inputs(n, c, seed=0):
    """Whitened data as the algorithm sees it: unit-variance rows, W orthonormal (a decorrelated Gaussian draw)."""
    rng = np.random.default_rng(77 * n + c + seed)
    return rng.standard_normal((c, n)), R.sym_decorrelation(rng.standard_normal((c, c)))


def step_case(engine, n, c, pad=0, max_grid=0):
    Y, W = step_inputs(n, c)
    engine.reserve(n, c)
    out = engine.ica_step(strided(Y, pad), W, max_grid=max_grid).cpu().numpy()
    A, b, bound_A, bound_b = R.ica_step_ld(Y, W)
    err_A = np.abs(out[:c * c].reshape(c, c).astype(L) - A)
    err_b = np.abs(out[c * c:].astype(L) - b)
    assert (err_A <= bound_A).all() and (err_b <= bound_b).all(), \
        f"n={n} c={c}: worst error/bound A {(err_A / bound_A).max():.3f} b {(err_b / bound_b).max():.3f}"
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, SHARE - 1, SHARE + 1])
@pytest.mark.parametrize("c", [1, 2, 3, 5, 8])
def test_ica_step_rows(engine, n, c):
    step_case(engine, n, c, pad=5 if n % 2 else 0)


@pytest.mark.parametrize("c", [1, 2, 3, 5, 8])
def test_ica_step_is_bit_identical(engine, c):
    """One row beyond a full capped grid (3 workgroups, 4 slabs: workgroup 0 makes a second trip) - the slabs are cut
    by n alone, so the capped grid, the plan's own grid, a second call and another stream give the same bits."""
    n = 3 * SHARE + 1
    a = step_case(engine, n, c, max_grid=3)
    assert np.array_equal(a, step_case(engine, n, c)) and np.array_equal(a, step_case(engine, n, c, max_grid=1))
    with torch.cuda.stream(torch.cuda.Stream(DEV)):
        e = step_case(engine, n, c)
    assert np.array_equal(a, e)


def test_ica_step_needs_its_workspace():
    eng = _map_native.MapEngine(DEV)
    Y, W = step_inputs(5000, 3)
    with pytest.raises(_map_native.RangeNativeError, match="range_map_reserve"):
        eng.ica_step(dev(Y), W)
    eng.reserve(5000, 3)
    eng.ica_step(dev(Y), W)
    eng.close()


# ---- sources ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, SHARE - 1, SHARE + 1])
@pytest.mark.parametrize("c", [1, 2, 3, 5, 8])
def test_sources(engine, n, c):
    rng = np.random.default_rng(5 * n + c)
    Y, M = rng.standard_normal((c, n)), rng.standard_normal((c, c))
    got = engine.sources(strided(Y, 3), M, max_grid=2 if n > 512 else 0).cpu().numpy()
    want, bound = R.sources_ld(Y, M)
    assert got.shape == (n, c) and (np.abs(got.astype(L) - want) <= bound).all()


# ---- equalisation -------------------------------------------------------------------------------------------------
def equalize_case(engine, x, stride=1, nbins=256, max_grid=0):
    want, counts, edges = R.equalize(x, nbins)
    PAD = 16
    src = torch.full((PAD + len(x) * stride + PAD,), float("nan"), dtype=torch.float64, device=DEV)
    dst = torch.full_like(src, -7.0)
    src[PAD:PAD + len(x) * stride:stride] = dev(x)
    got, cnt = engine.equalize(src[PAD:PAD + len(x) * stride:stride], dev(edges),
                               out=dst[PAD:PAD + len(x) * stride:stride], max_grid=max_grid)
    assert np.array_equal(cnt.cpu().numpy(), counts) and np.array_equal(counts, np.histogram(x, bins=nbins)[0])
    full = dst.cpu().numpy()
    touched = np.zeros(len(full), dtype=bool)
    touched[PAD:PAD + len(x) * stride:stride] = True
    assert (full[~touched] == -7.0).all()
    got = got.cpu().numpy()
    err = np.abs(got - want).max()
    assert err <= 2.0 ** -50 and got.min() >= 0.0 and got.max() <= 1.0, err
    return got


@pytest.mark.parametrize("case", sorted(R.equalize_cases()))
def test_equalize_edge_cases(engine, case):
    equalize_case(engine, R.equalize_cases()[case], stride=3 if case in ("normal", "constant") else 1)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 3 * 256 + 1])
def test_equalize_rows(engine, n):
    x = np.random.default_rng(n).laplace(size=n)
    a = equalize_case(engine, x, stride=2, max_grid=3)          # (3 * 256 + 1: a second trip)
    assert np.array_equal(a, equalize_case(engine, x, stride=2))
    equalize_case(engine, x, nbins=7)
    equalize_case(engine, x, nbins=1024)


# ---- the plan's own grid cap -------------------------------------------------------------------------------------
def test_one_row_beyond_the_plans_own_grid(engine):
    """Rows found from the plan so that its own cap (not a test's max_grid) is reached and workgroup 0 makes a second
    trip: projection, sources and equalisation.  The ICA step never gets there: its slabs are capped at the grid's
    size, so its second trip exists only under max_grid (test_ica_step_is_bit_identical)."""
    p = _map_native.plan(1 << 30, 3)
    n_proj = p["proj_grid"] * p["proj_rows"] + 1
    n_eq = p["eq_grid"] * p["eq_rows"] + 1
    assert _map_native.plan(n_proj, 3)["proj_grid"] == p["proj_grid"] == _map_native.plan(n_proj - 1, 3)["proj_grid"]
    assert _map_native.plan(n_eq, 3)["eq_grid"] == p["eq_grid"] and p["slabs"] <= p["step_grid"]
    project_case(engine, n_proj, 3, 5, pad=1)
    project_case(engine, n_proj, 2, 4, pad=0)
    rng = np.random.default_rng(9)
    Y, M = rng.standard_normal((2, n_eq)), rng.standard_normal((2, 2))
    got = engine.sources(dev(Y), M).cpu().numpy()
    want, bound = R.sources_ld(Y, M)
    assert (np.abs(got.astype(L) - want) <= bound).all()
    equalize_case(engine, Y[0])


# ---- ica_colors on what scikit-learn produced ---------------------------------------------------------------------
@pytest.mark.parametrize("f,tag,c,it", RUNS)
@pytest.mark.parametrize("where", ["host_f32", "device_f64"])
def test_ica_colors_against_the_golden(golden, f, tag, c, it, where):
    X = golden[f + "_X"]
    feats = X if where == "host_f32" else dev(X.astype(np.float64))
    colors, info = ica_colors(feats, n_components=c, device=DEV, return_info=True)
    key = f"{f}_{tag}_"
    d_ref = float(golden[key + "d_ref"])
    err = np.abs(info["sources"] - golden[key + "svd"]).max()
    print(f"{f} {tag} {where}: n_iter {info['n_iter']}, sources - golden {err:.2e} = {err / d_ref:.1f} d_ref")
    assert info["n_iter"] == int(golden[key + "n_iter"]) and info["converged"]
    assert err <= 100 * d_ref
    assert np.allclose(info["limits"], golden[key + "limits"], rtol=1e-6, atol=1e-12)
    assert colors.shape == (X.shape[0], c) and colors.dtype == np.float64
    for k in range(c):
        assert np.abs(colors[:, k] - R.equalize(info["sources"][:, k])[0]).max() <= 2.0 ** -50
    assert colors.min() >= 0.0 and colors.max() <= 1.0
    assert np.abs(info["sources"].std(axis=0) - 1).max() < 1e-12 and np.abs(info["sources"].mean(axis=0)).max() < 1e-12
    Xs = R.standardise(X.astype(np.float64))[0]
    assert np.abs(np.dot(Xs, info["components_"].T) - info["sources"]).max() <= 100 * d_ref
    if f.startswith("sphere"):
        assert info["std_"][7] == 1e-8 and info["mean_"][7] == 0.25


def test_ica_colors_stopped_at_three_iterations(golden):
    X = golden["sphere_640x96_X"]
    with pytest.warns(ConvergenceWarning, match="did not converge"):
        colors, info = ica_colors(X, max_iter=3, device=DEV, return_info=True)
    assert info["n_iter"] == 3 and not info["converged"]
    assert np.abs(info["sources"] - golden["sphere_640x96_c3_it3_svd"]).max() <= 100 * float(golden["sphere_640x96_c3_it3_d_ref"])
    assert np.allclose(info["limits"], golden["sphere_640x96_c3_it3_limits"], rtol=1e-6)
    # the same call again: the same bits, also of the colours
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        again = ica_colors(X, max_iter=3, device=DEV)
    assert np.array_equal(colors, again)


def test_ica_colors_refuses_on_the_device(golden, monkeypatch):
    X = dev(golden["synth_600x50_X"].astype(np.float64)).clone()
    X[17, 4] = float("nan")
    with pytest.raises(ValueError, match=r"non-finite.*column 4"):
        ica_colors(X)
    X[17, 4] = float("inf")
    with pytest.raises(ValueError, match=r"non-finite.*column 4"):
        ica_colors(X.float())
    for bad in (np.nan, np.inf, -np.inf):               # host arrays: refused from the device's column sums too
        for dtype in (np.float64, np.float32):
            H = golden["synth_600x50_X"][:40].astype(dtype)
            H[11, 3] = bad
            with pytest.raises(ValueError, match=r"non-finite.*column 3"):
                ica_colors(H, device=DEV)
    # two float64 copies of the matrix must fit: refused before anything is allocated, both sizes named
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (100000, 1 << 40))
    with pytest.raises(ValueError, match=r"needs \d+ more bytes.*100000 bytes are free"):
        ica_colors(golden["synth_600x50_X"], device=DEV)


# ---- end to end ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(tmp_path_factory):
    from range_amd import load_model
    from tools import synth
    tmp = tmp_path_factory.mktemp("icamap_models")
    ck = synth.write_checkpoint(str(tmp / "enc.ckpt"), L=10, hidden=64, seed=5)
    db = synth.write_bank(str(tmp / "db.npz"), 700, seed=3)
    return {"Theory": load_model("Theory", pretrained_path="unused", device=DEV),
            "RANGE+": load_model("RANGE+", pretrained_path=ck, device=DEV, db_path=db, beta=0.5)}


@pytest.mark.parametrize("name", ["Theory", "RANGE+"])
def test_embedding_map_end_to_end(models, name):
    model = models[name]
    locs = coord_grid((24, 48))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)
        colors = embedding_map(model, locs)
        direct = ica_colors(model(locs, return_device=True))
        chunked = embedding_map(model, locs, batch_size=500)
    assert colors.shape == (1152, 3) and colors.dtype == np.float64
    assert np.array_equal(colors, direct)
    assert colors.min() >= 0.0 and colors.max() <= 1.0
    assert chunked.shape == (1152, 3) and np.abs(chunked - colors).max() < 1e-6


def test_command_line_tool(models, tmp_path):
    out = str(tmp_path / "map")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "embedding_map.py"), "--grid", "24", "48",
                        "--location_model_name", "Theory", "--out", out, "--device", DEV],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(out + ".npz")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)
        want = embedding_map(models["Theory"], coord_grid((24, 48)))
    assert np.array_equal(z["colors"], want) and np.array_equal(z["locs"], coord_grid((24, 48)))
    assert z["grid"].tolist() == [24, 48]
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.image as mpimg
    img = mpimg.imread(out + ".png")
    assert img.ndim == 3 and img.shape[2] in (3, 4) and img.shape[0] > 100 and img.shape[1] > 100
    h = subprocess.run([sys.executable, os.path.join(REPO, "tools", "embedding_map.py"), "--help"],
                       capture_output=True, text=True, timeout=120)
    text = " ".join(h.stdout.split())
    assert h.returncode == 0 and "no coastlines" in text and "--input_csv" in h.stdout and "--range_db" in h.stdout
