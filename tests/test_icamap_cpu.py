"""The embedding map, CPU side (no GPU): the numpy restatement the GPU tests lean on (tests/icamap_refs.py) against
the sources scikit-learn's FastICA produced (tests/golden/icamap.npz, written by make_golden_icamap.py) and against
the installed scikit-learn; ``coord_grid`` bit for bit against the reference's; the equalisation restatement against
numpy.histogram at bin edges, extremes and on a constant column; planted defects; the launch plan under the host
sanitizers; the refusals of ``ica_colors``."""
import os
import subprocess
import warnings

import numpy as np
import pytest

import icamap_refs as R
from range_amd import embedding_map as embedding_map_fn
from range_amd.embedding_map import (check_finite_sums, check_shape, coord_grid, ica_colors, sym_decorrelation,
                                     whitening)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = [("synth_600x50", "c3", 3, 1000), ("synth_601x130", "c3", 3, 1000), ("sphere_640x96", "c3", 3, 1000),
        ("sphere_640x96", "c2", 2, 1000), ("sphere_640x96", "c5", 5, 1000), ("sphere_640x96", "c3_it3", 3, 3)]
GPU_FACTOR = 100          # the GPU tests' bound on the sources: 100 * d_ref (tests/test_gpu_icamap.py)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "icamap.npz"))


@pytest.fixture(scope="module")
def restated(golden):
    """The restatement on every recorded run, once."""
    return {(f, tag): R.fastica_sources(golden[f + "_X"].astype(np.float64), c, 2001, it) for f, tag, c, it in RUNS}


def test_fixture_is_small_and_complete(golden, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "icamap.npz")) < 1024 * 1024
    for f, tag, c, it in RUNS:
        X = golden[f + "_X"]
        assert X.dtype == np.float32 and X.shape[0] >= 600 and np.isfinite(X).all()
        key = f"{f}_{tag}_"
        assert golden[key + "svd"].shape == golden[key + "eigh"].shape == (X.shape[0], c)
        assert len(golden[key + "limits"]) == int(golden[key + "n_iter"]) <= it
        assert float(golden[key + "d_ref"]) == np.abs(golden[key + "svd"] - golden[key + "eigh"]).max() > 0
        lim = golden[key + "limits"]
        assert (np.abs(lim - R.TOL) >= 0.01 * R.TOL).all() and (lim[:-1] >= R.TOL).all()
        assert (lim[-1] < R.TOL) == (it == 1000)
    sphere = golden["sphere_640x96_X"]
    assert (sphere[:, 7] == 0.25).all()                 # the constant column: the 1e-8 rule


@pytest.mark.parametrize("f,tag,c,it", RUNS)
def test_restatement_against_the_golden(golden, restated, f, tag, c, it):
    key, r = f"{f}_{tag}_", restated[f, tag]
    assert r["n_iter"] == int(golden[key + "n_iter"])
    err = np.abs(r["sources"] - golden[key + "svd"]).max()
    print(f"{f} {tag}: restatement - golden {err:.2e}, d_ref {float(golden[key + 'd_ref']):.2e}")
    assert err <= 10 * float(golden[key + "d_ref"])
    assert np.array_equal(r["limits"], golden[key + "limits"]) or np.allclose(r["limits"], golden[key + "limits"], rtol=1e-6)


@pytest.mark.parametrize("f,tag,c,it", RUNS)
def test_restatement_against_live_sklearn(golden, restated, f, tag, c, it):
    decomposition = pytest.importorskip("sklearn.decomposition")
    Xs = R.standardise(golden[f + "_X"].astype(np.float64))[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ica = decomposition.FastICA(n_components=c, random_state=2001, whiten="unit-variance", max_iter=it)
        S = ica.fit(Xs).transform(Xs)
    key = f"{f}_{tag}_"
    assert ica.n_iter_ == restated[f, tag]["n_iter"]
    assert np.abs(restated[f, tag]["sources"] - S).max() <= 10 * float(golden[key + "d_ref"])


def test_package_host_algebra_is_the_restatements(golden):
    """range_amd/embedding_map.py's own host pieces (whitening from the Gram matrix, the decorrelation) against the
    restatement: K' (x - mean) is sqrt(n) K xs."""
    X = golden["sphere_640x96_X"].astype(np.float64)
    n = X.shape[0]
    Xs, mu, sd = R.standardise(X)
    Zc = X - mu
    std, K, Kp = whitening(np.tril(np.dot(Zc.T, Zc)), n, 3)
    assert std[7] == 1e-8 and np.allclose(std, sd, rtol=1e-12)
    lam, u, _ = R.eig_top(Xs, 3)
    assert np.allclose(K, ((u * np.sign(u[0])) / np.sqrt(lam)).T, rtol=1e-9, atol=1e-12)
    assert np.allclose(np.dot(Kp, Zc.T), np.sqrt(n) * np.dot(K, Xs.T), rtol=1e-9, atol=1e-9)
    W = np.random.RandomState(2001).normal(size=(3, 3))
    assert np.array_equal(sym_decorrelation(W), R.sym_decorrelation(W))
    assert np.allclose(np.dot(sym_decorrelation(W), sym_decorrelation(W).T), np.eye(3), atol=1e-12)


def test_coord_grid_is_bitwise_the_references(golden):
    g = coord_grid((5, 7))
    assert g.dtype == np.float32 and g.shape == (35, 2) and np.array_equal(g, golden["grid_5x7"])
    assert g[0].tolist() == [-180.0, 90.0] and g[-1].tolist() == [180.0, -90.0]
    s = coord_grid((4, 6), golden["grid_split_ids"], 2)
    assert s.dtype == np.float32 and np.array_equal(s, golden["grid_4x6_split"]) and s.shape == (8, 2)
    import range_amd
    assert range_amd.coord_grid is coord_grid and range_amd.ica_colors is ica_colors
    assert range_amd.embedding_map is embedding_map_fn and callable(embedding_map_fn)


@pytest.mark.parametrize("case", sorted(R.equalize_cases()))
def test_equalize_restatement_counts_are_numpys(case):
    x = R.equalize_cases()[case]
    out, counts, edges = R.equalize(x)
    want, np_edges = np.histogram(x, bins=256)
    assert np.array_equal(edges, np_edges) and np.array_equal(counts, want) and counts.sum() == len(x)
    centres = (np_edges[:-1] + np_edges[1:]) / 2.0
    assert np.array_equal(out, np.interp(x, centres, want.cumsum() / float(len(x))))
    assert out.min() >= 0.0 and out.max() <= 1.0
    if case == "constant":
        assert counts[128] == len(x) and (out == out[0]).all()


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_a_planted_defect_moves_the_sources_beyond_the_gpu_bound(golden, defect):
    """Each defect, planted in the restatement, fails the bound the GPU tests put on ``ica_colors``."""
    f = "sphere_640x96" if defect == "sign_rule" else "synth_600x50"
    got = R.fastica_sources(golden[f + "_X"].astype(np.float64), 3, 2001, 1000, defect=defect)
    err = np.abs(got["sources"] - golden[f + "_c3_svd"]).max()
    print(f"{defect}: moves the sources by {err:.2e}")
    assert err > GPU_FACTOR * float(golden[f + "_c3_d_ref"])


def test_map_plan_under_sanitizers(tmp_path):
    """host_plan.h: map_plan - slabs that cover every row once and do not depend on the grid, capped grids,
    workspace sizes, 2^40 rows, the refusals - compiled with g++ under AddressSanitizer and
    UndefinedBehaviorSanitizer and run on the CPU."""
    exe = str(tmp_path / "map_plan")
    src = os.path.join(REPO, "tests", "native", "map_plan_sanitize.cpp")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    src, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "map_plan ok" in p.stdout, p.stdout + p.stderr


def test_plan_binding_matches_the_header():
    from range_amd import _map_native
    header = open(os.path.join(REPO, "include", "range_map.h")).read()
    import re
    assert set(re.findall(r"\b(range_map_[a-z0-9_]+)\s*\(", header)) == set(_map_native.SYMBOLS)
    lib = _map_native.load_library()
    for name in _map_native.SYMBOLS:
        assert hasattr(lib, name), name
    p = _map_native.plan(1000000, 3)
    assert (p["chunk"], p["slabs"], p["step_grid"], p["ws_bytes"]) == (1024, 977, 977, 977 * 12 * 8)
    assert _map_native.plan(3 * 1024 + 1, 3, 3)["step_grid"] == 3
    with pytest.raises(_map_native.RangeNativeError):
        _map_native.plan(0, 3)


def test_refusals():
    X = np.random.default_rng(0).standard_normal((20, 5))
    for c in (0, 9, -1, 2.5):
        with pytest.raises(ValueError, match="n_components"):
            ica_colors(X, n_components=c)
    with pytest.raises(ValueError, match="exceeds the 5 feature columns"):
        ica_colors(X, n_components=6)
    with pytest.raises(ValueError, match="at least 2 rows"):
        ica_colors(X[:1], n_components=3)
    with pytest.raises(ValueError, match="2-d"):
        ica_colors(X[0])
    with pytest.raises(ValueError, match="float32 or float64"):
        ica_colors(X.astype(np.int64))
    with pytest.raises(ValueError, match="nbins"):
        ica_colors(X, nbins=1)
    for bad in (np.nan, np.inf, -np.inf):
        for dtype in (np.float64, np.float32):
            Y = X.astype(dtype)
            Y[11, 3] = bad
            with np.errstate(invalid="ignore"):
                sums = Y.sum(axis=0, dtype=np.float64)
            with pytest.raises(ValueError, match=r"non-finite.*column 3"):
                check_finite_sums(sums)            # (ica_colors takes the sums from the device: test_gpu_icamap.py)
    Y = X.copy()
    Y[2, 1], Y[3, 1] = np.inf, -np.inf                    # (inf - inf: the sum is NaN)
    with np.errstate(invalid="ignore"):
        sums = Y.sum(axis=0)
    with pytest.raises(ValueError, match="non-finite"):
        check_finite_sums(sums)
    check_finite_sums(X.sum(axis=0))
    check_shape(2, 1, 1)
    with pytest.raises(ValueError, match="lon/lat"):
        embedding_map_fn(None, np.zeros((5, 3)))
