"""The cluster map, CPU side (no GPU): the numpy restatement of the linkage rounds the GPU tests lean on
(tests/cluster_refs.py) against the partitions scikit-learn and the heights scipy produced
(tests/golden/cluster_map.npz, written by make_golden_cluster.py); the input condition that makes those partitions
exact; float64 numpy under the normaliser's and the distances' bounds; the replay property; planted defects; the launch
plan and the cut under the host sanitizers; the binding against the header; the refusals of ``cluster_labels`` that
need no device."""
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_refs as R
from range_amd import _cluster_native
from range_amd.cluster_map import check_shape, cluster_labels, cluster_map, rows_to_cluster

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("rand", "grid", "masked")
KS = (1, 2, 8, 17)
L = np.longdouble


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "cluster_map.npz"))


def case_inputs(golden, name):
    """(X float64, mask or None, the rows that get clustered, position of the masked representative among them)"""
    X = golden[name + "_X"].astype(np.float64)
    mask = golden[name + "_mask"] if name + "_mask" in golden.files else None
    idx, rep = rows_to_cluster(mask, len(X))
    return X, mask, idx, rep


@pytest.fixture(scope="module")
def restated(golden):
    """Per case, once: the float64 numpy distances of the clustered rows and the restatement's rounds on them."""
    out = {}
    for name in CASES:
        X, mask, idx, rep = case_inputs(golden, name)
        D = R.distances(R.normalize(X, mask)[0][idx])
        out[name] = (D, R.linkage_rounds(D), idx, rep)
    return out


def expand(labels, idx, rep, n):
    full = np.full(n, labels[rep] if rep is not None else -1, dtype=np.int32)
    full[idx] = labels
    return full


def test_fixture_is_small_and_complete(golden, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "cluster_map.npz")) < 1024 * 1024
    assert len(golden["versions"]) == 3 and any(v.startswith("scikit-learn") for v in golden["versions"])
    assert golden["rand_X"].shape == (300, 16) and golden["grid_X"].shape == golden["masked_X"].shape == (312, 16)
    for name in CASES:
        X, mask, idx, rep = case_inputs(golden, name)
        assert golden[name + "_X"].dtype == np.float32 and np.isfinite(X).all()
        assert golden[name + "_heights"].shape == (len(idx) - 1,)
        for k in KS + (len(X),):
            lab = golden[f"{name}_k{k}"]
            assert lab.shape == (len(X),) and len(np.unique(lab)) == k and np.array_equal(lab, R.first_occurrence(lab))
    mask = golden["masked_mask"]
    assert 0.55 <= (mask == 0).mean() <= 0.65 and set(np.unique(mask)) == {0.0, 1.0}
    assert (golden["masked_X"][mask == 1] == 0).sum() == 3                 # the planted zeros in unmasked rows
    assert len(np.unique(golden["grid_X"], axis=0)) == 312                 # no two rows coincide


@pytest.mark.parametrize("name", CASES)
def test_the_input_condition_that_makes_the_partitions_exact(golden, restated, name):
    """The smallest gap between two distinct entries of the reference distance matrix exceeds twice the distance
    bound: every computation of the distances within the bound orders them alike.  A condition on the input."""
    D = restated[name][0]
    gap = R.smallest_gap(D)
    print(f"{name}: smallest gap {gap:.2e}, bound {R.dist_bound(16):.2e}")
    assert gap == float(golden[name + "_gap"]) and gap > 2 * R.dist_bound(16)
    il = np.tril_indices(len(D), -1)
    assert len(np.unique(D[il])) == len(il[0])                             # no ties at all among the clustered rows


@pytest.mark.parametrize("name", CASES)
def test_restatement_against_the_golden(golden, restated, name):
    D, r, idx, rep = restated[name]
    n = len(golden[name + "_X"])
    assert np.array_equal(np.sort(r["heights"]), golden[name + "_heights"])            # bit for bit scipy's
    assert 1 <= r["rounds"] <= len(idx) - 1 and r["scans"] >= len(idx)
    print(f"{name}: {len(idx)} rows, {r['rounds']} rounds, {r['scans'] / len(idx):.2f} row scans a row")
    for k in KS + (len(idx),):
        lab, Z = _cluster_native.cut(r["merges"], r["heights"], k)
        lab_py, Z_py = R.cut(r["merges"], r["heights"], k)
        assert np.array_equal(lab, lab_py) and np.array_equal(Z, Z_py) and lab.dtype == np.int32
        if k <= 17 or rep is None:
            # (clustering the distinct rows and one representative is clustering all rows)
            assert np.array_equal(expand(lab, idx, rep, n), golden[f"{name}_k{k if k <= 17 else n}"])
    assert R.replay(D, r["merges"], r["heights"]) == 0.0


@pytest.mark.parametrize("name", CASES)
def test_linkage_matrix_is_scipys(golden, restated, name):
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    D, r, idx, rep = restated[name]
    Z = _cluster_native.cut(r["merges"], r["heights"], 1)[1]
    assert hierarchy.is_valid_linkage(Z) and np.array_equal(Z[:, 2], golden[name + "_heights"])
    M = D.copy()
    np.fill_diagonal(M, 0.0)
    from scipy.spatial.distance import squareform
    want = hierarchy.linkage(squareform(M, checks=False), "complete")
    assert np.array_equal(Z, want)                       # (no ties: the tree and scipy's numbering of it are unique)
    for k in (2, 8, 17):
        lab = _cluster_native.cut(r["merges"], r["heights"], k)[0]
        assert np.array_equal(R.first_occurrence(hierarchy.fcluster(Z, k, "maxclust")), lab)


def test_restatement_against_live_sklearn(golden):
    cluster = pytest.importorskip("sklearn.cluster")
    X = golden["rand_X"].astype(np.float64)[:120]
    E = R.normalize(X)[0]
    r = R.linkage_rounds(R.distances(E))
    for k in (2, 5, 11):
        want = cluster.AgglomerativeClustering(n_clusters=k, metric="cosine", linkage="complete").fit(E).labels_
        assert np.array_equal(_cluster_native.cut(r["merges"], r["heights"], k)[0], R.first_occurrence(want))


@pytest.mark.parametrize("d", [1, 3, 16, 250, 1280])
def test_float64_numpy_passes_both_bounds(d):
    rng = np.random.default_rng(d)
    X = rng.standard_normal((65, d)) * rng.uniform(0.1, 10.0, (65, 1))
    mask = rng.uniform(0.2, 2.0, 65) * (rng.random(65) < 0.6)
    X[rng.random(X.shape) < 0.05] = 0.0
    for m in (None, mask):
        if m is None:
            X = X.copy()
            X[~X.any(axis=1), 0] = 1.0                   # (without a mask nothing is filled: no zero rows)
        E, n2 = R.normalize(X, m)
        El, n2l = R.normalize_ld(X, m)
        assert (np.abs(E.astype(L) - El) <= norm_slack(El, d)).all()
        assert (np.abs(n2.astype(L) - n2l) <= R.norm2_bound(d) * n2l).all()
        with np.errstate(invalid="ignore"):              # (inf - inf on the diagonal)
            err = np.abs(R.distances(E).astype(L) - R.distances_ld(E))
        np.fill_diagonal(err, 0)
        assert err.max() <= R.dist_bound(d), float(err.max() / R.dist_bound(d))
    if d == 1:
        assert set(np.unique(np.abs(R.normalize(X + 0.5)[0]))) == {1.0}


def norm_slack(El, d):
    return R.norm_bound(d) * np.abs(El)


def test_masked_rows_and_zero_fill_follow_the_definition(golden):
    X, mask, idx, rep = case_inputs(golden, "masked")
    Y = R.masked_features(X, mask)
    fill = np.sqrt(1.0 / 16)
    assert (Y[mask == 0] == fill).all() and (Y[mask == 1] == 0).sum() == 0 and (Y == fill).sum() == 16 * (mask == 0).sum() + 3
    assert np.array_equal(R.masked_features(X, None), X)                   # without a mask nothing is filled
    assert len(idx) == (mask == 1).sum() + 1 and idx[rep] == np.flatnonzero(mask == 0)[0]
    assert rows_to_cluster(None, 5)[1] is None and rows_to_cluster(np.ones(5), 5)[1] is None


@pytest.mark.parametrize("kind", ["perm", "line", "ties"])
def test_replay_on_exact_matrices(kind):
    D = {"perm": R.permutation_matrix(65), "line": R.line_matrix(40), "ties": R.tie_matrix(64)}[kind]
    r = R.linkage_rounds(D)
    assert R.replay(D, r["merges"], r["heights"]) == 0.0
    if kind != "ties":
        assert np.array_equal(np.sort(r["heights"]), R.scipy_heights(D))
    if kind == "line":
        assert r["rounds"] == 39                        # one pair a round: the loop at its bound


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_a_planted_defect_is_caught(golden, restated, defect):
    """Each defect, planted in the restatement, changes a fixture partition or fails the replay."""
    caught = []
    for name in ("rand", "grid"):
        D, good, idx, rep = restated[name]
        try:
            r = good if defect == "emission_order" else R.linkage_rounds(D, defect=defect)
            parts_differ = any(not np.array_equal(R.cut(r["merges"], r["heights"], k, defect == "emission_order")[0],
                                                  golden[f"{name}_k{k}"]) for k in (2, 8, 17))
            replay_fails = False
            if defect != "emission_order":
                try:
                    replay_fails = R.replay(D, r["merges"], r["heights"]) > 0.0
                except AssertionError:
                    replay_fails = True
        except AssertionError:
            parts_differ = replay_fails = True
        print(f"{defect} on {name}: partition differs {parts_differ}, replay fails {replay_fails}")
        caught.append(parts_differ or replay_fails)
    assert all(caught)


def test_cluster_plan_under_sanitizers(tmp_path):
    """host_plan.h: cluster_plan and cluster_cut - walks that cover every row, tile and item once under any grid cap,
    a workspace without overlaps, 2^17 rows without overflow, the refusals; the cut on hand-made merge lists -
    compiled with g++ under AddressSanitizer and UndefinedBehaviorSanitizer and run on the CPU."""
    exe = str(tmp_path / "cluster_plan")
    src = os.path.join(REPO, "tests", "native", "cluster_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    src, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "cluster_plan ok" in p.stdout, p.stdout + p.stderr


def test_binding_matches_the_header():
    header = open(os.path.join(REPO, "include", "range_cluster.h")).read()
    assert set(re.findall(r"\b(range_cluster_[a-z0-9_]+)\s*\(", header)) == set(_cluster_native.SYMBOLS)
    assert int(re.search(r"#define RANGE_CLUSTER_MAX_ROWS (\d+)", header).group(1)) == _cluster_native.MAX_ROWS
    lib = _cluster_native.load_library()
    for name in _cluster_native.SYMBOLS:
        assert hasattr(lib, name), name
    p = _cluster_native.plan(64800, 256)
    assert p["matrix_bytes"] == 64800 * 64800 * 8 and p["chunks"] == 64 and p["fin_items"] == 1013 * 1014 // 2
    assert _cluster_native.plan(64800, 256, 3)["scan_grid"] == 3 and _cluster_native.plan(64800, 256, 3)["ws_bytes"] == p["ws_bytes"]
    for bad in ((0, 16), (_cluster_native.MAX_ROWS + 1, 16), (10, 0)):
        with pytest.raises(_cluster_native.RangeNativeError):
            _cluster_native.plan(*bad)
    with pytest.raises(_cluster_native.RangeNativeError, match="bad cut"):
        _cluster_native.cut([[0, 1], [0, 1]], [1.0, 2.0], 2)
    import range_amd
    assert range_amd.cluster_labels is cluster_labels and range_amd.cluster_map is cluster_map
    assert {"cluster_labels", "cluster_map"} <= set(range_amd.__all__)


def test_refusals():
    X = np.random.default_rng(0).standard_normal((20, 5))
    with pytest.raises(ValueError, match="at least 2 rows"):
        cluster_labels(X[:1], 1)
    for k in (0, 21, -1, 2.5, True):
        with pytest.raises(ValueError, match=r"n_clusters must be an integer in 1\.\.20"):
            cluster_labels(X, k)
    with pytest.raises(ValueError, match="2-d"):
        cluster_labels(X[0], 2)
    with pytest.raises(ValueError, match="float32 or float64"):
        cluster_labels(X.astype(np.int64), 2)
    with pytest.raises(ValueError, match="float32 or float64"):
        cluster_labels(X.astype(np.float16), 2)
    with pytest.raises(ValueError, match="one value a row"):
        cluster_labels(X, 2, mask=np.ones(19))
    with pytest.raises(ValueError, match="non-finite"):
        cluster_labels(X, 2, mask=np.full(20, np.nan))
    mask = np.zeros(20)
    mask[:4] = 1
    with pytest.raises(ValueError, match=r"n_clusters=6 exceeds the 5 distinct rows"):
        cluster_labels(X, 6, mask=mask)
    with pytest.raises(RuntimeError, match="GPU device"):
        cluster_labels(X, 2, device="cpu")
    check_shape(2, 1, 1)
    check_shape(2, 1, np.int64(2))
    with pytest.raises(ValueError, match="lon/lat"):
        cluster_map(None, np.zeros((5, 3)), 2)
    with pytest.raises(ValueError, match="does not hold the 6 locations"):
        cluster_map(None, np.zeros((6, 2)), 2, grid_size=(2, 4))
