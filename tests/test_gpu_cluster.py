"""GPU tests of the cluster map (cluster_kernels.h, include/range_cluster.h, range_amd/cluster_map.py,
tools/cluster_map.py): the normaliser and the distances through the C ABI against long-double numpy at the wave, tile
and panel edges; the linkage on exact matrices against scipy and the numpy restatement of the rounds
(tests/cluster_refs.py, pinned to scikit-learn's partitions by tests/test_cluster_cpu.py); results bit for bit across
calls, streams and grids; ``cluster_labels`` on the fixtures scikit-learn produced (tests/golden/cluster_map.npz); the
model driver and the command-line tool end to end.  Run with ``pytest -m gpu``.

Bounds (derived in tests/cluster_refs.py, not taken from what the kernels give): normalised entries (D + 4) 2^-53
relative, squared norms (D + 3) 2^-53 relative; distances from given rows
(D + 8) 2^-53.  The partitions on the fixtures are exact (the input condition of test_cluster_cpu.py).  The heights of
``cluster_labels`` against scipy's on float64 numpy distances: each side is within (D + 8) 2^-53 of the exact distance
of its own unit rows, and those rows differ by (D + 4) 2^-53 relative per entry on each side, which moves a dot product
of two of them by at most 2 (D + 4) 2^-53 per side: (6 D + 32) 2^-53 in all."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import cluster_refs as R
from range_amd import _cluster_native
from range_amd.cluster_map import cluster_labels, cluster_map
from range_amd.embedding_map import coord_grid

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
L = np.longdouble
KS = (1, 2, 8, 17)
_kernels = open(os.path.join(REPO, "range_amd", "csrc", "probe_kernels.h")).read()
GEMM_TILE = int(re.search(r"constexpr int GEMM_TILE = (\d+);", _kernels).group(1))
GEMM_KT = int(re.search(r"constexpr int GEMM_KT = (\d+);", _kernels).group(1))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "cluster_map.npz"))


@pytest.fixture(scope="module")
def engine():
    eng = _cluster_native.ClusterEngine(DEV)
    eng.reserve(600, 1280)
    return eng


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def strided(a, pad):
    """A device copy of the 2-d host array whose rows are `pad` elements apart beyond their length (NaN between)."""
    buf = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=torch.float64, device=DEV)
    buf[:, :a.shape[1]] = dev(a)
    return buf[:, :a.shape[1]]


# ---- normalise ----------------------------------------------------------------------------------------------------
def normalize_case(engine, n, d, with_mask, pad=3, max_grid=0):
    rng = np.random.default_rng(100 * n + d + with_mask)
    X = rng.standard_normal((n, d)) * rng.uniform(0.1, 10.0, (n, 1))
    mask = None
    if with_mask:
        mask = rng.uniform(0.2, 2.0, n) * (rng.random(n) < 0.6)
        X[rng.random(X.shape) < 0.1] = 0.0                # planted zeros, in unmasked rows too
    Xd = strided(X, pad)
    out = torch.full((n, d + 2), -7.0, dtype=torch.float64, device=DEV)
    E, n2 = engine.normalize(Xd, None if mask is None else dev(mask), out=out[:, :d], max_grid=max_grid)
    E, n2 = E.cpu().numpy(), n2.cpu().numpy()
    El, n2l = R.normalize_ld(X, mask)
    err = np.abs(E.astype(L) - El)
    assert (err <= R.norm_bound(d) * np.abs(El)).all(), f"n={n} d={d}: {float((err / np.abs(El)).max() / R.U):.1f} u"
    assert (np.abs(n2.astype(L) - n2l) <= R.norm2_bound(d) * n2l).all()
    assert (out[:, d:].cpu().numpy() == -7.0).all() and np.array_equal(Xd.cpu().numpy(), X)
    if with_mask:
        fill = np.sqrt(1.0 / d)
        assert np.array_equal(E[mask == 0], np.broadcast_to((fill / np.sqrt(n2))[mask == 0][:, None], (int((mask == 0).sum()), d)))
    return E, n2


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("d", [1, 3, 16, 250, 1280])
def test_normalize(engine, n, d):
    for with_mask in (False, True):
        a = normalize_case(engine, n, d, with_mask)
        b = normalize_case(engine, n, d, with_mask, pad=0, max_grid=3)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_normalize_rows_wider_than_the_registers(engine):
    """d > 2048: the row does not stay in registers and is read a second time."""
    normalize_case(engine, 5, 2049, True)
    normalize_case(engine, 5, 2100, False, max_grid=1)


# ---- distances ----------------------------------------------------------------------------------------------------
def distance_case(engine, n, d, pad_e=0, pad_d=0, max_grid=0, twins=False):
    rng = np.random.default_rng(10 * n + d)
    X = rng.standard_normal((n, d))
    if twins:
        X[n // 2:] = X[:n - n // 2]                       # identical rows
    E = R.normalize(X)[0]
    out = torch.full((n, n + pad_d), -7.0, dtype=torch.float64, device=DEV)
    D = engine.distances(strided(E, pad_e), out=out[:, :n], max_grid=max_grid).cpu().numpy()
    assert (out[:, n:].cpu().numpy() == -7.0).all()
    assert np.array_equal(D, D.T) and np.isposinf(np.diagonal(D)).all()
    off = ~np.eye(n, dtype=bool)
    assert (D[off] >= 0).all() and not np.signbit(D[off]).any()
    with np.errstate(invalid="ignore"):                    # (inf - inf on the diagonal)
        err = np.abs(D.astype(L) - R.distances_ld(E))
    assert err[off].max() <= R.dist_bound(d), f"n={n} d={d}: {float(err[off].max() / R.U):.1f} u against {d + 8}"
    return D


@pytest.mark.parametrize("n", [GEMM_TILE - 1, GEMM_TILE, GEMM_TILE + 1])
@pytest.mark.parametrize("d", [GEMM_KT - 1, GEMM_KT, GEMM_KT + 1])
def test_distances_at_tile_and_panel_edges(engine, n, d):
    a = distance_case(engine, n, d)
    assert np.array_equal(a, distance_case(engine, n, d, pad_e=3, pad_d=5, max_grid=3))
    assert np.array_equal(a, distance_case(engine, n, d, max_grid=1))
    with torch.cuda.stream(torch.cuda.Stream(DEV)):
        b = distance_case(engine, n, d)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("n,d", [(2, 3), (65, 1), (300, 250), (65, 1280), (257, 1280)])
def test_distances_shapes(engine, n, d):
    """d = 1280 at few tiles: the GEMM splits K into slabs (reserved by the engine fixture)."""
    distance_case(engine, n, d, pad_d=1)


@pytest.mark.parametrize("d", [3, 16, 250])
def test_distances_of_identical_rows_are_not_negative(engine, d):
    n = 130
    D = distance_case(engine, n, d, twins=True)
    twin = D[np.arange(n - n // 2), np.arange(n - n // 2) + n // 2]
    assert (twin >= 0).all() and (twin <= R.dist_bound(d)).all()


# ---- linkage on given matrices ------------------------------------------------------------------------------------
def linkage_case(engine, D, pad=0, max_grid=0):
    n = D.shape[0]
    buf = strided(D, pad) if pad else dev(D)
    merges, heights, rounds = engine.linkage(buf, max_grid=max_grid)
    return merges.cpu().numpy(), heights.cpu().numpy(), rounds


def identical_everywhere(engine, D, first):
    """A second call, another stream and capped grids give the first call's bits."""
    for max_grid in (0, 1, 3):
        again = linkage_case(engine, D, max_grid=max_grid)
        assert all(np.array_equal(a, b) for a, b in zip(first, again)), max_grid
    with torch.cuda.stream(torch.cuda.Stream(DEV)):
        again = linkage_case(engine, D, pad=2)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 255, 256, 257, 600])
def test_linkage_of_distinct_integers(engine, n):
    D = R.permutation_matrix(n)
    got = linkage_case(engine, D, pad=3 if n == 65 else 0)
    want = R.linkage_rounds(D)
    order, worder = np.argsort(got[1], kind="stable"), np.argsort(want["heights"], kind="stable")
    assert np.array_equal(got[0][order], want["merges"][worder])
    assert np.array_equal(got[1][order], R.scipy_heights(D))                            # bit for bit
    assert np.array_equal(got[0], want["merges"]) and got[2] == want["rounds"] <= n - 1  # the same scheme, round by round
    assert R.replay(D, got[0], got[1]) == 0.0
    identical_everywhere(engine, D, got)


def test_linkage_takes_the_loop_to_its_bound(engine):
    """Points 2^0 .. 2^39 on a line: one pair merges a round."""
    D = R.line_matrix(40)
    got = linkage_case(engine, D)
    assert got[2] == 39 and np.array_equal(got[0], np.stack([np.zeros(39), np.arange(1, 40)], axis=1))
    assert np.array_equal(got[1], R.scipy_heights(D)) and np.array_equal(got[1], R.linkage_rounds(D)["heights"])
    labels, Z = _cluster_native.cut(got[0], got[1], 5)
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import squareform
    want = linkage(squareform(D, checks=False), "complete")
    assert np.array_equal(Z, want) and np.array_equal(labels, R.first_occurrence(fcluster(want, 5, "maxclust")))
    identical_everywhere(engine, D, got)


@pytest.mark.parametrize("n", [64, 257])
def test_linkage_with_ties_passes_the_replay(engine, n):
    D = R.tie_matrix(n)
    got = linkage_case(engine, D)
    assert R.replay(D, got[0], got[1]) == 0.0 and 1 <= got[2] <= n - 1
    labels, Z = _cluster_native.cut(got[0], got[1], 7)
    from scipy.cluster.hierarchy import is_valid_linkage
    assert is_valid_linkage(Z) and len(np.unique(labels)) == 7
    identical_everywhere(engine, D, got)


def test_linkage_needs_its_workspace_and_a_symmetric_matrix(engine):
    eng = _cluster_native.ClusterEngine(DEV)
    D = R.permutation_matrix(50)
    with pytest.raises(_cluster_native.RangeNativeError, match="range_cluster_reserve"):
        eng.linkage(dev(D))
    eng.reserve(50, 4)
    eng.linkage(dev(D))
    eng.close()
    with pytest.raises(ValueError, match="square"):
        engine.linkage(dev(D[:, :40]))
    # not symmetric, nearest neighbours in a cycle 0 -> 1 -> 2 -> 3 -> 4 -> 0: a round without a reciprocal pair is
    # an error of the call, and the loop ends
    A = np.array([[0, 1, 9, 9, 2], [2, 0, 1, 9, 9], [9, 2, 0, 1, 9], [9, 9, 2, 0, 1], [1, 9, 9, 2, 0.0]])
    with pytest.raises(_cluster_native.RangeNativeError, match="error -5.*reciprocal pairs"):
        engine.linkage(dev(A))


# ---- cluster_labels on what scikit-learn produced -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["rand", "grid", "masked"])
@pytest.mark.parametrize("where", ["host_f32", "device_f64"])
def test_cluster_labels_against_the_golden(golden, name, where):
    from scipy.cluster.hierarchy import fcluster, is_valid_linkage
    X = golden[name + "_X"]
    mask = golden[name + "_mask"] if name == "masked" else None
    n = len(X)
    feats = X if where == "host_f32" else dev(X.astype(np.float64))
    for k in KS + (n,):
        if mask is not None and k == n:
            with pytest.raises(ValueError, match="distinct rows"):
                cluster_labels(feats, k, mask=mask, device=DEV)
            continue
        labels, info = cluster_labels(feats, k, mask=mask, device=DEV, return_info=True)
        assert labels.shape == (n,) and labels.dtype == np.int32
        assert np.array_equal(labels, golden[f"{name}_k{k}"]), k
        Z, m = info["linkage"], info["n_clustered"]
        assert m == (n if mask is None else int((mask == 1).sum()) + 1) and Z.shape == (m - 1, 4)
        assert is_valid_linkage(Z) and 1 <= info["rounds"] <= m - 1
        if 1 < k < m:
            sub = labels[info["rows"]]
            assert np.array_equal(R.first_occurrence(fcluster(Z, k, "maxclust")), sub)
        err = np.abs(info["heights"] - golden[name + "_heights"]).max()
        assert err <= (6 * 16 + 32) * R.U, err / R.U
    if where == "device_f64":
        assert np.array_equal(feats.cpu().numpy(), X.astype(np.float64))       # the caller's tensor is not normalised in place
        assert np.array_equal(cluster_labels(feats.float(), 8, mask=mask), golden[f"{name}_k8"])
    else:
        a = cluster_labels(X, 17, mask=mask, device=DEV, return_info=True)
        b = cluster_labels(X.astype(np.float64), 17, mask=mask, device=DEV, return_info=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1]["linkage"], b[1]["linkage"])


def test_cluster_labels_refuses_on_the_device(golden, monkeypatch):
    X = golden["rand_X"].astype(np.float64)
    for bad in (np.nan, np.inf, -np.inf):
        for dtype in (np.float64, np.float32):
            H = X[:40].astype(dtype)
            H[11, 3] = bad
            with pytest.raises(ValueError, match=r"non-finite.*column 3"):
                cluster_labels(H, 2, device=DEV)
    Z = dev(X[:50]).clone()
    Z[7] = 0.0
    Z[30] = 0.0
    with pytest.raises(ValueError, match=r"row 7 has zero norm"):
        cluster_labels(Z, 2)
    T = X[:50].copy()
    T[9] = 1e-200                                          # squares underflow: no direction left
    with pytest.raises(ValueError, match=r"row 9 has zero norm"):
        cluster_labels(T, 2, device=DEV)
    mask = np.ones(50)
    mask[7] = mask[30] = 0.0
    assert cluster_labels(Z, 3, mask=mask).shape == (50,)   # with a mask the zero rows are filled
    with pytest.raises(RuntimeError, match="GPU device"):
        cluster_labels(X, 2, device="cpu")
    # the distance matrix must fit: refused before anything is allocated, the bytes named
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (100000, 1 << 40))
    with pytest.raises(ValueError, match=r"needs \d+ more bytes.*distance matrix is 720000\).*100000 bytes are free"):
        cluster_labels(X, 2, device=DEV)


# ---- end to end ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(tmp_path_factory):
    from range_amd import load_model
    from tools import synth
    tmp = tmp_path_factory.mktemp("cluster_models")
    ck = synth.write_checkpoint(str(tmp / "enc.ckpt"), L=10, hidden=64, seed=5)
    db = synth.write_bank(str(tmp / "db.npz"), 700, seed=3)
    return {"Theory": load_model("Theory", pretrained_path="unused", device=DEV),
            "RANGE+": load_model("RANGE+", pretrained_path=ck, device=DEV, db_path=db, beta=0.5)}


@pytest.mark.parametrize("name", ["Theory", "RANGE+"])
def test_cluster_map_end_to_end(models, engine, name):
    model = models[name]
    locs = coord_grid((12, 20))
    labels, info = cluster_map(model, locs, 6, grid_size=(12, 20), return_info=True)
    assert labels.shape == (12, 20) and labels.dtype == np.int32 and len(np.unique(labels)) == 6
    assert labels[0, 0] == 0 and np.array_equal(labels.reshape(-1), R.first_occurrence(labels))
    flat = cluster_map(model, locs, 6)
    assert flat.shape == (240,) and np.array_equal(flat, labels.reshape(-1))
    # the replay property on the model's own embeddings and the device's own distances of them (where an encoder is
    # periodic in longitude the +-180 degree columns coincide: ties are real here)
    feats = model(locs, return_device=True).to(torch.float64)
    d = feats.shape[1]
    E, _ = engine.normalize(feats)
    engine.reserve(240, d)
    D = engine.distances(E)
    D_host = D.cpu().numpy()
    merges, heights, rounds = engine.linkage(D)
    merges, heights = merges.cpu().numpy(), heights.cpu().numpy()
    assert R.replay(D_host, merges, heights) <= 2 * R.dist_bound(d)
    assert np.array_equal(_cluster_native.cut(merges, heights, 6)[0], flat) and rounds == info["rounds"]
    # a land mask: the masked cells share one label
    mask = (np.arange(240).reshape(12, 20) % 5 != 0).astype(np.float64)
    masked = cluster_map(model, locs, 4, grid_size=(12, 20), mask=mask)
    assert masked.shape == (12, 20) and len(np.unique(masked[mask == 0])) == 1 and len(np.unique(masked)) == 4


def test_command_line_tool(models, tmp_path):
    out = str(tmp_path / "clusters")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "cluster_map.py"), "--grid", "12", "20",
                        "--location_model_name", "Theory", "--n_clusters", "6", "--out", out, "--device", DEV],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(out + ".npz")
    want = cluster_map(models["Theory"], coord_grid((12, 20)), 6, grid_size=(12, 20))
    assert np.array_equal(z["labels"], want) and np.array_equal(z["locs"], coord_grid((12, 20)))
    assert z["grid"].tolist() == [12, 20] and int(z["n_clusters"]) == 6 and z["linkage"].shape == (239, 4)
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.image as mpimg
    img = mpimg.imread(out + ".png")
    assert img.ndim == 3 and img.shape[2] in (3, 4) and img.shape[0] > 100 and img.shape[1] > 100
    h = subprocess.run([sys.executable, os.path.join(REPO, "tools", "cluster_map.py"), "--help"],
                       capture_output=True, text=True, timeout=120)
    text = " ".join(h.stdout.split())
    assert h.returncode == 0 and "no coastlines" in text and "--input_csv" in h.stdout and "--n_clusters" in h.stdout
