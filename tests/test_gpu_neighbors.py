"""GPU tests of the neighbour and grid geo priors (neighbor_kernel.h, include/range_neighbors.h,
range_amd/geo_baselines.py, csp_eval.compute_acc_batch's baseline branches): through the C ABI and through Python,
against the numpy restatement (tests/neighbor_refs.py, pinned bit for bit to the reference's own functions by
tests/test_neighbors_cpu.py) and against the fixture itself.  Votes, priors and the three rank integers are EXACT;
random sweeps first compute every query's gap to its threshold on the restatement and leave out queries nearer than
2^-40 (relative) - at most 1 % of a case, none with the seeds used (asserted on the CPU).  Run with ``pytest -m gpu``."""
import logging
import os

import numpy as np
import pytest
import torch

import neighbor_refs as R
from range_amd import _neighbors_native as nn
from range_amd import csp_eval
from range_amd import geo_baselines as gb

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "neighbor_priors.npz")
DEV = "cuda:0"
ULP = 2.0 ** -52
SENT, PAD = -777, 64


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def dev(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))
    return torch.from_numpy(a).to(DEV)


def engine_for(s_deg, classes, C, hav, cells=None):
    eng = nn.NeighborEngine(DEV)
    eng.set_neighbors(R.metric_locs(s_deg, hav), classes, C, hav, cells=cells)
    return eng


def images(B, C, seed, dtype=np.float32):
    rng = np.random.default_rng(seed)
    img = rng.random((B, C)).astype(dtype)
    img[rng.random((B, C)) < 0.1] = 0.0            # exact zeros: ties among the scores
    return img


def assert_ranks(got, prior, img, labels):
    want = R.ranks(prior, img, labels)
    for g, w, name in zip(got, want, ("greater", "tied_after", "argmax")):
        assert np.array_equal(g, w), name


def asin_amplification(a):
    """d = 2 asin(sqrt(a)): the relative error of d per relative error of a, (a / d) dd/da."""
    r = np.sqrt(a)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = r / (2 * np.arcsin(r) * np.sqrt(1 - a))
    return np.where(a > 0, f, 0.5)


# The device's sin and cos are within 4 ulp of the exact values (the OpenCL bound the device library documents),
# numpy's within 1: every factor of a = s0 s0 + c1 c2 s1 s1 differs by at most 5 ulp relatively, a product of four
# by 20 plus 3 roundings, and the sum of two non-negative terms keeps the larger relative error plus one rounding:
# 24 ulp; 32 taken.  The euclidean d2 has no library call: exact.
RED_REL_BOUND = 32 * ULP


@pytest.mark.parametrize("case", [f"{m}_C{c}" for m in ("haversine", "euclidean") for c in (1, 5, 33)])
def test_fixture_priors_bit_for_bit(golden, case):
    hav, C = case.startswith("haversine"), int(case.split("_C")[1])
    s, q, classes = golden[case + "_s"], golden[case + "_q"], golden[case + "_classes"]
    hp = dict(dist_type="haversine" if hav else "euclidean", dist_thresh=float(golden[case + "_dist_thresh"]))
    p = gb.NeighborPrior(s, classes, C, hp, device=DEV)
    assert np.array_equal(p.prior(q, "distance"), golden[case + "_prior_distance"])
    for k in (int(k) for k in golden[case + "_ks"]):
        p.num_neighbors = k
        assert np.array_equal(p.prior(q, "knn"), golden[f"{case}_prior_knn{k}"])
        # the k-th distance BallTree.query recorded: sqrt / asin run on the host (numpy, 1 ulp each), the bound is
        # RED_REL_BOUND through d(a) - half of it for the square root, asin_amplification for the haversine - plus 4 ulp
        got, want = p.kth_distance(q, k), golden[f"{case}_kth{k}"]
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).sum() == 1
        ok = ~np.isnan(want)
        red = (np.sin(want[ok] / 2) ** 2) if hav else want[ok] ** 2
        bound = (RED_REL_BOUND * np.maximum(0.5, asin_amplification(red) if hav else 0.5) + 4 * ULP) * np.abs(want[ok])
        err = np.abs(got[ok] - want[ok])
        print(f"{case} k={k}: kth distance uses {np.max(err / np.maximum(bound, 1e-300)):.3f} of its bound")
        assert (err <= bound).all()
    with pytest.raises(ValueError, match="num_neighbors"):
        p.num_neighbors = len(s) + 1
        p.prior(q, "knn")


@pytest.mark.parametrize("case", ["grid_pc2", "grid_pc3", "grid_pc1", "grid_pchalf"])
def test_grid_fixture_bit_for_bit(golden, case):
    s, q, classes, want = golden[case + "_s"], golden[case + "_q"], golden[case + "_classes"], golden[case + "_prior"]
    pc = float(golden[case + "_pseudo_count"])
    hp = dict(gp_size=[int(v) for v in golden[case + "_gp_size"]], pseudo_count=int(pc) if pc == int(pc) else pc)
    p = gb.GridPrior(s, classes, want.shape[1], hp, device=DEV)
    assert np.array_equal(p.eval(q), want, equal_nan=True)
    assert np.array_equal(p.eval(q[7]), want[7], equal_nan=True) and p.eval(q[7]).shape == (want.shape[1],)
    with pytest.raises(ValueError, match="row 1"):
        p.eval(np.array([[0.0, 0.0], [180.0, 0.0]]))


@pytest.mark.parametrize("C", [1, 5, 33, 8142])
@pytest.mark.parametrize("hav", [True, False], ids=["haversine", "euclidean"])
def test_sweep_through_the_c_abi(hav, C):
    """N in {1, 255, 256, 257, 1000} x B in {1, G - 1, G, G + 1, 3 G + 1} x radius and k in {1, 2, 64, N}: votes, priors
    and the three integers against the restatement, exactly."""
    G = nn.plan(1, 1, C)["group"]
    assert G == {1: 8, 5: 8, 33: 8, 8142: 4}[C] and 3 * G + 1 <= R.SWEEP_B
    thresh = R.SWEEP_THRESH[hav]
    for seed, N in R.SWEEP_SEEDS:
        s, q = R.sweep_points(seed, N)
        rng = np.random.default_rng(seed + C)
        classes = rng.integers(0, C, N)
        labels = rng.integers(0, C, R.SWEEP_B)
        img = images(R.SWEEP_B, C, seed)
        eng = engine_for(s, classes, C, hav)
        assert eng.neighbor_points == N and eng.neighbor_classes == C
        qd, labd, imgd = dev(R.metric_locs(q, hav)), dev(labels, np.int32), dev(img)
        red = R.red_matrix(R.metric_locs(q, hav), R.metric_locs(s, hav), hav)
        preds = [("distance", None)] + [("knn", k) for k in R.SWEEP_KS + (N,) if k <= N]
        for ptype, k in preds:
            gap = R.threshold_gap(red, gb.radius_threshold(thresh, hav)) if ptype == "distance" else R.knn_gap(red, k)
            keep = gap >= R.GAP_SWEEP
            assert (~keep).sum() <= 0.01 * len(keep)
            cnt, _, _ = R.neighbor_counts(q, s, classes, C, hav, ptype, dist_thresh=thresh, k=k)
            prior = R.prior_neighbors(cnt)
            kw = dict(mode=nn.RADIUS, thr=gb.radius_threshold(thresh, hav)) if ptype == "distance" else dict(mode=nn.KNN, k=k)
            for B in sorted({1, G - 1, G, G + 1, 3 * G + 1} - {0}):
                rows = np.flatnonzero(keep[:B])
                got_p, got_c = eng.neighbor_prior(qd[:B], None, want_counts=True, **kw)
                assert np.array_equal(got_c.cpu().numpy()[rows], cnt[:B][rows]), (N, B, ptype, k)
                assert np.array_equal(got_p.cpu().numpy()[rows], prior[:B][rows]), (N, B, ptype, k)
                got = eng.neighbor_rank(qd[:B], None, labels=labd[:B], img=imgd[:B].contiguous(), **kw)
                assert_ranks([g.cpu().numpy()[rows] for g in got], prior[:B][rows], img[:B][rows], labels[:B][rows])
        eng.close()


def test_selection_against_the_restatement():
    for hav in (True, False):
        for seed, N in R.SWEEP_SEEDS:
            s, q = R.sweep_points(seed, N)
            q[2] = (np.nan, 1.0)
            eng = engine_for(s, np.zeros(N, dtype=np.int64), 1, hav)
            qm = R.metric_locs(q, hav)
            red = R.red_matrix(qm, R.metric_locs(s, hav), hav)
            for k in [k for k in R.SWEEP_KS + (N,) if k <= N]:
                want_r, want_j = R.select_kth(red, k)
                for max_grid in (0, 3):
                    got_r, got_j = (t.cpu().numpy() for t in eng.neighbor_select(dev(qm), k, max_grid=max_grid))
                    keep = R.knn_gap(red, k) >= R.GAP_SWEEP
                    assert keep.all()
                    assert np.array_equal(got_j, want_j), (hav, N, k)
                    assert np.isnan(got_r[2]) and got_j[2] == -1
                    ok = ~np.isnan(want_r)
                    if hav:
                        assert (np.abs(got_r[ok] - want_r[ok]) <= RED_REL_BOUND * np.abs(want_r[ok])).all()
                    else:
                        assert np.array_equal(got_r[ok], want_r[ok])
            with pytest.raises(nn.RangeNativeError, match="neighbours of"):
                eng.neighbor_select(dev(qm), N + 1)
            with pytest.raises(nn.RangeNativeError, match="neighbours of"):
                eng.neighbor_select(dev(qm), 0)
            eng.close()


def abi_rank(eng, q, qcell, mode, labels, img, kind, stream=None, max_grid=0, chunks=0, **kw):
    """range_neighbor_rank_grid through ctypes, the outputs between sentinels that must come back untouched."""
    B = labels.shape[0]
    bufs = [torch.full((PAD + B + PAD,), SENT, dtype=torch.int32, device=DEV) for _ in range(3)]
    torch.cuda.synchronize()
    st = stream if stream is not None else torch.cuda.current_stream(eng.device)
    rc = eng.lib.range_neighbor_rank_grid(eng._h, None if q is None else q.data_ptr(), None if qcell is None else qcell.data_ptr(),
                                          B, mode, kw.get("k", 0), kw.get("thr", 0.0), kw.get("pc", 0.0), kw.get("cpc", 0.0),
                                          None if img is None else img.data_ptr(), kind, labels.data_ptr(),
                                          *(b[PAD:].data_ptr() for b in bufs), max_grid, chunks, st.cuda_stream)
    assert rc == 0, eng.lib.range_last_error().decode()
    st.synchronize()
    out = []
    for b in bufs:
        h = b.cpu().numpy()
        assert (h[:PAD] == SENT).all() and (h[PAD + B:] == SENT).all()
        out.append(h[PAD:PAD + B])
    return out


def test_duplicates_flags_and_image_kinds():
    hav, C, N = True, 5, 300
    s = R.random_locs(N, 31)
    s[[40, 41, 150, 299]] = s[7]                   # an exact duplicate group: 7, 40, 41, 150, 299
    classes = np.arange(N) % C
    q = R.queries_near(s, 9, 32)
    q[0] = s[7]                                    # red = 0 to all five: k = 3 cuts the group after index 41
    q[4] = (np.nan, 3.0)
    q[5] = (np.inf, 3.0)
    q[6] = (10.0, -np.inf)
    eng = engine_for(s, classes, C, hav)
    qd = dev(R.metric_locs(q, hav))
    group = [7, 40, 41, 150, 299]
    for k in (1, 3, 5, 6):
        cnt, m, red = R.neighbor_counts(q, s, classes, C, hav, "knn", k=k)
        keep = R.knn_gap(red, k) >= R.GAP_SWEEP
        assert keep[[0, 4, 5, 6]].all() and keep.sum() >= 8
        assert red[0, group].tolist() == [0.0] * 5
        sixth = int(np.argsort(red[0], kind="stable")[5])
        assert m[0].nonzero()[0].tolist() == sorted((group + [sixth])[:k])       # the lower indices of the group first
        got_p, got_c = eng.neighbor_prior(qd, None, nn.KNN, k=k, want_counts=True)
        assert np.array_equal(got_c.cpu().numpy()[keep], cnt[keep])
        assert cnt[[4, 5, 6]].sum() == 0 and np.array_equal(got_p.cpu().numpy()[[4, 5, 6]], np.full((3, C), 1.0 / C))
        r, j = (t.cpu().numpy() for t in eng.neighbor_select(qd, k))
        assert j[0] == (group + [sixth])[k - 1] and (r[0] == 0.0) == (k <= 5)
        assert np.isnan(r[[4, 5, 6]]).all() and (j[[4, 5, 6]] == -1).all()
    # flags and image kinds, radius predicate
    thr = gb.radius_threshold(0.12, hav)
    cnt, _, _ = R.neighbor_counts(q, s, classes, C, hav, "distance", dist_thresh=0.12)
    prior = R.prior_neighbors(cnt)
    labels = np.array([0, 1, -1, C, 4, 2, 3, 1, 0])
    img64 = images(9, C, 5, np.float64)
    img64[1, 1] = np.nan                           # the label's score: -1
    img64[7, 3] = np.nan                           # another class's: greater counts it, argmax is its index
    labd = dev(labels, np.int32)
    for img, kind in ((img64.astype(np.float32), nn.CSP_IMG_F32), (img64, nn.CSP_IMG_F64), (None, nn.CSP_IMG_NONE)):
        got = abi_rank(eng, qd, None, nn.RADIUS, labd, None if img is None else dev(img), kind, thr=thr)
        want = R.ranks(prior, img, labels)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        assert (got[0][[2, 3]] == -2).all() and (got[2][[2, 3]] == -2).all()
        if img is not None:
            assert got[0][1] == -1 and got[1][1] == -1 and got[2][1] == -1 and got[2][7] == 3 and got[0][7] >= 1
    eng.close()


def test_split_grid_stream_and_repeats_give_the_same_bits():
    hav, C, N, B = False, 33, 1000, 25
    s, q = R.sweep_points(105, N)
    rng = np.random.default_rng(8)
    classes, labels, img = rng.integers(0, C, N), rng.integers(0, C, B), images(B, C, 8)
    cells = gb.train_cells(s, 12, 6)
    eng = engine_for(s, classes, C, hav, cells=cells)
    qd, labd, imgd = dev(q), dev(labels, np.int32), dev(img)
    qc = dev(gb.query_cells(q, 12, 6))
    assert nn.plan(B, N, C)["chunks"] == 4 and nn.plan(B, N, C, chunks=3)["chunks"] == 3 and nn.plan(B, N, C, max_grid=1)["grid"] == 1
    side = torch.cuda.Stream(device=DEV)
    for mode, kw, src in ((nn.RADIUS, dict(thr=49.0), (qd, None)), (nn.KNN, dict(k=64), (qd, None)),
                          (nn.CELL, dict(pc=2.0, cpc=66.0), (None, qc))):
        base = abi_rank(eng, src[0], src[1], mode, labd, imgd, nn.CSP_IMG_F32, chunks=1, **kw)
        base_p, base_c = (t.cpu().numpy() for t in eng.neighbor_prior(src[0], src[1], mode, want_counts=True, chunks=1, **kw))
        assert base_c.sum() > 0
        for geometry in (dict(chunks=3), dict(chunks=0), dict(chunks=64), dict(max_grid=1), dict(max_grid=2, chunks=2),
                         dict(stream=side), dict(chunks=1), dict(chunks=3)):
            got = abi_rank(eng, src[0], src[1], mode, labd, imgd, nn.CSP_IMG_F32, **geometry, **kw)
            for g, w in zip(got, base):
                assert np.array_equal(g, w), (mode, geometry)
            if "stream" not in geometry:
                p, c = (t.cpu().numpy() for t in eng.neighbor_prior(src[0], src[1], mode, want_counts=True, **geometry, **kw))
                assert np.array_equal(c, base_c) and np.array_equal(p, base_p, equal_nan=True), (mode, geometry)
    # and the restatement, for the cell predicate too
    cnt, qcell = R.grid_counts(q, s, classes, C, [12, 6])
    got = abi_rank(eng, None, qc, nn.CELL, labd, imgd, nn.CSP_IMG_F32, pc=2.0, cpc=66.0, chunks=3)
    for g, w in zip(got, R.ranks(R.prior_grid(cnt, qcell, 2), img, labels)):
        assert np.array_equal(g, w)
    eng.close()


def test_refusals():
    eng = nn.NeighborEngine(DEV)
    q = dev(np.zeros((4, 2)))
    lab = dev(np.zeros(4), np.int32)
    with pytest.raises(nn.RangeNativeError, match="range_set_neighbors"):
        eng.neighbor_select(q, 1)
    with pytest.raises(nn.RangeNativeError, match="32768"):
        eng.set_neighbors(np.zeros((3, 2)), np.zeros(3, dtype=np.int32), nn.MAX_CLASSES + 1, False)
    with pytest.raises(nn.RangeNativeError, match="training point 2"):
        eng.set_neighbors(np.zeros((3, 2)), np.array([0, 1, 5], dtype=np.int32), 5, False)
    assert eng.neighbor_points == 0
    eng.set_neighbors(np.zeros((3, 2)), np.array([0, 1, 4], dtype=np.int32), 5, False)
    with pytest.raises(nn.RangeNativeError, match="k"):
        eng.neighbor_rank(q, None, nn.KNN, labels=lab, k=4)
    with pytest.raises(nn.RangeNativeError, match="cells"):
        eng.neighbor_rank(None, dev(np.zeros(4), np.int32), nn.CELL, labels=lab, pc=2.0, cpc=10.0)
    with pytest.raises(nn.RangeNativeError, match="mode"):
        eng.neighbor_rank(q, None, 7, labels=lab)
    with pytest.raises(ValueError, match="labels"):
        eng.neighbor_rank(q, None, nn.RADIUS, labels=lab[:3], thr=1.0)
    # the class cap itself runs: one row of 128 KB
    big = nn.NeighborEngine(DEV)
    big.set_neighbors(np.array([[0.0, 0.0], [1.0, 1.0]]), np.array([7, nn.MAX_CLASSES - 1], dtype=np.int32), nn.MAX_CLASSES, False)
    p, c = big.neighbor_prior(dev(np.array([[0.0, 0.0], [50.0, 50.0]])), None, nn.RADIUS, thr=4.0, want_counts=True)
    c = c.cpu().numpy()
    assert c.sum() == 2 and c[0, 7] == 1 and c[0, nn.MAX_CLASSES - 1] == 1 and c[1].sum() == 0
    assert p.cpu().numpy()[0, 7] == 2.0 / (nn.MAX_CLASSES + 2)
    g = gb.GridPrior(np.array([[0.0, 0.0]]), np.array([0]), 3, {"gp_size": [4, 4], "pseudo_count": 2}, device=DEV)
    with pytest.raises(ValueError, match="row 0"):
        g.label_ranks(np.array([[-300.0, 0.0]]), np.array([0]))
    with pytest.raises(ValueError, match="outside the classes"):
        g.label_ranks(np.array([[0.0, 0.0]]), np.array([3]))


def test_compute_acc_batch_end_to_end(golden):
    log = logging.getLogger("neighbors-gpu-test")
    s, q = R.sweep_points(105, 1000)
    q[3] = (np.nan, 0.0)
    C, B = 33, len(q)
    rng = np.random.default_rng(12)
    classes, labels, img = rng.integers(0, C, len(s)), rng.integers(0, C, B), images(B, C, 12)
    split = (np.arange(B) % 2).astype(np.int64)
    for dist_type in ("haversine", "euclidean"):
        hp = dict(dist_type=dist_type, dist_thresh=R.SWEEP_THRESH[dist_type == "haversine"], num_neighbors=64,
                  gp_size=[12, 6], pseudo_count=2)
        host = {"nn_dist": R.NumpyNeighborPrior(s, classes, C, hp), "nn_knn": R.NumpyNeighborPrior(s, classes, C, hp),
                "grid": R.NumpyNeighborPrior(s, classes, C, hp, grid=True), "train_freq": gb.train_freq_prior(classes, C)}
        nbr = gb.NeighborPrior(s, classes, C, hp, device=DEV)
        gpu = {"nn_dist": nbr, "nn_knn": nbr, "grid": gb.GridPrior(s, classes, C, hp, device=DEV), "train_freq": host["train_freq"]}
        for ptype in ("train_freq", "nn_dist", "nn_knn", "grid"):
            for preds in (img, torch.from_numpy(img.astype(np.float64)), None):
                want = csp_eval.compute_acc_batch(None if preds is None else np.asarray(preds), labels, split, val_feats=q,
                                                  prior_type=ptype, prior=host[ptype], logger=log, return_acc=True)
                got = csp_eval.compute_acc_batch(preds, labels, split, val_feats=q, prior_type=ptype, prior=gpu[ptype],
                                                 batch_size=7, logger=log, return_acc=True)
                assert [int(c) for c in got[0]] == [int(c) for c in want[0]] and got[1] == want[1], (dist_type, ptype)
                assert len(got[0]) == B
