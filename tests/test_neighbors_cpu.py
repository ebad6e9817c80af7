"""CPU tests of the neighbour and grid geo priors (range_amd/geo_baselines.py, csp_eval.compute_acc_batch's baseline
branches, host_plan.h: neighbor_plan): the numpy restatement (tests/neighbor_refs.py) reproduces, bit for bit, what
the reference's own ``compute_neighbor_prior`` / ``GridPrior`` and scikit-learn's ``BallTree`` gave
(tests/golden/neighbor_priors.npz); planted defects each miss it; the launch plan under the host sanitizers; the
seeds of the GPU sweeps leave out no query; ``compute_acc_batch`` on numpy stand-ins.  No GPU."""
import logging
import os
import re
import subprocess

import numpy as np
import pytest

import neighbor_refs as R
from range_amd import csp_eval
from range_amd import geo_baselines as gb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "neighbor_priors.npz")
NEIGHBOR_CASES = [f"{m}_C{c}" for m in ("haversine", "euclidean") for c in (1, 5, 33)]
GRID_CASES = ["grid_pc2", "grid_pc3", "grid_pc1", "grid_pchalf"]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def case_inputs(golden, case):
    hav = case.startswith("haversine")
    C = int(case.split("_C")[1])
    return hav, C, golden[case + "_s"], golden[case + "_q"], golden[case + "_classes"]


@pytest.mark.parametrize("case", NEIGHBOR_CASES)
def test_restatement_reproduces_the_reference(golden, case):
    hav, C, s, q, classes = case_inputs(golden, case)
    thresh = float(golden[case + "_dist_thresh"])
    cnt, m, red = R.neighbor_counts(q, s, classes, C, hav, "distance", dist_thresh=thresh)
    assert np.array_equal(m, golden[case + "_members_distance"].astype(bool))
    assert np.array_equal(R.prior_neighbors(cnt), golden[case + "_prior_distance"])          # bit for bit
    assert R.threshold_gap(red, gb.radius_threshold(thresh, hav)).min() >= R.GAP_FIXTURE
    assert m.sum(1).min() == 0 and np.isnan(q[:, 0]).sum() == 1
    for k in golden[case + "_ks"]:
        k = int(k)
        cnt, m, red = R.neighbor_counts(q, s, classes, C, hav, "knn", k=k)
        assert np.array_equal(m, golden[f"{case}_members_knn{k}"].astype(bool))
        assert np.array_equal(R.prior_neighbors(cnt), golden[f"{case}_prior_knn{k}"])
        assert R.knn_gap(red, k).min() >= R.GAP_FIXTURE
        # the k-th distance BallTree.query returned, from red_k
        red_k, j_last = R.select_kth(red, k)
        with np.errstate(invalid="ignore"):
            d = 2 * np.arcsin(np.sqrt(red_k)) if hav else np.sqrt(red_k)
        want = golden[f"{case}_kth{k}"]
        assert np.array_equal(np.isnan(d), np.isnan(want))
        np.testing.assert_allclose(d[~np.isnan(d)], want[~np.isnan(want)], rtol=1e-12)
        assert (j_last[np.isnan(red_k)] == -1).all()
    # the NaN query: the uniform prior
    nan_row = int(np.flatnonzero(np.isnan(q[:, 0]))[0])
    assert np.array_equal(golden[case + "_prior_distance"][nan_row], np.ones(C) / C)


@pytest.mark.parametrize("case", GRID_CASES)
def test_grid_restatement_reproduces_the_reference(golden, case):
    s, q, classes = golden[case + "_s"], golden[case + "_q"], golden[case + "_classes"]
    gp_size, pc, want = [int(v) for v in golden[case + "_gp_size"]], float(golden[case + "_pseudo_count"]), golden[case + "_prior"]
    pc = int(pc) if pc == int(pc) else pc
    C = want.shape[1]
    cnt, qc = R.grid_counts(q, s, classes, C, gp_size)
    got = R.prior_grid(cnt, qc, pc)
    assert np.array_equal(got, want, equal_nan=True)                                          # bit for bit, NaN where 0 / 0
    sc = gb.train_cells(s, *gp_size)
    assert sc[0] == gp_size[0] * gp_size[1] - 1 and sc[1] >= 0 and sc[2] == -2 and sc[4] == -2    # closed edge; outside
    assert (qc == -1).sum() == 1 and cnt[5].sum() >= 1
    if case == "grid_pc1":
        assert np.isnan(want).any()


def test_planted_defects_miss_the_fixture(golden):
    case = "haversine_C33"
    hav, C, s, q, classes = case_inputs(golden, case)
    want_d, want_k = golden[case + "_prior_distance"], golden[case + "_prior_knn7"]
    qm, sm = R.metric_locs(q, hav), R.metric_locs(s, hav)
    red = R.red_matrix(qm, sm, hav)
    thr = gb.radius_threshold(float(golden[case + "_dist_thresh"]), hav)
    assert np.array_equal(R.prior_neighbors(R.counts_of(R.members_radius(red, thr), classes, C)), want_d)
    # lon / lat swapped
    swapped = R.red_matrix(qm[:, ::-1], sm[:, ::-1], hav)
    assert not np.array_equal(R.prior_neighbors(R.counts_of(R.members_radius(swapped, thr), classes, C)), want_d)
    assert not np.array_equal(R.prior_neighbors(R.counts_of(R.members_knn(swapped, 7), classes, C)), want_k)
    # `<` for `<=`: a query that sits on a training point, threshold 0 (the point itself is a member)
    on = R.red_matrix(sm[:4], sm, hav)
    assert R.members_radius(on, 0.0).sum(1).min() >= 1 and R.members_radius(on, 0.0, strict=True).sum() == 0
    # the k-boundary inside a group of exact duplicates: the total order takes the lower indices
    dup = np.concatenate([s[:10], s[[3, 3, 3]]])
    cls = np.arange(13) % C
    redd = R.red_matrix(R.metric_locs(s[3:4], hav), R.metric_locs(dup, hav), hav)
    m = R.members_knn(redd, 2)
    assert m[0].nonzero()[0].tolist() == [3, 10]
    other = np.zeros_like(m)
    other[0, [11, 12]] = True                      # the same distances, the group cut in another order
    assert not np.array_equal(R.counts_of(m, cls, C), R.counts_of(other, cls, C))
    # the grid: pseudo_count off by one, and the open last edge
    g = "grid_pc2"
    gs, gq, gcls, want = golden[g + "_s"], golden[g + "_q"], golden[g + "_classes"], golden[g + "_prior"]
    gp_size = [int(v) for v in golden[g + "_gp_size"]]
    cnt, qc = R.grid_counts(gq, gs, gcls, want.shape[1], gp_size)
    assert np.array_equal(R.prior_grid(cnt, qc, 2), want)
    assert not np.array_equal(R.prior_grid(cnt, qc, 2, off_by=1), want)
    sc = gb.train_cells(gs, *gp_size)
    x = (gs[:, 0] + 180) / 360.0 * gp_size[0]
    y = (gs[:, 1] + 90) / 180.0 * gp_size[1]
    sc_open = np.where((x >= gp_size[0]) | (y >= gp_size[1]), -2, sc)          # the last edge open
    cnt_open = R.counts_of(qc[:, None] == sc_open[None, :], gcls, want.shape[1])
    assert not np.array_equal(R.prior_grid(cnt_open, qc, 2), want)


def test_sweep_seeds_leave_out_no_query():
    """The GPU sweeps leave out queries nearer than 2^-40 (relative) to a threshold; with these seeds there is none."""
    for hav in (True, False):
        for seed, N in R.SWEEP_SEEDS:
            s, q = R.sweep_points(seed, N)
            red = R.red_matrix(R.metric_locs(q, hav), R.metric_locs(s, hav), hav)
            assert R.threshold_gap(red, gb.radius_threshold(R.SWEEP_THRESH[hav], hav)).min() >= R.GAP_SWEEP
            for k in R.SWEEP_KS + (N,):
                if k <= N:
                    assert R.knn_gap(red, k).min() >= R.GAP_SWEEP, (hav, seed, k)


def test_cells_and_thresholds():
    assert gb.radius_threshold(2.0, False) == 4.0 and gb.radius_threshold(0.3, True) == np.sin(0.15) ** 2
    # int() truncation: just below zero is cell 0, as the reference's int() gives; the far edge is outside
    assert gb.query_cells(np.array([[-180.0 - 1e-9, -90.0]]), 10, 5).tolist() == [0]
    assert gb.query_cells(np.array([[np.nan, 0.0], [179.9, 89.9]]), 10, 5).tolist() == [-1, 49]
    with pytest.raises(ValueError, match="row 1"):
        gb.query_cells(np.array([[0.0, 0.0], [180.0, 0.0]]), 10, 5)
    with pytest.raises(ValueError, match="row 0"):
        gb.query_cells(np.array([[-220.0, 0.0]]), 10, 5)     # (-200 truncates to cell 0, as int() does)
    with pytest.raises(ValueError, match="row 0"):
        gb.query_cells(np.array([[0.0, np.nan]]), 10, 5)
    assert gb.train_cells(np.array([[180.0, 90.0], [-180.0, -90.0], [180.1, 0.0], [np.nan, 0.0]]), 10, 5).tolist() == [49, 0, -2, -2]


def test_train_freq_and_hyper_params():
    cls = np.array([0, 0, 3, 1, 3, 3])
    p = gb.train_freq_prior(cls, 5)
    assert np.array_equal(p, np.array([3.0, 2.0, 1.0, 4.0, 1.0]) / 11.0)
    hp = gb.get_cross_val_hyper_params("inat_2018")
    assert hp == dict(num_neighbors=1500, dist_type="euclidean", dist_thresh=2.0, gp_size=[180, 60], pseudo_count=2,
                      kde_dist_type="euclidean", kde_quant=5.0, kde_nb=700)
    assert gb.get_cross_val_hyper_params({"dataset": "birdsnap", "meta_type": "orig_meta"})["num_neighbors"] == 100
    assert gb.get_cross_val_hyper_params("yfcc")["dist_thresh"] == 2.0 / 6371.4 and gb.get_cross_val_hyper_params("nope") == {}
    hp["gp_size"][0] = 1                         # a copy: the table stays
    assert gb.get_cross_val_hyper_params("inat_2018")["gp_size"] == [180, 60]


def test_compute_acc_batch_on_stand_in_priors(golden):
    case = "euclidean_C33"
    hav, C, s, q, classes = case_inputs(golden, case)
    hp = dict(dist_type="euclidean", dist_thresh=float(golden[case + "_dist_thresh"]), num_neighbors=7, gp_size=[12, 6],
              pseudo_count=2)
    rng = np.random.default_rng(9)
    B = q.shape[0]
    img = rng.random((B, C)).astype(np.float32)
    labels = rng.integers(0, C, B)
    split = (np.arange(B) % 3 == 0).astype(np.int64)
    log = logging.getLogger("neighbors-test")

    def expect(prior, preds):
        g, e, am = R.ranks(prior, preds, labels)
        ranks = 1 + g.astype(np.int64) + e
        return am.tolist(), {sid: {k: round(int((ranks[split == sid] <= k).sum()) * 100 / int((split == sid).sum()), 2)
                                   for k in csp_eval.TOP_KS} for sid in (0, 1)}

    for ptype, tag in (("nn_dist", "distance"), ("nn_knn", "knn7")):
        prior = R.NumpyNeighborPrior(s, classes, C, hp)
        for preds in (img, None):
            pred, acc = csp_eval.compute_acc_batch(preds, labels, split, val_feats=q, prior_type=ptype, prior=prior,
                                                   batch_size=10, logger=log, return_acc=True)
            want_pred, want_acc = expect(golden[f"{case}_prior_{tag}"], preds)
            assert [int(c) for c in pred] == want_pred and acc == want_acc and len(pred) == B     # no row dropped
        assert prior.calls == 8
    gq = golden["grid_pc2_q"]
    prior = R.NumpyNeighborPrior(golden["grid_pc2_s"], golden["grid_pc2_classes"], 33, hp, grid=True)
    pred, acc = csp_eval.compute_acc_batch(img, labels, split, val_feats=gq, prior_type="grid", prior=prior, logger=log,
                                           return_acc=True)
    assert ([int(c) for c in pred], acc) == expect(golden["grid_pc2_prior"], img)
    # train_freq: the (C,) array, on the host
    freq = gb.train_freq_prior(classes, C)
    for preds in (img, None):
        pred, acc = csp_eval.compute_acc_batch(preds, labels, split, prior_type="train_freq", prior=freq, batch_size=7,
                                               logger=log, return_acc=True)
        assert ([int(c) for c in pred], acc) == expect(np.repeat(freq[None], B, 0), preds)
    # refusals
    assert csp_eval.UNSUPPORTED_PRIORS == ("kde", "tang_et_al")
    for name in csp_eval.BASELINE_PRIORS:
        with pytest.raises(NotImplementedError, match=name):
            csp_eval.compute_acc_batch(img, labels, split, val_feats=q, prior_type=name, prior=None, logger=log)
    with pytest.raises(ValueError, match="val_feats"):
        csp_eval.compute_acc_batch(img, labels, split, prior_type="nn_knn", prior=R.NumpyNeighborPrior(s, classes, C, hp), logger=log)
    with pytest.raises(ValueError, match="outside"):
        csp_eval.compute_acc_batch(img, labels + C, split, prior_type="train_freq", prior=freq, logger=log)


def test_bindings_declare_the_neighbor_entry_points():
    from range_amd import _neighbors_native as nn
    header = open(os.path.join(REPO, "include", "range_neighbors.h")).read()
    assert set(re.findall(r"\b(range_(?:set_)?neighbor[a-z0-9_]*)\s*\(", header)) == set(nn.SYMBOLS)
    for name, value in (("RADIUS", 0), ("KNN", 1), ("CELL", 2), ("MAX_CLASSES", 32768)):
        assert f"#define RANGE_NEIGHBOR_{name} {value}" in header and getattr(nn, name) == value
    assert "#define RANGE_ABI_VERSION 9" in open(os.path.join(REPO, "include", "range_hip.h")).read()
    lib = nn.load_library()
    for name in nn.SYMBOLS:
        assert hasattr(lib, name)
    p = nn.plan(24000, 436000, 8142, 1500)
    assert p["group"] == 4 and p["groups"] == 6000 and p["chunks"] == 1 and p["ws_bytes"] == 0 and p["passes"] * p["digit_bits"] >= 64
    assert nn.plan(9, 1000, 33)["group"] == 8 and nn.plan(9, 1000, 33, chunks=3)["chunks"] == 3
    for bad in ((0, 5, 3, 0), (5, 0, 3, 0), (5, 5, 32769, 0), (5, 5, 3, 6)):
        with pytest.raises(nn.RangeNativeError):
            nn.plan(*bad)


def test_prior_objects_refuse_without_a_gpu_or_with_bad_arguments():
    s = R.random_locs(20, 1)
    with pytest.raises(RuntimeError, match="GPU only"):
        gb.NeighborPrior(s, np.zeros(20, dtype=np.int64), 3, {"dist_type": "euclidean"}, device="cpu")
    with pytest.raises(ValueError, match="train_locs"):
        gb.NeighborPrior(np.zeros((0, 2)), np.zeros(0, dtype=np.int64), 3, {}, device="cpu")
    with pytest.raises(ValueError, match="gp_size"):
        gb.GridPrior(s, np.zeros(20, dtype=np.int64), 3, {"gp_size": [0, 4], "pseudo_count": 2}, device="cpu")


def test_neighbor_plan_under_sanitizers(tmp_path):
    """host_plan.h: neighbor_plan (tests/native/neighbor_plan.cpp) compiled with g++ under AddressSanitizer and
    UndefinedBehaviorSanitizer and run on the CPU."""
    exe = str(tmp_path / "neighbor_plan")
    src = os.path.join(REPO, "tests", "native", "neighbor_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    src, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "neighbor_plan ok" in p.stdout, p.stdout + p.stderr
