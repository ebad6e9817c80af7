"""GPU tests of the KDE geo prior (kde_kernel.h, include/range_neighbors.h: range_kde_*, range_amd/geo_baselines.py:
KdePrior, csp_eval.compute_acc_batch's 'kde' branch), in the three layers of tests/kde_refs.py: the kernel's raw
64-bit sums against the integer emulation under layer 2's per-member bound; prior and the three rank integers EXACT
functions of the returned sums; KdePrior.prior against the reference's recorded priors (tests/golden/kde_priors.npz)
under layer 3's derived bound.  Launch geometry, stream, repeats, the order of the bins and counts-vs-duplicates
change no bit.  Run with ``pytest -m gpu``."""
import logging
import os

import numpy as np
import pytest
import torch

import kde_refs as K
import neighbor_refs as R
from range_amd import _neighbors_native as nn
from range_amd import csp_eval
from range_amd import geo_baselines as gb

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "kde_priors.npz")
DEV = "cuda:0"
QUANTS = (5.0, 1.0, 0.001)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def dev(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))
    return torch.from_numpy(a).to(DEV)


def engine_for(blocs_deg, bclasses, counts, C, hav):
    eng = nn.NeighborEngine(DEV)
    eng.set_kde_points(R.metric_locs(blocs_deg, hav), bclasses, counts, C, hav)
    return eng


def images(B, C, seed, dtype=np.float32):
    rng = np.random.default_rng(seed)
    img = rng.random((B, C)).astype(dtype)
    img[rng.random((B, C)) < 0.1] = 0.0            # exact zeros: ties among the scores
    return img


def scan(eng, rows, B=None, **geometry):
    """(prior, sums) of the first B rows with the host's thr and two_h2."""
    B = len(rows.thr) if B is None else B
    p, s = eng.kde_prior(dev(rows.qm[:B]), dev(rows.thr[:B]), dev(rows.two_h2[:B]), want_sums=True, **geometry)
    return p.cpu().numpy(), s.cpu().numpy()


def rank(eng, rows, labels, img, B=None, **geometry):
    B = len(rows.thr) if B is None else B
    out = eng.kde_rank(dev(rows.qm[:B]), dev(rows.thr[:B]), dev(rows.two_h2[:B]), labels=dev(labels[:B], np.int32),
                       img=None if img is None else dev(img[:B]), **geometry)
    return [t.cpu().numpy() for t in out]


def assert_exact_from_sums(prior, sums, ranks, img, labels):
    assert np.array_equal(prior, K.prior_from_sums(sums))
    for g, w, name in zip(ranks, K.ranks_from_sums(sums, img, labels), ("greater", "tied_after", "argmax")):
        assert np.array_equal(g, w), name


@pytest.mark.parametrize("C", [1, 5, 33, 8142, 16384])
@pytest.mark.parametrize("hav", [True, False], ids=["haversine", "euclidean"])
def test_sweep_through_the_c_abi(hav, C):
    """M in {1, 255, 256, 257, 1000} x B in {1, G - 1, G, G + 1, 3 G + 1} x kde_nb in {1, 2, 64, M}: the raw sums within
    layer 2's bound of the emulation, prior and the three integers exact from the sums."""
    G = nn.kde_plan(1, 1, C, 1)["group"]
    assert G == {1: 8, 5: 8, 33: 8, 8142: 2, 16384: 1}[C] and 3 * G + 1 <= K.SWEEP_B
    used = 0.0
    for seed, M in K.SWEEP_SEEDS:
        s, classes, counts, q = K.sweep_points(seed, M, C)
        rng = np.random.default_rng(seed + C)
        labels, img = rng.integers(0, C, K.SWEEP_B), images(K.SWEEP_B, C, seed)
        eng = engine_for(s, classes, counts, C, hav)
        bits = eng.kde_scale_bits
        assert eng.neighbor_points == M and eng.neighbor_classes == C and bits == K.scale_bits(int(counts.sum()))
        for nb in [k for k in K.SWEEP_NBS + (M,) if k <= M]:
            rows = K.Rows(q, s, hav, nb)
            gap, own = rows.gaps()
            keep = np.minimum(gap, own) >= R.GAP_SWEEP
            assert keep.all()                                                    # (asserted on the CPU too)
            want = K.fixed_sums(rows, classes, counts, C, bits)
            bound = K.layer2_units(rows, classes, counts, C, bits)
            for B in sorted({1, G - 1, G, G + 1, 3 * G + 1} - {0}):
                prior, sums = scan(eng, rows, B)
                err = np.abs(sums - want[:B]).astype(np.float64)
                assert (err <= bound[:B]).all(), (M, nb, B, float((err - bound[:B]).max()))
                assert ((sums > 0) == (want[:B] > 0)).all() and sums.sum(1).max() < 2 ** 62
                used = max(used, float((err / np.maximum(bound[:B], 1)).max()))
                assert_exact_from_sums(prior, sums, rank(eng, rows, labels, img, B), img[:B], labels[:B])
        eng.close()
    print(f"C={C} {'haversine' if hav else 'euclidean'}: the sums use {used:.3f} of layer 2's bound")


def test_stacked_bins_nan_query_flags_and_image_kinds():
    hav, C = False, 5
    s = R.random_locs(300, 41)
    s[[40, 41, 150, 299, 12]] = s[7]               # six bins on one location, their classes below
    classes = np.arange(300) % C
    counts = 1 + np.arange(300) % 4
    q = R.queries_near(s, 9, 42)
    q[0] = s[7] + (0.01, 0.02)                     # the six are its nearest: kde_nb = 3 cuts the stack, all six are taken
    q[4] = (np.nan, 3.0)
    q[6] = (10.0, np.nan)
    eng = engine_for(s, classes, counts, C, hav)
    bits = eng.kde_scale_bits
    stack = [7, 12, 40, 41, 150, 299]
    rows = K.Rows(q, s, hav, 3)
    assert rows.members[0].nonzero()[0].tolist() == stack and rows.members[[4, 6]].sum() == 0
    gap, own = rows.gaps()
    assert min(gap.min(), own.min()) >= R.GAP_SWEEP
    # the selection on the weighted set: the k-th BIN, bit for bit (euclidean red has no library call)
    red_k = eng.neighbor_select(dev(rows.qm), 3)[0].cpu().numpy()
    assert np.array_equal(red_k, rows.red_k, equal_nan=True) and np.isnan(red_k[[4, 6]]).all()
    prior, sums = scan(eng, rows)
    want = K.fixed_sums(rows, classes, counts, C, bits)
    assert (np.abs(sums - want) <= K.layer2_units(rows, classes, counts, C, bits)).all()
    assert (sums[0] > 0).sum() == len({int(classes[j]) for j in stack})
    assert sums[[4, 6]].sum() == 0 and np.array_equal(prior[[4, 6]], np.full((2, C), 1.0 / C))
    # a NaN thr is "no member", whatever the coordinates
    rows.thr[2] = np.nan
    prior2, sums2 = scan(eng, rows)
    assert sums2[2].sum() == 0 and np.array_equal(prior2[2], np.full(C, 1.0 / C))
    keep = [0, 1, 3, 4, 5, 6, 7, 8]
    assert np.array_equal(sums2[keep], sums[keep])
    # flags and image kinds
    labels = np.array([0, 1, -1, C, 4, 2, 3, 1, 0])
    img64 = images(9, C, 5, np.float64)
    img64[1, 1] = np.nan                           # the label's score: -1
    img64[7, 3] = np.nan                           # another class's: greater counts it, argmax is its index
    for img in (img64.astype(np.float32), img64, None):
        got = rank(eng, rows, labels, img)
        for g, w in zip(got, K.ranks_from_sums(sums2, img, labels)):
            assert np.array_equal(g, w)
        assert (got[0][[2, 3]] == -2).all() and (got[2][[2, 3]] == -2).all()
        if img is not None:
            assert got[0][1] == -1 and got[1][1] == -1 and got[2][1] == -1 and got[2][7] == 3 and got[0][7] >= 1
    eng.close()


@pytest.mark.parametrize("hav", [True, False], ids=["haversine", "euclidean"])
def test_geometry_stream_order_and_duplicates_give_the_same_bits(hav):
    C, M, B = 33, 1000, K.SWEEP_B
    s, classes, counts, q = K.sweep_points(205, M, C)
    q[3] = (np.nan, 1.0)
    rng = np.random.default_rng(8)
    labels, img = rng.integers(0, C, B), images(B, C, 8)
    eng = engine_for(s, classes, counts, C, hav)
    bits = eng.kde_scale_bits
    assert nn.kde_plan(B, M, C, int(counts.sum()))["chunks"] == 4 and nn.kde_plan(B, M, C, M, max_grid=1)["grid"] == 1
    rows = K.Rows(q, s, hav, 64)
    base_p, base_s = scan(eng, rows, chunks=1)
    base_r = rank(eng, rows, labels, img, chunks=1)
    assert base_s.sum() > 0
    assert_exact_from_sums(base_p, base_s, base_r, img, labels)
    side = torch.cuda.Stream(device=DEV)
    for geometry in (dict(chunks=3), dict(chunks=0), dict(chunks=64), dict(max_grid=1), dict(max_grid=2, chunks=2), dict(chunks=1),
                     dict(chunks=3)):
        p, sm = scan(eng, rows, **geometry)
        assert np.array_equal(sm, base_s) and np.array_equal(p, base_p), geometry
        for g, w in zip(rank(eng, rows, labels, img, **geometry), base_r):
            assert np.array_equal(g, w), geometry
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        p, sm = scan(eng, rows)
        got_r = rank(eng, rows, labels, img, chunks=3)
    side.synchronize()
    assert np.array_equal(sm, base_s) and np.array_equal(p, base_p) and all(np.array_equal(g, w) for g, w in zip(got_r, base_r))
    eng.close()
    # the bins installed in another order
    perm = np.random.default_rng(4).permutation(M)
    eng = engine_for(s[perm], classes[perm], counts[perm], C, hav)
    for geometry in (dict(chunks=1), dict(chunks=3)):
        p, sm = scan(eng, rows, **geometry)
        assert np.array_equal(sm, base_s) and np.array_equal(p, base_p)
    eng.close()
    # a bin of count n installed as n bins of count 1 (the same scale bits: the total is the same)
    rep = np.repeat(np.arange(M), counts)
    eng = engine_for(s[rep], classes[rep], np.ones(len(rep), dtype=np.int64), C, hav)
    assert eng.kde_scale_bits == bits and eng.neighbor_points == counts.sum()
    p, sm = scan(eng, rows)
    assert np.array_equal(sm, base_s) and np.array_equal(p, base_p)
    eng.close()


def test_refusals_and_the_class_cap():
    eng = nn.NeighborEngine(DEV)
    ll, cls = np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0]]), np.array([0, 1, 4], dtype=np.int32)
    q, v = dev(np.array([[0.5, 0.5], [50.0, 50.0]])), dev(np.array([4.0, 4.0]))
    with pytest.raises(nn.RangeNativeError, match="16384"):
        eng.set_kde_points(ll, cls, np.ones(3), nn.KDE_MAX_CLASSES + 1, False)
    with pytest.raises(nn.RangeNativeError, match="count 0 of bin 1"):
        eng.set_kde_points(ll, cls, np.array([1, 0, 2]), 5, False)
    with pytest.raises(nn.RangeNativeError, match="count -3 of bin 2"):
        eng.set_kde_points(ll, cls, np.array([1, 1, -3]), 5, False)
    with pytest.raises(nn.RangeNativeError, match="beyond 2\\^31 - 1"):
        eng.set_kde_points(ll, cls, np.array([2 ** 30, 2 ** 30, 1]), 5, False)
    with pytest.raises(nn.RangeNativeError, match="bin|point 2"):
        eng.set_kde_points(ll, np.array([0, 1, 5], dtype=np.int32), np.ones(3), 5, False)
    assert eng.neighbor_points == 0 and eng.kde_scale_bits == 0
    with pytest.raises(nn.RangeNativeError, match="range_set_neighbors"):
        eng.kde_rank(q, v, v, labels=dev(np.zeros(2), np.int32))
    # the wrong kind of set, in both directions
    eng.set_neighbors(ll, cls, 5, False)
    assert eng.kde_scale_bits == 0
    with pytest.raises(nn.RangeNativeError, match="range_set_kde_points"):
        eng.kde_prior(q, v, v)
    with pytest.raises(nn.RangeNativeError, match="range_set_kde_points"):
        eng.kde_rank(q, v, v, labels=dev(np.zeros(2), np.int32))
    eng.set_kde_points(ll, cls, np.array([2 ** 30, 2 ** 30 - 2, 1]), 5, False)          # the largest total: 2^31 - 1
    assert eng.kde_scale_bits == 31 and eng.neighbor_points == 3
    with pytest.raises(nn.RangeNativeError, match="cells"):
        eng.neighbor_rank(None, dev(np.zeros(2), np.int32), nn.CELL, labels=dev(np.zeros(2), np.int32), pc=2.0, cpc=10.0)
    assert eng.neighbor_select(q, 3)[0].shape == (2,)                                    # the selection works on it
    p, sm = eng.kde_prior(q, v, v, want_sums=True)
    sm = sm.cpu().numpy()
    assert 0 < sm.sum(1).max() < 2 ** 62 and sm[1].sum() == 0
    with pytest.raises(ValueError, match="thresholds"):
        eng.kde_prior(q, v[:1], v)
    eng.close()
    # the class cap itself runs: one row of 128 KB
    big = nn.NeighborEngine(DEV)
    big.set_kde_points(np.array([[0.0, 0.0], [1.0, 1.0]]), np.array([7, nn.KDE_MAX_CLASSES - 1], dtype=np.int32), np.array([2, 1]),
                       nn.KDE_MAX_CLASSES, False)
    p, sm = big.kde_prior(dev(np.array([[0.0, 0.0], [50.0, 50.0]])), dev(np.array([4.0, 4.0])), dev(np.array([2.0, 2.0])), want_sums=True)
    sm, p = sm.cpu().numpy(), p.cpu().numpy()
    assert sm[0, 7] == 2 * 2 ** 52 and sm[0].nonzero()[0].tolist() == [7, nn.KDE_MAX_CLASSES - 1] and sm[1].sum() == 0
    assert abs(int(sm[0, -1]) - int(np.rint(np.exp(-1.0) * 2.0 ** 52))) <= K.member_units(K.U_EXP, 52)
    assert np.array_equal(p, K.prior_from_sums(sm))
    big.close()


@pytest.mark.parametrize("name", [f"{m}_C{c}" for m in ("haversine", "euclidean") for c in (1, 5, 33)])
def test_kde_prior_against_the_fixture(golden, name):
    """KdePrior.prior within layer 3's bound of the reference's priors on every recorded row; label_ranks and the
    bandwidth against the recorded ones."""
    hav, C = name.startswith("haversine"), int(name.split("_C")[1])
    s, q, classes, labels, img = (golden[name + k] for k in ("_s", "_q", "_classes", "_labels", "_img"))
    used = 0.0
    for n, quant in enumerate(QUANTS):
        tag = f"{name}_q{n}"
        hp = dict(kde_quant=quant, kde_nb=1, kde_dist_type="haversine" if hav else "euclidean")
        p = gb.KdePrior(s, classes, C, hp, device=DEV)
        for got, key in zip((p.binned_classes, p.binned_locs, p.counts), ("_bclasses", "_blocs", "_counts")):
            assert np.array_equal(got, golden[tag + key])
        M = p.num_bins
        bits = p.engine.kde_scale_bits
        assert bits == K.scale_bits(len(s))
        for nb, label in ((1, "1"), (7, "7"), (M, "M")):
            case = f"{tag}_nb{label}"
            p.kde_nb = nb
            want, h = golden[case + "_prior"], golden[case + "_h"]
            rows = K.Rows(q, p.binned_locs, hav, nb)
            bound = K.layer3_bound(rows, C, bits)
            got = p.prior(q)
            rel = np.abs(got - want) / want
            print(f"{case}: largest relative error {rel.max():.3e}, {float((rel / bound[:, None]).max()):.4f} of the bound")
            assert (rel <= bound[:, None]).all(), case
            used = max(used, float((rel / bound[:, None]).max()))
            nan = np.isnan(h)
            assert np.array_equal(got[nan], np.full((2, C), 1.0 / C))
            ranks, pred = p.label_ranks(q, labels, img)
            assert np.array_equal(ranks, golden[case + "_ranks"]) and np.array_equal(pred, golden[case + "_argmax"]), case
            # h: red_k within 32 ulp (haversine; exact otherwise), the host's sqrt / asin and the tree's 4 ulp
            bw = p.bandwidth(q)
            assert np.array_equal(np.isnan(bw), nan)
            amp = np.maximum(K.asin_amplification(np.sin(h[~nan]) ** 2), 0.5) if hav else 0.5
            assert (np.abs(bw[~nan] - h[~nan]) <= ((32 * amp if hav else 0) + 8) * K.ULP * h[~nan]).all(), case
        p.engine.close()
    print(f"{name}: KdePrior.prior uses {used:.4f} of layer 3's bound")


def test_kde_prior_refusals():
    s = R.random_locs(50, 3)
    classes = np.arange(50) % 3
    hp = dict(kde_quant=0.001, kde_nb=1, kde_dist_type="euclidean")
    p = gb.KdePrior(s, classes, 3, hp, device=DEV)
    q = R.queries_near(s, 4, 4)
    assert p.prior(q).shape == (4, 3)
    on = q.copy()
    on[2] = p.binned_locs[11]                       # on a bin: the nearest is at distance 0
    with pytest.raises(ValueError, match="row 2.*same location"):
        p.prior(on)
    with pytest.raises(ValueError, match="row 2.*same location"):
        p.label_ranks(on, np.zeros(4, dtype=np.int64))
    for bad in ((np.inf, 1.0), (1.0, -np.inf)):
        inf = q.copy()
        inf[1] = bad
        with pytest.raises(ValueError, match="row 1.*infinite"):
            p.prior(inf)
    p.kde_nb = p.num_bins + 1
    with pytest.raises(ValueError, match="kde_nb = 51 of 50 bins"):
        p.prior(q)
    p.kde_nb = 0
    with pytest.raises(ValueError, match="kde_nb"):
        p.bandwidth(q)
    p.kde_nb = 2
    with pytest.raises(ValueError, match="outside the classes"):
        p.label_ranks(q, np.full(4, 3))
    nanq = q.copy()
    nanq[0, 1] = np.nan
    nanq[3, 0] = np.nan
    assert np.array_equal(p.prior(nanq)[[0, 3]], np.full((2, 3), 1.0 / 3)) and np.isnan(p.bandwidth(nanq)[[0, 3]]).all()


def test_compute_acc_batch_end_to_end():
    log = logging.getLogger("kde-gpu-test")
    s, _, _, q = K.sweep_points(205, 1000, 33)
    q[3] = (np.nan, 0.0)
    C, B = 33, len(q)
    rng = np.random.default_rng(12)
    classes, labels, img = rng.integers(0, C, len(s)), rng.integers(0, C, B), images(B, C, 12)
    split = (np.arange(B) % 2).astype(np.int64)
    for dist_type in ("haversine", "euclidean"):
        hp = dict(kde_dist_type=dist_type, kde_quant=1.0, kde_nb=64)
        host, gpu = K.NumpyKdePrior(s, classes, C, hp), gb.KdePrior(s, classes, C, hp, device=DEV)
        for preds in (img, torch.from_numpy(img.astype(np.float64)), None):
            want = csp_eval.compute_acc_batch(None if preds is None else np.asarray(preds), labels, split, val_feats=q,
                                              prior_type="kde", prior=host, logger=log, return_acc=True)
            got = csp_eval.compute_acc_batch(preds, labels, split, val_feats=q, prior_type="kde", prior=gpu, batch_size=7,
                                             logger=log, return_acc=True)
            assert [int(c) for c in got[0]] == [int(c) for c in want[0]] and got[1] == want[1], dist_type
            assert len(got[0]) == B
