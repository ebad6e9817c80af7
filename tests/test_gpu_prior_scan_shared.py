"""The scan, the fold and the workspace that the count rows (neighbor_kernel.h) and the KDE rows (kde_kernel.h) share,
where the sharing can break and the sweeps of test_gpu_neighbors.py / test_gpu_kde.py do not reach: a group of 7
queries, whose rows end off a 16-byte boundary so that the query records sit behind padding, and one context that
runs split scans of both row kinds through its one workspace."""
import numpy as np
import pytest
import torch

import kde_refs as K
import neighbor_refs as R
from range_amd import _neighbors_native as nn
from range_amd import geo_baselines as gb

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G_ODD = 7
B_ODD = G_ODD + 1                                 # one full group and one with a single live row
# one chunk; two chunks of one tile each: a real fold; one workgroup walking both groups
GEOMETRIES = (dict(chunks=1), dict(chunks=2), dict(max_grid=1))


def dev(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))
    return torch.from_numpy(a).to(DEV)


def images(B, C, seed):
    rng = np.random.default_rng(seed)
    img = rng.random((B, C)).astype(np.float32)
    img[rng.random((B, C)) < 0.1] = 0.0            # exact zeros: ties among the scores
    return img


def assert_geometries(plan_of):
    """GEOMETRIES are what their comments say for 257 points and B_ODD queries."""
    want = (dict(grid=2, chunks=1), dict(grid=2, chunks=2), dict(grid=1, chunks=1))
    for geometry, w in zip(GEOMETRIES, want):
        p = plan_of(**geometry)
        assert p["group"] == G_ODD and p["groups"] == 2 and {k: p[k] for k in w} == w, geometry
        assert (p["lds_bytes"] - G_ODD * 48) % 16 == 0 and (p["ws_bytes"] > 0) == (p["chunks"] > 1)


def neighbor_results(eng, q, labels, img, geometry, **kw):
    prior, counts = eng.neighbor_prior(q, None, want_counts=True, **geometry, **kw)
    ranks = eng.neighbor_rank(q, None, labels=labels, img=img, **geometry, **kw)
    return [t.cpu().numpy() for t in (prior, counts) + tuple(ranks)]


def kde_results(eng, rows, B, labels, img, geometry):
    q, thr, two_h2 = dev(rows.qm[:B]), dev(rows.thr[:B]), dev(rows.two_h2[:B])
    prior, sums = eng.kde_prior(q, thr, two_h2, want_sums=True, **geometry)
    ranks = eng.kde_rank(q, thr, two_h2, labels=labels, img=img, **geometry)
    return [t.cpu().numpy() for t in (prior, sums) + tuple(ranks)]


@pytest.mark.parametrize("hav", [True, False], ids=["haversine", "euclidean"])
def test_count_rows_with_seven_queries_a_workgroup(hav):
    C, N, B = 4225, 257, B_ODD
    assert (G_ODD * C * 4) % 16 != 0
    assert_geometries(lambda **g: nn.plan(B, N, C, **g))
    s, q = R.sweep_points(104, N)
    rng = np.random.default_rng(104 + C)
    classes, labels, img = rng.integers(0, C, N), rng.integers(0, C, B), images(B, C, 104)
    eng = nn.NeighborEngine(DEV)
    eng.set_neighbors(R.metric_locs(s, hav), classes, C, hav)
    qd, labd, imgd = dev(R.metric_locs(q, hav)[:B]), dev(labels, np.int32), dev(img)
    red = R.red_matrix(R.metric_locs(q, hav), R.metric_locs(s, hav), hav)
    thresh = R.SWEEP_THRESH[hav]
    for ptype, k in (("distance", None), ("knn", 64)):
        gap = R.threshold_gap(red, gb.radius_threshold(thresh, hav)) if ptype == "distance" else R.knn_gap(red, k)
        keep = gap >= R.GAP_SWEEP
        assert (~keep).sum() <= 0.01 * len(keep)
        rows = np.flatnonzero(keep[:B])
        cnt, _, _ = R.neighbor_counts(q, s, classes, C, hav, ptype, dist_thresh=thresh, k=k)
        prior = R.prior_neighbors(cnt)
        kw = dict(mode=nn.RADIUS, thr=gb.radius_threshold(thresh, hav)) if ptype == "distance" else dict(mode=nn.KNN, k=k)
        got = [neighbor_results(eng, qd, labd, imgd, geometry, **kw) for geometry in GEOMETRIES]
        for geometry, g in zip(GEOMETRIES, got):
            assert g[1].sum() > 0
            assert np.array_equal(g[1][rows], cnt[:B][rows]), (ptype, geometry)
            assert np.array_equal(g[0][rows], prior[:B][rows]), (ptype, geometry)
            for r, w, name in zip(g[2:], R.ranks(prior[:B][rows], img[rows], labels[rows]), ("greater", "tied_after", "argmax")):
                assert np.array_equal(r[rows], w), (ptype, geometry, name)
            assert all(np.array_equal(a, b) for a, b in zip(g, got[0])), (ptype, geometry)
    eng.close()


@pytest.mark.parametrize("hav", [True, False], ids=["haversine", "euclidean"])
def test_kde_rows_with_seven_queries_a_workgroup(hav):
    C, M, B, nb = 2113, 257, B_ODD, 64
    assert (G_ODD * C * 8) % 16 != 0
    s, classes, counts, q = K.sweep_points(204, M, C)
    assert_geometries(lambda **g: nn.kde_plan(B, M, C, int(counts.sum()), **g))
    rng = np.random.default_rng(204 + C)
    labels, img = rng.integers(0, C, B), images(B, C, 204)
    eng = nn.NeighborEngine(DEV)
    eng.set_kde_points(R.metric_locs(s, hav), classes, counts, C, hav)
    bits = eng.kde_scale_bits
    assert bits == K.scale_bits(int(counts.sum()))
    rows = K.Rows(q, s, hav, nb)
    gap, own = rows.gaps()
    assert (np.minimum(gap, own) >= R.GAP_SWEEP).all()
    want = K.fixed_sums(rows, classes, counts, C, bits)[:B]
    bound = K.layer2_units(rows, classes, counts, C, bits)[:B]
    got = [kde_results(eng, rows, B, dev(labels, np.int32), dev(img), geometry) for geometry in GEOMETRIES]
    for geometry, (prior, sums, *ranks) in zip(GEOMETRIES, got):
        err = np.abs(sums - want).astype(np.float64)
        assert (err <= bound).all(), (geometry, float((err - bound).max()))
        assert ((sums > 0) == (want > 0)).all() and (sums > 0).any() and sums.sum(1).max() < 2 ** 62
        assert np.array_equal(prior, K.prior_from_sums(sums)), geometry
        for r, w, name in zip(ranks, K.ranks_from_sums(sums, img, labels), ("greater", "tied_after", "argmax")):
            assert np.array_equal(r, w), (geometry, name)
        assert all(np.array_equal(a, b) for a, b in zip([prior, sums] + ranks, got[0])), geometry
    eng.close()


def test_one_context_both_row_kinds_one_workspace():
    """Neighbours, KDE bins and the neighbours again on one engine, each scanned in two chunks through the one
    workspace: what a fresh engine gives in one chunk."""
    hav, C, N, B = False, 33, 257, R.SWEEP_B
    s, q = R.sweep_points(104, N)
    ks, kclasses, kcounts, kq = K.sweep_points(204, N, C)
    rng = np.random.default_rng(11)
    classes, labels, img = rng.integers(0, C, N), dev(rng.integers(0, C, B), np.int32), dev(images(B, C, 11))
    rows = K.Rows(kq, ks, hav, 64)
    thr = gb.radius_threshold(R.SWEEP_THRESH[hav], hav)
    assert nn.plan(B, N, C, chunks=2)["chunks"] == 2 and nn.kde_plan(B, N, C, int(kcounts.sum()), chunks=2)["chunks"] == 2
    # the KDE rows' workspace is twice the count rows': the second installation makes the one buffer grow
    assert nn.kde_plan(B, N, C, int(kcounts.sum()), chunks=2)["ws_bytes"] == 2 * nn.plan(B, N, C, chunks=2)["ws_bytes"]

    def neighbors(eng, geometry):
        eng.set_neighbors(s, classes, C, hav)
        return (neighbor_results(eng, dev(q), labels, img, geometry, mode=nn.RADIUS, thr=thr)
                + neighbor_results(eng, dev(q), labels, img, geometry, mode=nn.KNN, k=64))

    def kde(eng, geometry):
        eng.set_kde_points(ks, kclasses, kcounts, C, hav)
        return kde_results(eng, rows, B, labels, img, geometry)

    fresh = []
    for step in (neighbors, kde):
        eng = nn.NeighborEngine(DEV)
        fresh.append(step(eng, dict(chunks=1)))
        eng.close()
    assert fresh[0][1].sum() > 0 and fresh[0][6].sum() > 0 and (fresh[1][1] > 0).any()
    eng = nn.NeighborEngine(DEV)
    for step, want in ((neighbors, fresh[0]), (kde, fresh[1]), (neighbors, fresh[0])):
        got = step(eng, dict(chunks=2))
        assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want)), step.__name__
    eng.close()
