"""The other tenants of a context that has a history (`-m gpu`): the CSP network and its class head, the neighbour /
KDE slot, the positional encoders' frequency tables, the checkerboard scan - all on ONE context that also serves an
exact retrieval bank, whose results must not move - and the probe context's map and cluster workspaces.

Each family's result on the used context equals, bit for bit, the result of a fresh context that only ever saw the
final state, and meets that family's existing reference at its existing bound (csp_head_refs, csp_rank_refs,
neighbor_refs, kde_refs, posenc_refs, checker_refs, icamap_refs, cluster_refs).  What a replaced installation leaves
behind in the grow-only buffers is made to show: a poisoned larger head under a smaller one, training points of the
wrong class at the queries' own locations behind a smaller set, a larger support set behind a smaller one.
"""
import os

import numpy as np
import pytest
import torch

import checker_refs as CK
import cluster_refs as CL
import csp_head_refs as H
import csp_rank_refs as RK
import csp_refs as CR
import icamap_refs as IM
import kde_refs as K
import lifecycle as L
import neighbor_refs as R
import posenc_refs as P
from exact_helpers import DEV, _assert_equal, _dev
from range_amd import _cluster_native, _map_native, _native, csp, posenc
from range_amd import _neighbors_native as nn
from range_amd import geo_baselines as gb
from tools import exact_bank as X

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
INVALID, STATE = -1, -3
PROBS, LOGITS, SUM = _native.CSP_HEAD_PROBS, _native.CSP_HEAD_LOGITS, _native.CSP_HEAD_SUM
KIND = {"gridcell": posenc.KIND_GRID, "theory": posenc.KIND_THEORY}
RET_N = 4099

_USED = []


def _used():
    """The one context of this module: every family below runs on it, and so does the retrieval."""
    if not _USED:
        eng = nn.NeighborEngine(DEV)
        eng.set_bank(*L.exact(RET_N).rows(0, RET_N))
        _USED.append(eng)
    return _USED[0]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for e in _USED:
        e.close()
    _USED.clear()
    torch.cuda.empty_cache()


def _retrieval(eng):
    """Statistics, pass 2 from kept logits and the top-k stream on the exact bank: exact, and returned."""
    bank, q = L.exact(RET_N), L.route_queries(RET_N)
    e32, xq = _dev(q.e32), _dev(q.xq)
    st = eng.scan_stats(e32, xq, L.TAU, L.TAU, keep_logits=True)
    out = eng.attend_kept(0, xq, L.TAU, L.TAU, L.BETA, st)
    tv, ti = eng.topk_stream(e32, 16)
    _assert_equal(st, _dev(X.expect_stats(bank, q, L.TAU, L.TAU)), "scan_stats")
    _assert_equal(out, _dev(X.expect(bank, q, L.BETA)), "attend_kept")
    wv, wi = X.topk_expect(bank, q, 16)
    _assert_equal(ti, _dev(wi), "topk_stream indices")
    _assert_equal(tv, _dev(wv), "topk_stream values")
    return st, out, tv, ti


def _same_retrieval(eng, before, what):
    for a, b in zip(_retrieval(eng), before):
        assert torch.equal(a, b), f"the retrieval moved behind {what}"


def dev(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))
    return torch.from_numpy(a).to(DEV)


def _equal(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        same = g.dtype == w.dtype and np.array_equal(g, w, equal_nan=g.dtype.kind == "f")
        assert same, f"{what}: output {i} differs from a fresh context's"


# -- the CSP network and its head ----------------------------------------------------------------------------------
def _install_net(eng, net):
    widths = [w.shape[0] for w in net["weights"]]
    eng.set_csp(KIND[net["spa_enc_type"]], net["freq_list"], widths, net["weights"], net["biases"], net["ln_gamma"],
                net["ln_beta"], csp.ACTIVATIONS[net["act"]], net["skip"], net["use_layn"])


def _csp_outputs(eng, feats, lonlat, img, labels):
    """The head's three modes, the fused predict call and the rank integers, as host arrays."""
    x, q = dev(feats, np.float32), dev(lonlat, np.float64)
    outs = [eng.csp_head(x, None, m) for m in (PROBS, LOGITS, SUM)]
    outs += [eng.csp_predict(q, None, PROBS), eng.csp_predict(q, None, SUM)]
    outs += list(eng.csp_rank(x, dev(labels, np.int32), None if img is None else dev(img)))
    return [t.cpu().numpy() for t in outs]


def test_csp_network_replaced_behind_a_head():
    """8 142 classes -> the network replaced (the head must be gone) -> 33 classes -> another network -> 5 classes, each
    smaller head over the larger one's buffer, whose last contents saturate the sigmoid."""
    enc_g, head_g = np.load(os.path.join(GOLDEN, "csp_encoders.npz")), np.load(os.path.join(GOLDEN, "csp_head.npz"))
    used = _used()
    before = _retrieval(used)
    lonlat = enc_g["lonlat"]
    prev_C = 0
    for case in ("design", "theory", "c_odd"):
        head = H.case_head(enc_g, head_g, case)
        net = CR.case_network(enc_g, head["enc_case"])
        W, feats, C = head["W"], head["feats"], head["C"]
        rows = H.finite_rows(feats)
        img, labels = RK.inputs(case, C, feats.shape[0])
        _install_net(used, net)
        assert used.csp_classes == 0, "a head survived the replacement of its network"
        if prev_C:
            x, q = dev(feats, np.float32), dev(lonlat, np.float64)
            buf = torch.full((feats.shape[0] * prev_C,), -7.0, dtype=torch.float32, device=DEV)
            s = torch.cuda.current_stream().cuda_stream
            n = feats.shape[0]
            assert used.lib.range_csp_head(used._h, x.data_ptr(), n, None, prev_C, PROBS, buf.data_ptr(), s) == INVALID
            assert used.lib.range_csp_predict(used._h, q.data_ptr(), n, None, prev_C, PROBS, buf.data_ptr(), s) == INVALID
            assert bool((buf == -7.0).all())
        used.set_csp_head(W)
        assert used.csp_classes == C
        fresh = _native.HipEngine(DEV)
        try:
            _install_net(fresh, net)
            fresh.set_csp_head(W)
            want = _csp_outputs(fresh, feats, lonlat, img, labels)
        finally:
            fresh.close()
        got = _csp_outputs(used, feats, lonlat, img, labels)
        _equal(got, want, f"{case}: head of {C} classes behind {prev_C}")
        probs, logits, sums = got[0], got[1], got[2]
        kinds = {"probs": probs[:, head["cols"]], "single": probs[:, head["classes"]], "logits": logits[:, head["classes"]],
                 "sums": sums}
        for kind in H.KINDS:
            err = float(np.abs(kinds[kind][rows].astype(np.float64) - H.restated(head, kind)[rows]).max())
            assert err <= H.gpu_bound(head_g, case, head, kind), (case, kind, err)
        # the rank integers: the counting rule on the head's own probabilities (test_gpu_csp_rank's exact check)
        for g, w, name in zip(got[5:], RK.rank_rule(RK.scores(probs, img), labels), ("greater", "tied_after", "argmax")):
            assert np.array_equal(g.astype(np.int64), w), (case, name)
        # leave a head behind whose probabilities are all 0 or 1: what a stale column would show
        used.set_csp_head((W.astype(np.float64) * 1e6).astype(np.float32))
        sat = used.csp_head(dev(feats, np.float32), None, PROBS).cpu().numpy()[rows]
        assert np.isin(sat, (0.0, 1.0)).mean() > 0.99
        prev_C = C
        _same_retrieval(used, before, f"the CSP head of {C} classes")


# -- the neighbour / KDE slot ----------------------------------------------------------------------------------------
def _images(B, C, seed):
    rng = np.random.default_rng(seed)
    img = rng.random((B, C)).astype(np.float32)
    img[rng.random((B, C)) < 0.1] = 0.0
    return img


def _neighbor_outputs(eng, q, labels, img, thr, k, **geometry):
    out = []
    for kw in (dict(mode=nn.RADIUS, thr=thr), dict(mode=nn.KNN, k=k)):
        prior, counts = eng.neighbor_prior(q, None, want_counts=True, **geometry, **kw)
        out += [prior, counts] + list(eng.neighbor_rank(q, None, labels=labels, img=img, **geometry, **kw))
    return [t.cpu().numpy() for t in out]


def _kde_outputs(eng, rows, B, labels, img, **geometry):
    q, thr, two_h2 = dev(rows.qm[:B]), dev(rows.thr[:B]), dev(rows.two_h2[:B])
    prior, sums = eng.kde_prior(q, thr, two_h2, want_sums=True, **geometry)
    return [t.cpu().numpy() for t in (prior, sums) + tuple(eng.kde_rank(q, thr, two_h2, labels=labels, img=img, **geometry))]


def test_neighbor_sets_shrink_and_change_kind():
    """5 000 points of 40 classes - among them points of class 6 AT the small set's queries - then 300 points of 7
    classes: votes, priors and ranks exact; then a weighted set smaller still, then the 300 again."""
    hav, B, k = False, R.SWEEP_B, 64
    N1, C1, N2, C2, M3 = 5000, 40, 300, 7, 120
    s2, q2 = R.sweep_points(104, N2)
    rng = np.random.default_rng(5)
    cls2 = rng.integers(0, C2, N2)
    s1 = np.concatenate([R.sweep_points(105, N2)[0], np.resize(q2[:B], (N1 - N2, 2))])
    cls1 = np.concatenate([rng.integers(0, C1, N2), np.full(N1 - N2, 6)])
    labels2, img2 = dev(rng.integers(0, C2, B), np.int32), dev(_images(B, C2, 5))
    labels1, img1 = dev(rng.integers(0, C1, B), np.int32), dev(_images(B, C1, 6))
    thr = gb.radius_threshold(R.SWEEP_THRESH[hav], hav)
    qd = dev(q2[:B])
    ks, kcls, kcnt, kq = K.sweep_points(204, M3, C2)
    krows = K.Rows(kq, ks, hav, 64)

    fresh = nn.NeighborEngine(DEV)
    try:
        fresh.set_neighbors(s2, cls2, C2, hav)
        want2 = _neighbor_outputs(fresh, qd, labels2, img2, thr, k)
    finally:
        fresh.close()
    fresh = nn.NeighborEngine(DEV)
    try:
        fresh.set_kde_points(ks, kcls, kcnt, C2, hav)
        want3 = _kde_outputs(fresh, krows, B, labels2, img2)
    finally:
        fresh.close()

    used = _used()
    before = _retrieval(used)
    used.set_neighbors(s1, cls1, C1, hav)
    big = _neighbor_outputs(used, qd, labels1, img1, thr, k, chunks=2)          # (the split scan: its partial rows stay behind)
    assert (big[1][:, 6] > 0).all() and (big[6][:, 6] > 0).all(), "the planted points do not vote"
    assert used.kde_scale_bits == 0
    for geometry in (dict(), dict(chunks=2)):
        used.set_neighbors(s2, cls2, C2, hav)
        assert used.neighbor_points == N2 and used.neighbor_classes == C2 and used.kde_scale_bits == 0
        got2 = _neighbor_outputs(used, qd, labels2, img2, thr, k, **geometry)
        _equal(got2, want2, f"300 points behind 5 000 {geometry}")
        # the integer results of neighbor_refs, on the queries that keep the sweep's distance from a threshold
        red = R.red_matrix(q2, s2, hav)
        for ptype, o in (("distance", 0), ("knn", 5)):
            gap = R.threshold_gap(red, thr) if ptype == "distance" else R.knn_gap(red, k)
            rows = np.flatnonzero((gap >= R.GAP_SWEEP)[:B])
            assert len(rows) >= B - 1
            cnt, _, _ = R.neighbor_counts(q2, s2, cls2, C2, hav, ptype, dist_thresh=R.SWEEP_THRESH[hav], k=k)
            prior = R.prior_neighbors(cnt)
            assert np.array_equal(got2[o + 1][rows], cnt[:B][rows]) and np.array_equal(got2[o][rows], prior[:B][rows]), ptype
            ranks = R.ranks(prior[:B][rows], img2.cpu().numpy()[rows], labels2.cpu().numpy()[rows])
            for g, w, name in zip(got2[o + 2:o + 5], ranks, ("greater", "tied_after", "argmax")):
                assert np.array_equal(g[rows], w), (ptype, name)
        with pytest.raises(nn.RangeNativeError, match=f"error {STATE}:"):
            used.kde_rank(dev(krows.qm[:B]), dev(krows.thr[:B]), dev(krows.two_h2[:B]), labels=labels2)
        # the weighted set, smaller still
        used.set_kde_points(ks, kcls, kcnt, C2, hav)
        bits = used.kde_scale_bits
        assert bits == K.scale_bits(int(kcnt.sum())) > 0 and used.neighbor_points == M3
        got3 = _kde_outputs(used, krows, B, labels2, img2, **geometry)
        _equal(got3, want3, f"120 bins behind 300 points {geometry}")
        gap, own = krows.gaps()
        assert (np.minimum(gap, own) >= R.GAP_SWEEP).all()
        err = np.abs(got3[1] - K.fixed_sums(krows, kcls, kcnt, C2, bits)[:B]).astype(np.float64)
        assert (err <= K.layer2_units(krows, kcls, kcnt, C2, bits)[:B]).all()
        assert np.array_equal(got3[0], K.prior_from_sums(got3[1]))
        ranks = K.ranks_from_sums(got3[1], img2.cpu().numpy(), labels2.cpu().numpy())
        for g, w, name in zip(got3[2:], ranks, ("greater", "tied_after", "argmax")):
            assert np.array_equal(g, w), name
        # the count route that reads the word the counts now occupy refuses (range_neighbors.h)
        with pytest.raises(nn.RangeNativeError, match=f"error {INVALID}:"):
            used.neighbor_rank(None, dev(np.zeros(B), np.int32), nn.CELL, labels=labels2, pc=2.0, cpc=10.0)
        _equal(_kde_outputs(used, krows, B, labels2, img2, **geometry), want3, "the weighted set behind a refusal")
    used.set_neighbors(s2, cls2, C2, hav)
    assert used.kde_scale_bits == 0
    _equal(_neighbor_outputs(used, qd, labels2, img2, thr, k), want2, "300 points behind the weighted set")
    _same_retrieval(used, before, "the neighbour sets")


# -- the positional encoders' frequency tables ----------------------------------------------------------------------------
def test_posenc_tables_in_turn():
    """40 frequency tables one after the other on a context that keeps every table it has seen: prefixes of the
    models' own tables (different F, a common prefix), pairs equal in all but their last entry, the first again."""
    used = _used()
    before = _retrieval(used)
    q = np.ascontiguousarray(np.concatenate([np.array([[0.0, 0.0], [180.0, 90.0], [-180.0, -90.0]]),
                                             np.random.default_rng(3).uniform([-180, -90], [180, 90], (62, 2))]))
    qd = dev(q)
    tables = []
    for name in ("Theory", "s2vec_spherem"):
        f = np.asarray(posenc.freq_list(name), dtype=np.float64)
        for F in (1, 2, 3, 5, 8, len(f) - 1, len(f)):
            tables.append((name, f[:F].copy()))
            if F >= 2:
                g = f[:F].copy()
                g[-1] = f[0]                         # equal in its first F - 1 entries
                tables.append((name, g))
    tables = (tables * 2)[:39] + [tables[0]]
    assert len(tables) == 40
    fresh_out = {}
    for name, f in tables:
        key = (name, f.tobytes())
        if key not in fresh_out:                    # a context that sees this table alone
            fresh = _native.HipEngine(DEV)
            try:
                fresh_out[key] = fresh.posenc_features(qd, P.KINDS.index(P.KIND_OF_MODEL[name]), f).cpu().numpy()
            finally:
                fresh.close()
    for i, (name, f) in enumerate(tables):
        kind = P.KIND_OF_MODEL[name]
        got = used.posenc_features(qd, P.KINDS.index(kind), f).cpu().numpy()
        assert np.array_equal(got, fresh_out[(name, f.tobytes())], equal_nan=True), f"table {i} ({name}, F = {len(f)})"
        P.assert_close(kind, got, P.encode(kind, q, f))
    _same_retrieval(used, before, "the frequency tables")


# -- the checkerboard scan ------------------------------------------------------------------------------------------------
def test_nearest_support_shrinks():
    """10 000 supports over several chunks (their partial pairs stay in the workspace), then 7 supports."""
    used = _used()
    before = _retrieval(used)
    q = CK.random_points(257, 41)
    big, small = CK.random_points(10000, 42), CK.random_points(7, 43)
    qr = dev(np.radians(q))
    idx, dist = used.nearest_support(qr, dev(np.radians(big)), max_chunks=8)
    want_idx, want_dist = CK.nearest(q, big, chunks=8)
    ok = CK.relative_gap(q, big) >= CK.GAP_MIN
    assert ok.mean() > 0.99 and np.array_equal(idx.cpu().numpy()[ok], want_idx[ok])
    CK.assert_dist_close(dist.cpu().numpy(), want_dist)
    fresh = _native.HipEngine(DEV)
    try:
        f_idx, f_dist = fresh.nearest_support(qr, dev(np.radians(small)))
    finally:
        fresh.close()
    for max_chunks in (0, 8):
        idx, dist = used.nearest_support(qr, dev(np.radians(small)), max_chunks=max_chunks)
        assert torch.equal(idx, f_idx) and torch.equal(dist, f_dist)
        idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
        assert idx.min() >= 0 and idx.max() < 7
        want_idx, want_dist = CK.nearest(q, small)
        assert (CK.relative_gap(q, small) >= CK.GAP_MIN).all() and np.array_equal(idx, want_idx)
        CK.assert_dist_close(dist, want_dist)
    _same_retrieval(used, before, "the checkerboard scans")


# -- the probe context: map and cluster workspaces -------------------------------------------------------------------------
def test_probe_context_reserved_large_then_used_small():
    """range_map_reserve / range_cluster_reserve for a large problem, the large problem run, then a small one - under the
    large reservation and under its own: a fresh context's bits, within icamap_refs' / cluster_refs' bounds."""
    rng = np.random.default_rng(9)
    # the ICA step
    Yb, Wb = rng.standard_normal((8, 20000)), IM.sym_decorrelation(rng.standard_normal((8, 8)))
    Ys, Ws = rng.standard_normal((3, 300)), IM.sym_decorrelation(rng.standard_normal((3, 3)))
    fresh = _map_native.MapEngine(DEV)
    fresh.reserve(300, 3)
    want = fresh.ica_step(dev(Ys), Ws).cpu().numpy()
    fresh.close()
    A, b, bound_A, bound_b = IM.ica_step_ld(Ys, Ws)
    used = _map_native.MapEngine(DEV)
    try:
        used.reserve(20000, 8)
        used.ica_step(dev(Yb), Wb)
        for again in (False, True):
            if again:
                used.reserve(300, 3)
            got = used.ica_step(dev(Ys), Ws).cpu().numpy()
            assert np.array_equal(got, want), f"ica_step behind a larger problem (reserved again: {again})"
            assert (np.abs(got[:9].reshape(3, 3).astype(np.longdouble) - A) <= bound_A).all()
            assert (np.abs(got[9:].astype(np.longdouble) - b) <= bound_b).all()
    finally:
        used.close()
    # distances and the linkage
    nb, ns, d = 600, 70, 40
    Eb, Es = CL.normalize(rng.standard_normal((nb, d)))[0], CL.normalize(rng.standard_normal((ns, d)))[0]
    fresh = _cluster_native.ClusterEngine(DEV)
    fresh.reserve(ns, d)
    Dw = fresh.distances(dev(Es))
    want = [Dw.cpu().numpy()] + [t.cpu().numpy() if torch.is_tensor(t) else t for t in fresh.linkage(Dw.clone())]
    fresh.close()
    used = _cluster_native.ClusterEngine(DEV)
    try:
        used.reserve(nb, d)
        used.linkage(used.distances(dev(Eb)))
        for again in (False, True):
            if again:
                used.reserve(ns, d)
            D = used.distances(dev(Es))
            got = [D.cpu().numpy()] + [t.cpu().numpy() if torch.is_tensor(t) else t for t in used.linkage(D.clone())]
            for g, w in zip(got, want):
                assert np.array_equal(g, w), f"cluster map behind a larger problem (reserved again: {again})"
            off = ~np.eye(ns, dtype=bool)
            with np.errstate(invalid="ignore"):
                err = np.abs(got[0].astype(np.longdouble) - CL.distances_ld(Es))
            assert err[off].max() <= CL.dist_bound(d)
            ref = CL.linkage_rounds(got[0])           # the rounds of cluster_kernels.h on the kernel's own matrix
            assert np.array_equal(got[1], ref["merges"]) and np.array_equal(got[2], ref["heights"]) and got[3] == ref["rounds"]
    finally:
        used.close()
