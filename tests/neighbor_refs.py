"""The numpy restatement of the neighbour and grid geo priors (range_amd/csrc/neighbor_kernel.h,
range_amd/geo_baselines.py): reduced distances in scikit-learn's expression order, the three membership predicates,
the total order (red, then index) of the k nearest, the two prior formulas, and ``csp_eval.rank_counts`` for the
ranks.  tests/test_neighbors_cpu.py pins it, bit for bit, to what the reference's own functions gave
(tests/golden/neighbor_priors.npz); the GPU tests compare the kernels with it.  numpy only.

Locations: (lon, lat) DEGREES at this level, as ``geo_baselines`` takes them; ``metric_locs`` converts to what the
metric works on (radians for haversine), as trainer.py does before it builds the BallTree."""
from __future__ import annotations

import numpy as np

from range_amd import csp_eval
from range_amd import geo_baselines as gb

GAP_FIXTURE = 1e-9            # the fixture's condition (make_golden_neighbors.py)
GAP_SWEEP = 2.0 ** -40        # random sweeps leave out queries nearer than this (relative) to a threshold
# the random sweeps of tests/test_gpu_neighbors.py: (seed, N) with SWEEP_B queries each; tests/test_neighbors_cpu.py
# asserts that they leave out no query
SWEEP_SEEDS = ((101, 1), (102, 255), (103, 256), (104, 257), (105, 1000))
SWEEP_B = 25                  # 3 G + 1 at the largest G
SWEEP_KS = (1, 2, 64)         # and N
SWEEP_THRESH = {True: 0.12, False: 7.0}


def sweep_points(seed: int, N: int):
    s = random_locs(N, seed)
    return s, queries_near(s, SWEEP_B, seed + 50)


def metric_locs(locs_deg, haversine: bool) -> np.ndarray:
    locs = np.asarray(locs_deg, dtype=np.float64).reshape(-1, 2)
    return np.deg2rad(locs) if haversine else locs


def red_matrix(q, s, haversine: bool) -> np.ndarray:
    """(B, N) reduced distances of metric-space (lon, lat) rows ``q`` against ``s``."""
    lon1, lat1 = q[:, 0][:, None], q[:, 1][:, None]
    lon2, lat2 = s[:, 0][None, :], s[:, 1][None, :]
    with np.errstate(invalid="ignore"):
        if haversine:
            s0 = np.sin(0.5 * (lat1 - lat2))
            s1 = np.sin(0.5 * (lon1 - lon2))
            return s0 * s0 + np.cos(lat1) * np.cos(lat2) * s1 * s1
        dlat, dlon = lat1 - lat2, lon1 - lon2
        return dlat * dlat + dlon * dlon


def members_radius(red, thr: float, strict: bool = False) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return red < thr if strict else red <= thr


def select_kth(red, k: int):
    """Per row the k-th smallest pair under (red, index) among the pairs with a number for red: (red_k (B,) float64,
    j_last (B,) int64); (NaN, -1) for a row with fewer than k."""
    B, N = red.shape
    red_k, j_last = np.full(B, np.nan), np.full(B, -1, dtype=np.int64)
    for i in range(B):
        valid = np.flatnonzero(~np.isnan(red[i]))
        if len(valid) < k:
            continue
        order = valid[np.lexsort((valid, red[i, valid]))]
        red_k[i], j_last[i] = red[i, order[k - 1]], order[k - 1]
    return red_k, j_last


def members_knn(red, k: int) -> np.ndarray:
    red_k, j_last = select_kth(red, k)
    j = np.arange(red.shape[1])[None, :]
    with np.errstate(invalid="ignore"):
        m = (red < red_k[:, None]) | ((red == red_k[:, None]) & (j <= j_last[:, None]))
    short = np.isnan(red_k)
    m[short] = ~np.isnan(red[short])
    return m


def counts_of(members, classes, num_classes: int) -> np.ndarray:
    out = np.zeros((members.shape[0], num_classes), dtype=np.int32)
    cls = np.asarray(classes)
    for i in range(members.shape[0]):
        out[i] = np.bincount(cls[members[i]], minlength=num_classes)
    return out


def prior_neighbors(cnt) -> np.ndarray:
    c = cnt.astype(np.float64)
    return (1.0 + c) / (1.0 + c).sum(axis=1, keepdims=True)


def prior_grid(cnt, qcell, pseudo_count, off_by: int = 0) -> np.ndarray:
    C = cnt.shape[1]
    c = cnt.astype(np.float64)
    den = c.sum(axis=1, keepdims=True) + (C * pseudo_count) - C
    with np.errstate(invalid="ignore", divide="ignore"):
        p = ((c + (pseudo_count + off_by)) - 1) / den
    p[np.asarray(qcell) == -1] = (np.ones(C) / np.ones(C).sum())
    return p


def neighbor_counts(q_deg, s_deg, classes, num_classes, haversine, ptype, dist_thresh=None, k=None):
    red = red_matrix(metric_locs(q_deg, haversine), metric_locs(s_deg, haversine), haversine)
    m = members_radius(red, gb.radius_threshold(dist_thresh, haversine)) if ptype == "distance" else members_knn(red, k)
    return counts_of(m, classes, num_classes), m, red


def grid_counts(q_deg, s_deg, classes, num_classes, gp_size):
    qc = gb.query_cells(q_deg, gp_size[0], gp_size[1])
    sc = gb.train_cells(s_deg, gp_size[0], gp_size[1])
    m = qc[:, None] == sc[None, :]
    return counts_of(m, classes, num_classes), qc


def scores(prior, img) -> np.ndarray:
    return prior if img is None else np.asarray(img).astype(np.float64) * prior


def ranks(prior, img, labels):
    """(greater, tied_after, argmax) of csp_eval.rank_counts on the scores."""
    return csp_eval.rank_counts(scores(prior, img), labels)


def threshold_gap(red, thr: float) -> np.ndarray:
    """Per row the smallest relative distance of a pair's red from the radius threshold (inf without pairs)."""
    with np.errstate(invalid="ignore"):
        g = np.abs(red - thr) / max(abs(thr), np.finfo(np.float64).tiny)
    g = np.where(np.isnan(g), np.inf, g)
    return g.min(axis=1) if red.shape[1] else np.full(red.shape[0], np.inf)


def knn_gap(red, k: int) -> np.ndarray:
    """Per row the relative gap between the k-th and the (k+1)-th reduced distance; inf where there is no (k+1)-th, for
    a row with fewer than k pairs, and where the two are EQUAL (exact duplicates tie on every device: the index
    decides)."""
    B, N = red.shape
    out = np.full(B, np.inf)
    for i in range(B):
        v = np.sort(red[i][~np.isnan(red[i])])
        if len(v) > k and v[k] != v[k - 1]:
            out[i] = (v[k] - v[k - 1]) / max(abs(v[k]), np.finfo(np.float64).tiny)
    return out


class NumpyNeighborPrior:
    """A stand-in for geo_baselines.NeighborPrior / GridPrior on the host: ``label_ranks`` from the restatement."""

    def __init__(self, s_deg, classes, num_classes, hyper_params, grid: bool = False):
        self.s, self.classes, self.C, self.hp, self.grid = np.asarray(s_deg, dtype=np.float64), np.asarray(classes), num_classes, hyper_params, grid
        self.calls = 0

    def prior(self, locs, ptype=None):
        if self.grid:
            cnt, qc = grid_counts(locs, self.s, self.classes, self.C, self.hp["gp_size"])
            return prior_grid(cnt, qc, self.hp["pseudo_count"])
        hav = self.hp["dist_type"] == "haversine"
        cnt, _, _ = neighbor_counts(locs, self.s, self.classes, self.C, hav, ptype, self.hp.get("dist_thresh"),
                                    self.hp.get("num_neighbors"))
        return prior_neighbors(cnt)

    def label_ranks(self, locs, labels, preds=None, ptype=None):
        self.calls += 1
        g, e, am = ranks(self.prior(np.asarray(locs, dtype=np.float64), ptype), preds, labels)
        if (g == -2).any():
            raise ValueError("labels outside the classes of the prior")
        ok = g >= 0
        return np.where(ok, 1 + g.astype(np.int64) + e, 0), np.where(ok, am, -1).astype(np.int64)


def random_locs(n: int, seed: int, blobs: int = 6) -> np.ndarray:
    """n (lon, lat) degrees clustered on a few blobs, so that radius and cell sets are neither empty nor everything."""
    rng = np.random.default_rng(seed)
    centres = np.stack([rng.uniform(-150, 150, blobs), rng.uniform(-60, 60, blobs)], 1)
    pts = centres[rng.integers(0, blobs, n)] + rng.normal(0, 6.0, (n, 2))
    pts[:, 0] = np.clip(pts[:, 0], -179.9, 179.9)
    pts[:, 1] = np.clip(pts[:, 1], -89.9, 89.9)
    return pts


def queries_near(s_deg, n: int, seed: int, spread: float = 3.0) -> np.ndarray:
    """n queries scattered around randomly chosen training points."""
    rng = np.random.default_rng(seed)
    q = np.asarray(s_deg)[rng.integers(0, len(s_deg), n)] + rng.normal(0, spread, (n, 2))
    q[:, 0] = np.clip(q[:, 0], -179.9, 179.9)
    q[:, 1] = np.clip(q[:, 1], -89.9, 89.9)
    return q
