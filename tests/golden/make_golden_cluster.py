#!/usr/bin/env python3
"""Golden vectors of the cluster map (range_amd/cluster_map.py), generated on the CPU in the development container
with the installed scikit-learn and scipy (never on the GPU box):

    python tests/golden/make_golden_cluster.py

``cluster_map.npz`` holds, per case C (features are float32 so that the file stays small; every consumer widens
them to float64 first, exactly):

* ``C_X`` the features, and for ``masked`` the mask ``masked_mask`` (1 land, 0 ocean);
  ``rand``: 300 x 16 Gaussian; ``grid``: a smooth field on a 13 x 24 lon/lat grid, D = 16, the lon end point
  excluded so that no two rows coincide (tests/cluster_refs.py: smooth_grid_features); ``masked``: the grid with about
  60 % of its rows masked and a few zeros planted in unmasked rows;
* ``C_k{K}`` for K in 1, 2, 8, 17, N: the partition of
  ``AgglomerativeClustering(n_clusters=K, metric="cosine", linkage="complete").fit(E).labels_`` renumbered by first
  occurrence, E being the rows after the mask, the zero fill and the L2 normalisation in float64 numpy - for
  ``masked`` on ALL rows, coinciding ones included.  The reference's own call (analysis.py:431) passes ``affinity=``,
  which this scikit-learn rejects, so its function cannot be run as is: this is the same estimator with the
  keyword's present name;
* ``C_heights``: ``scipy.cluster.hierarchy.linkage(squareform(D), "complete")[:, 2]`` of the float64 numpy distances
  D = max(0, 1 - E E^T) (tests/cluster_refs.py: distances) of the rows that get clustered (for ``masked``: the
  unmasked rows and the first masked one), and ``C_gap``: the smallest gap between two distinct entries of D;
* ``versions``: the libraries.

Condition asserted on every case (on the input, not a tolerance): the smallest gap exceeds twice the distance bound
(D + 8) 2^-53 - then every computation of the distances within the bound orders them alike, and the partitions are
exact.  The seed of ``grid`` is the first that holds it."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cluster_refs as R  # noqa: E402

KS = (1, 2, 8, 17)
GRID = (13, 24)


def partitions(E):
    from sklearn.cluster import AgglomerativeClustering
    n = E.shape[0]
    return {k: R.first_occurrence(AgglomerativeClustering(n_clusters=k, metric="cosine", linkage="complete")
                                  .fit(E).labels_) for k in KS + (n,)}


def case(X, mask=None):
    """X float32.  (partitions on all rows, heights and gap on the rows that get clustered)"""
    E = R.normalize(X.astype(np.float64), mask)[0]
    rows = np.arange(len(X))
    if mask is not None:
        keep = mask != 0
        keep[np.flatnonzero(mask == 0)[0]] = True
        rows = np.flatnonzero(keep)
    D = R.distances(E[rows])
    return partitions(E), R.scipy_heights(D), R.smallest_gap(D)


def main():
    import scipy
    import sklearn
    gold = {"versions": np.array([f"numpy {np.__version__}", f"scipy {scipy.__version__}",
                                  f"scikit-learn {sklearn.__version__}"])}
    d = 16
    need = 2 * R.dist_bound(d)
    cases = {"rand": (np.random.default_rng(300).standard_normal((300, d)).astype(np.float32), None)}
    for seed in range(100):
        X = R.smooth_grid_features(GRID[0], GRID[1], d, seed).astype(np.float32)
        land = X[:, 0].astype(np.float64) + 0.3 * X[:, 1] > np.quantile(X[:, 0] + 0.3 * X[:, 1], 0.6)
        mask = land.astype(np.float64)
        Xm = X.copy()
        unmasked = np.flatnonzero(land)
        Xm[unmasked[3], 5] = Xm[unmasked[3], 9] = Xm[unmasked[40], 0] = 0.0
        if case(X)[2] > need and case(Xm, mask)[2] > need:
            print(f"grid: seed {seed}")
            cases["grid"], cases["masked"] = (X, None), (Xm, mask)
            break
    for name, (X, mask) in cases.items():
        parts, heights, gap = case(X, mask)
        assert gap > need, (name, gap, need)
        gold[name + "_X"] = X
        if mask is not None:
            gold[name + "_mask"] = mask
        for k, lab in parts.items():
            assert len(np.unique(lab)) == k
            gold[f"{name}_k{k}"] = lab
        gold[name + "_heights"], gold[name + "_gap"] = heights, gap
        print(f"{name}: {X.shape}, {len(heights) + 1} rows clustered, smallest gap {gap:.2e} against 2 x bound {need:.2e}")
    path = os.path.join(HERE, "cluster_map.npz")
    np.savez_compressed(path, **gold)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()
