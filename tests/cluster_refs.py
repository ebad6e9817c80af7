"""References of the cluster map for tests/test_cluster_cpu.py and tests/test_gpu_cluster.py (not a test module):
long-double references of the normaliser and the distances with their bounds, a numpy restatement of the linkage
rounds (the scheme of range_amd/csrc/cluster_kernels.h, with defects that can be planted), the cut, the replay
property, and the generators of the test matrices.

Bounds, from any-order summation (u = 2^-53; a sum of m terms formed in any order by m - 1 roundings, every product
one more, is within m u sum|terms| of the exact sum to first order).

* Normalised entries, (D + 4) u relative.  y = x * mask: u.  |y|^2 is a sum of D squares: D u relative, so its root
  carries D u / 2 and a rounding of its own, u; the quotient another u.  Together (D / 2 + 3) u <= (D + 4) u, the rest
  covers the second-order terms.
* Distances from given unit rows E, (D + 8) u absolute.  s = e_i . e_j is a sum of D products:
  D u sum|e_ik e_jk| <= D u |e_i| |e_j| (Cauchy-Schwarz), and |e_i| |e_j| <= 1 + (D + 4) u for rows normalised in
  float64.  d = 1 - s rounds once more: u |d| <= 2 u.  Together (D + 2) u (1 + ...) <= (D + 8) u.  Clamping at 0 and
  mirroring are exact.
"""
from __future__ import annotations

import numpy as np

L = np.longdouble
U = 2.0 ** -53
DEFECTS = ("mean", "min", "no_phase_b", "no_refresh", "emission_order")


def dist_bound(d: int) -> float:
    return (d + 8) * U


def norm_bound(d: int) -> float:
    return (d + 4) * U


def norm2_bound(d: int) -> float:
    """Relative, of the squared norm: y = x * mask carries u, so y^2 carries 2 u and its own rounding, 3 u a term;
    the D - 1 additions (D - 1) u: (D + 2) u to first order, one more u for the rest."""
    return (d + 3) * U


# ---- the definition ------------------------------------------------------------------------------------------------
def fill_value(d: int) -> float:
    return float(np.sqrt(1.0 / d))


def masked_features(X, mask, dtype=np.float64):
    """Step 1 of the definition: rows times their mask value, then sqrt(1/D) on every entry that equals 0 (only with
    a mask)."""
    Y = np.asarray(X).astype(dtype)
    if mask is not None:
        Y = Y * np.asarray(mask).astype(dtype)[:, None]
        Y[Y == 0] += dtype(fill_value(Y.shape[1]))
    return Y


def normalize_ld(X, mask=None):
    """(E, norm2) in long double."""
    Y = masked_features(X, mask, L)
    n2 = (Y * Y).sum(axis=1)
    return Y / np.sqrt(n2)[:, None], n2


def normalize(X, mask=None):
    """(E, norm2) in float64 numpy."""
    Y = masked_features(X, mask, np.float64)
    n2 = np.einsum("ij,ij->i", Y, Y)
    return Y / np.sqrt(n2)[:, None], n2


def distances_ld(E):
    """max(0, 1 - E E^T) in long double, +inf on the diagonal."""
    El = np.asarray(E).astype(L)
    D = np.maximum(L(0), L(1) - np.dot(El, El.T))
    np.fill_diagonal(D, np.inf)
    return D


def distances(E):
    """The float64 numpy distances: the lower triangle of max(0, 1 - E E^T) mirrored, +inf on the diagonal."""
    E = np.ascontiguousarray(E, dtype=np.float64)
    D = np.tril(np.maximum(0.0, 1.0 - np.dot(E, E.T)), -1)
    D = D + D.T
    np.fill_diagonal(D, np.inf)
    return D


def smallest_gap(D) -> float:
    """The smallest difference between two distinct entries below the diagonal."""
    v = np.unique(np.asarray(D)[np.tril_indices(D.shape[0], -1)])
    return float(np.diff(v).min()) if len(v) > 1 else float("inf")


# ---- the rounds ----------------------------------------------------------------------------------------------------
def linkage_rounds(D, defect=None):
    """The rounds of cluster_kernels.h on a symmetric matrix: dict(merges (n - 1, 2) and heights (n - 1) in emission
    order, rounds, scans = rows scanned in all).  defect: one of DEFECTS (``emission_order`` belongs to ``cut``)."""
    D = np.array(D, dtype=np.float64)
    n = D.shape[0]
    np.fill_diagonal(D, np.inf)
    join = {"mean": lambda a, b: (a + b) / 2.0, "min": np.minimum}.get(defect, np.maximum)
    active, stale = np.ones(n, bool), np.ones(n, bool)
    nn, nnd = np.full(n, -1), np.zeros(n)
    merges, heights, rounds, scans = [], [], 0, 0
    while len(merges) < n - 1:
        rows = np.flatnonzero(stale & active)                              # (a)
        act = np.flatnonzero(active)
        for i in rows:                                                     # (b): (distance, then lower index)
            cand = act[act != i]
            k = cand[np.argmin(D[i, cand])]
            nn[i], nnd[i] = k, D[i, k]
        scans += len(rows)
        stale[:] = False
        I = np.array([i for i in act if nn[nn[i]] == i and i < nn[i]], dtype=np.int64)     # (c), ascending
        assert len(I) > 0, "a round without a reciprocal pair"
        J = nn[I]
        merges += list(zip(I.tolist(), J.tolist()))
        heights += nnd[I].tolist()
        D[I] = join(D[I], D[J])                                            # (d) A
        if defect != "no_phase_b":
            D[np.ix_(I, I)] = join(D[np.ix_(I, I)], D[np.ix_(I, J)])       # B (the own pair lands on the diagonal)
        D[:, I] = D[I].T                                                   # C
        np.fill_diagonal(D, np.inf)
        active[J] = False                                                  # (e)
        stale[I] = True
        if defect != "no_refresh":
            touched = np.zeros(n, bool)
            touched[I] = touched[J] = True
            stale |= active & touched[nn]
        rounds += 1
        assert rounds <= n - 1
    return dict(merges=np.array(merges, dtype=np.int32).reshape(-1, 2), heights=np.array(heights, dtype=np.float64),
                rounds=rounds, scans=scans)


def cut(merges, heights, k, emission_order=False):
    """(labels by first occurrence, Z): host_plan.h's cluster_cut in Python.  emission_order: the planted defect -
    the first n - k merges as emitted, not as sorted."""
    m = len(heights)
    n = m + 1
    order = np.arange(m) if emission_order else np.argsort(heights, kind="stable")
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    ident, size = list(range(n)), [1] * n
    Z = np.zeros((m, 4))
    labels = None

    def number():
        seen = {}
        return np.array([seen.setdefault(find(i), len(seen)) for i in range(n)], dtype=np.int32)

    if n - k == 0:
        labels = number()
    for s, t in enumerate(order):
        ra, rb = find(int(merges[t][0])), find(int(merges[t][1]))
        assert ra != rb
        Z[s] = (min(ident[ra], ident[rb]), max(ident[ra], ident[rb]), heights[t], size[ra] + size[rb])
        parent[rb] = ra
        size[ra] += size[rb]
        ident[ra] = n + s
        if s + 1 == n - k:
            labels = number()
    return labels, Z


def first_occurrence(labels):
    """Any labelling renumbered by first occurrence."""
    seen = {}
    return np.array([seen.setdefault(int(v), len(seen)) for v in np.asarray(labels).reshape(-1)], dtype=np.int32)


def replay(D, merges, heights):
    """The replay property: the merges, sorted stably by height, applied to a complete-linkage matrix kept here.
    Every merged pair must be two current clusters (named by their lowest rows) and its height must be the matrix
    entry, bit for bit.  Returns the largest excess of a merged entry over the global minimum of its moment."""
    D = np.array(D, dtype=np.float64)
    n = D.shape[0]
    np.fill_diagonal(D, np.inf)
    active = np.ones(n, bool)
    excess = 0.0
    for t in np.argsort(heights, kind="stable"):
        i, j = int(merges[t][0]), int(merges[t][1])
        assert i != j and active[i] and active[j], f"merge {t}: ({i}, {j}) are not two current clusters"
        assert heights[t] == D[i, j], f"merge {t}: height {heights[t]!r} is not the entry {D[i, j]!r}"
        act = np.flatnonzero(active)
        excess = max(excess, float(D[i, j] - D[np.ix_(act, act)].min()))
        D[i] = np.maximum(D[i], D[j])
        D[:, i] = D[i]
        D[i, i] = np.inf
        active[j] = False
    assert active.sum() == 1
    return excess


# ---- test matrices -------------------------------------------------------------------------------------------------
def permutation_matrix(n, seed=0):
    """Symmetric, distinct integers: a random permutation of 1..n(n-1)/2 below the diagonal; 0 on it."""
    rng = np.random.default_rng(1000 + 7 * n + seed)
    D = np.zeros((n, n))
    il = np.tril_indices(n, -1)
    D[il] = rng.permutation(n * (n - 1) // 2) + 1.0
    return D + D.T


def line_matrix(n=40):
    """Points 2^0 .. 2^(n-1) on a line, d = |p_i - p_j| (exact in float64): one pair merges a round."""
    p = 2.0 ** np.arange(n)
    return np.abs(p[:, None] - p[None, :])


def tie_matrix(n, seed=0):
    """Symmetric with entries in 1..5: ties everywhere."""
    rng = np.random.default_rng(2000 + n + seed)
    D = np.zeros((n, n))
    il = np.tril_indices(n, -1)
    D[il] = rng.integers(1, 6, len(il[0])).astype(np.float64)
    return D + D.T


def scipy_heights(D):
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import squareform
    M = np.array(D, dtype=np.float64)
    np.fill_diagonal(M, 0.0)
    return linkage(squareform(M, checks=False), "complete")[:, 2]


def smooth_grid_features(rows, cols, d, seed):
    """A smooth field on a rows x cols lon/lat grid (lon end point excluded: no two rows coincide): sin(P W + b) of
    the unit vectors P."""
    lon = np.radians(np.linspace(-180, 180, cols, endpoint=False))
    lat = np.radians(np.linspace(80, -80, rows))
    lon, lat = np.meshgrid(lon, lat)
    lon, lat = lon.reshape(-1), lat.reshape(-1)
    P = np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], axis=1)
    rng = np.random.default_rng(seed)
    return np.sin(np.dot(P, 1.5 * rng.standard_normal((3, d))) + rng.uniform(0, 2 * np.pi, d))
