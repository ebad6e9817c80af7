"""Cluster maps: complete-linkage clusters of a location encoder's embeddings, on the GPU.

Replaces the reference's location_models/csp/main/analysis.py:386-434 (``spa_enc_embed_clustering``): embed every
location, multiply the rows by an optional land mask and fill the zeros (:417-423), L2-normalise the rows (:425-426),
run ``AgglomerativeClustering(n_clusters, cosine, complete linkage)`` (:431) and shape the labels like the grid (:432).

Definition.  ``feats`` is (N, D).  (1) With a ``mask`` (N,), every row is multiplied by its mask value and sqrt(1/D)
is then added to every entry that equals 0, anywhere in the matrix (the reference fills only when it has a mask).
(2) e_i = x_i / |x_i|_2.  (3) d_ij = max(0, 1 - e_i . e_j) in float64.  (4) Complete linkage down to ``n_clusters``
clusters.  (5) Labels numbered by first occurrence: the cluster holding row 0 is 0, the next new cluster met going down
the rows is 1, and so on.  scikit-learn's own numbering follows the order of its heap and carries no meaning; the
partition is the same.

Everything that touches the N x D features or the N x N distances runs in HIP kernels (include/range_cluster.h and the
ridge probe's column sums and float64 GEMM); the stable sort of the N - 1 merges by height and the union-find of the
cut are host arithmetic.  There is no CPU fallback.

Masked rows (mask value 0) all become the same unit vector, so only the unmasked rows plus one representative - the
first masked row - are clustered, and every masked row takes the representative's label.  For ``n_clusters`` up to
the number of rows so clustered this is the partition that clustering all rows gives: coinciding rows merge first, at
height 0, and complete linkage then sees them as one point.

Deviation from the reference: float32 features are widened to float64 first."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .embedding_map import _device_of, check_finite_sums, embed_locations


def check_shape(n: int, d: int, n_clusters) -> None:
    """The refusals that need no data: N < 2, D < 1, n_clusters outside 1..N."""
    if n < 2:
        raise ValueError(f"clustering needs at least 2 rows, got {n}")
    if d < 1:
        raise ValueError("the features have no columns")
    if isinstance(n_clusters, bool) or not isinstance(n_clusters, (int, np.integer)) or not 1 <= n_clusters <= n:
        raise ValueError(f"n_clusters must be an integer in 1..{n}, got {n_clusters!r}")


def rows_to_cluster(mask: Optional[np.ndarray], n: int):
    """(idx, rep): the rows that are clustered - all of them, or with masked rows (mask == 0) the unmasked ones and
    the first masked one, ascending - and the position of that representative in ``idx`` (None without masked rows)."""
    if mask is None:
        return np.arange(n), None
    masked = mask == 0
    if not masked.any():
        return np.arange(n), None
    first = int(np.flatnonzero(masked)[0])
    keep = ~masked
    keep[first] = True
    idx = np.flatnonzero(keep)
    return idx, int(np.searchsorted(idx, first))


def _check_memory(dev: torch.device, n: int, d: int, resident: int) -> None:
    """Peak device memory: the n x n float64 distances, the float64 features and their normalised copy."""
    need = n * n * 8 + 2 * n * d * 8 + 64 * n - resident
    free, _ = torch.cuda.mem_get_info(dev)
    if need > free:
        raise ValueError(f"the cluster map of {n} x {d} features needs {need} more bytes of device memory (the "
                         f"{n} x {n} float64 distance matrix is {n * n * 8}), {free} bytes are free on {dev}")


def cluster_labels(feats, n_clusters: int, mask=None, device=None, return_info: bool = False):
    """The complete-linkage cosine clusters of ``feats`` (N, D) - a host array or a device tensor, float32 (widened
    to float64 first) or float64 - as (N,) int32 labels 0..n_clusters-1 numbered by first occurrence (see the module
    text; scikit-learn's numbering differs, the partition does not).  ``mask`` (N,): the reference's land mask, see
    the module text.

    ``return_info=True`` also returns a dict: ``linkage`` (scipy's Z of the rows that were clustered), ``heights``
    (its column 2), ``rounds`` (the linkage rounds on the device), ``n_clustered`` and ``rows`` (the indices of the
    clustered rows).  Refused with ``ValueError``: N < 2, ``n_clusters`` outside 1..N or beyond the distinct rows a
    mask leaves, a dtype other than float32 / float64, non-finite values (from the device's column sums), a row of
    zero norm (from the smallest squared norm; the first such row is named), a distance matrix that does not fit the
    free device memory (the bytes are named).  A non-GPU device raises ``RuntimeError``."""
    from ._cluster_native import MAX_ROWS, ClusterEngine, cut
    if not (isinstance(feats, (np.ndarray, torch.Tensor)) and feats.ndim == 2):
        raise ValueError("feats must be a 2-d array or tensor (N, D)")
    n, d = int(feats.shape[0]), int(feats.shape[1])
    check_shape(n, d, n_clusters)
    if feats.dtype not in (np.float32, np.float64, torch.float32, torch.float64):
        raise ValueError(f"feats must be float32 or float64, got {feats.dtype}")
    if mask is not None:
        mask = (mask.detach().cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask))
        mask = mask.astype(np.float64).reshape(-1)
        if mask.shape[0] != n:
            raise ValueError(f"mask must hold one value a row ({n}), got {mask.shape[0]}")
        if not np.isfinite(mask).all():
            raise ValueError("the mask holds non-finite values")
    idx, rep = rows_to_cluster(mask, n)
    m = len(idx)
    if n_clusters > m:
        raise ValueError(f"n_clusters={n_clusters} exceeds the {m} distinct rows the mask leaves ({n - m + 1} masked "
                         f"rows coincide)")
    if m > MAX_ROWS:
        raise ValueError(f"{m} rows to cluster: the distance matrix is limited to {MAX_ROWS} rows")
    dev = _device_of(feats, device)
    on_dev = isinstance(feats, torch.Tensor) and feats.device == dev and feats.dtype == torch.float64
    _check_memory(dev, m, d, m * d * 8 if on_dev and m == n else 0)
    eng = ClusterEngine(dev)
    try:
        with torch.cuda.device(dev):
            labels, info = _cluster(eng, dev, feats, d, idx, mask, int(n_clusters), cut)
    finally:
        eng.close()
    full = labels
    if m != n:
        full = np.full(n, labels[rep], dtype=np.int32)
        full[idx] = labels
    return (full, info) if return_info else full


def _cluster(eng, dev, feats, d, idx, mask, k, cut):
    """``cluster_labels`` behind its checks, on an open engine with ``dev`` current: the labels of the rows ``idx``."""
    m, n = len(idx), int(feats.shape[0])
    src = torch.as_tensor(feats)
    X = src.to(device=dev, dtype=torch.float64)
    if m != n:
        X = X[torch.from_numpy(idx).to(dev)]
    elif X.stride(1) != 1 or X.stride(0) < d:
        X = X.contiguous()
    own = m != n or X.data_ptr() != src.data_ptr()          # a copy of ours: normalised in place
    check_finite_sums(eng.colstats(X)[2].cpu().numpy())
    mask_dev = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask[idx])).to(dev)
    E, norm2 = eng.normalize(X, mask_dev, out=X if own else None)
    del X
    lo, hi = float(norm2.min()), float(norm2.max())
    if not lo > 0.0:
        row = int(idx[int(torch.nonzero(~(norm2 > 0.0))[0])])
        raise ValueError(f"row {row} has zero norm: a direction is needed for the cosine distance")
    if not np.isfinite(hi):
        row = int(idx[int(torch.nonzero(~torch.isfinite(norm2))[0])])
        raise ValueError(f"the squared norm of row {row} overflows float64")
    if m == 1:
        return np.zeros(1, dtype=np.int32), dict(linkage=np.empty((0, 4)), heights=np.empty(0), rounds=0,
                                                 n_clustered=1, rows=idx)
    eng.reserve(m, d)
    D = eng.distances(E)
    del E
    merges, heights, rounds = eng.linkage(D)
    del D
    labels, Z = cut(merges.cpu().numpy(), heights.cpu().numpy(), k)
    return labels, dict(linkage=Z, heights=Z[:, 2].copy(), rounds=rounds, n_clustered=m, rows=idx)


def cluster_map(model, locs, n_clusters: int, grid_size=None, mask=None, batch_size: int = 100000, **kw):
    """``cluster_labels`` of ``model``'s embeddings of ``locs`` (N, 2) (lon, lat), encoded as ``embedding_map`` encodes
    them (``embed_locations``).  With ``grid_size`` (H, W), H * W == N, the labels come back as (H, W) - the
    reference's ``cluster_labels`` image; ``mask`` may then be (H, W) too.  Keyword arguments go to
    ``cluster_labels``."""
    n = int(np.shape(locs)[0])
    if grid_size is not None:
        grid_size = (int(grid_size[0]), int(grid_size[1]))
        if grid_size[0] * grid_size[1] != n:
            raise ValueError(f"grid_size {grid_size} does not hold the {n} locations")
    if mask is not None and not isinstance(mask, torch.Tensor):
        mask = np.asarray(mask).reshape(-1)
    feats, kw["device"] = embed_locations(model, locs, batch_size, kw.get("device"))
    check_shape(n, int(feats.shape[1]), n_clusters)
    out = cluster_labels(feats, n_clusters, mask=mask, **kw)
    if grid_size is None:
        return out
    if isinstance(out, tuple):
        return out[0].reshape(grid_size), out[1]
    return out.reshape(grid_size)
