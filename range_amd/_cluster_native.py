"""ctypes binding of include/range_cluster.h (the cluster-map entry points of librange_hip.so).

``ClusterEngine`` is a ``ProbeEngine`` (same context, same helpers) with one method per ``range_cluster_*`` entry
point that takes a context; ``plan`` and ``cut`` need no GPU.  No arithmetic happens here; there is no CPU
fallback."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _probe_native
from ._native import RangeNativeError, _check  # noqa: F401
from ._probe_native import ProbeEngine

# every symbol include/range_cluster.h declares
SYMBOLS = (
    "range_cluster_plan", "range_cluster_reserve", "range_cluster_normalize", "range_cluster_distances",
    "range_cluster_linkage", "range_cluster_stage_times", "range_cluster_cut",
)
MAX_ROWS = 131072

_bound = False


def load_library() -> C.CDLL:
    global _bound
    lib = _probe_native.load_library()
    if _bound:
        return lib
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    lib.range_cluster_plan.argtypes = [i64, i32, i64, vp]
    lib.range_cluster_reserve.argtypes = [vp, i64, i32]
    lib.range_cluster_normalize.argtypes = [vp, vp, i64, i32, i64, vp, vp, i64, vp, i64, vp]
    lib.range_cluster_distances.argtypes = [vp, vp, i64, i32, i64, vp, i64, i64, vp]
    lib.range_cluster_linkage.argtypes = [vp, vp, i64, i64, vp, vp, vp, i64, vp]
    lib.range_cluster_stage_times.argtypes = [vp, vp]
    lib.range_cluster_cut.argtypes = [i64, vp, vp, i64, vp, vp]
    for name in SYMBOLS:
        getattr(lib, name)
    _bound = True
    return lib


def plan(n: int, d: int, max_grid: int = 0) -> Dict[str, int]:
    """The launch plan of n rows of d features (host_plan.h: cluster_plan); needs no GPU."""
    lib = load_library()
    out = np.zeros(8, dtype=np.int64)
    _check(lib, lib.range_cluster_plan(n, d, max_grid, out.ctypes.data))
    keys = ("matrix_bytes", "ws_bytes", "norm_grid", "fin_items", "fin_grid", "scan_grid", "chunks", "serial_rows")
    return dict(zip(keys, (int(v) for v in out)))


def cut(merges, heights, n_clusters: int, want_linkage: bool = True) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """(labels (n,) int32 numbered by first occurrence, Z (n - 1, 4) scipy's linkage matrix or None) from the merge
    record (n - 1, 2) / (n - 1,) of ``ClusterEngine.linkage`` (host_plan.h: cluster_cut); needs no GPU."""
    lib = load_library()
    merges = np.ascontiguousarray(merges, dtype=np.int32).reshape(-1, 2)
    heights = np.ascontiguousarray(heights, dtype=np.float64).reshape(-1)
    if merges.shape[0] != heights.shape[0]:
        raise ValueError(f"{merges.shape[0]} merges but {heights.shape[0]} heights")
    n = merges.shape[0] + 1
    labels = np.empty(n, dtype=np.int32)
    Z = np.empty((n - 1, 4), dtype=np.float64) if want_linkage else None
    _check(lib, lib.range_cluster_cut(n, merges.ctypes.data, heights.ctypes.data, int(n_clusters), labels.ctypes.data,
                                      None if Z is None else Z.ctypes.data))
    return labels, Z


class ClusterEngine(ProbeEngine):
    """One probe context on one GPU, with the cluster map's entry points."""

    def __init__(self, device: torch.device | int | str = 0):
        load_library()
        super().__init__(device)

    def reserve(self, n: int, d: int) -> None:
        _check(self.lib, self.lib.range_cluster_reserve(self._h, n, d))

    def normalize(self, X: torch.Tensor, mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                  max_grid: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """(E, norm2): E (n, d) = the rows of X (n, d) over their 2-norms, norm2 (n,) the squared norms; with ``mask``
        (n,) every row is multiplied by its mask value first and sqrt(1/d) added to the entries that are then zero.
        X and ``out`` may be row-strided views; ``out`` may be X."""
        ldx = self._ld(X, "normalize X")
        n, d = X.shape
        if mask is not None and tuple(self._chk(mask, torch.float64, 1).shape) != (n,):
            raise ValueError(f"normalize: mask must have shape ({n},), got {tuple(mask.shape)}")
        E = self.empty((n, d)) if out is None else out
        lde = self._ld(E, "normalize out")
        if tuple(E.shape) != (n, d):
            raise ValueError("normalize: out has the wrong shape")
        norm2 = self.empty(n)
        _check(self.lib, self.lib.range_cluster_normalize(self._h, X.data_ptr(), n, d, ldx, _probe_native._p(mask),
                                                          E.data_ptr(), lde, norm2.data_ptr(), max_grid,
                                                          self._stream()))
        return E, norm2

    def distances(self, E: torch.Tensor, out: Optional[torch.Tensor] = None, max_grid: int = 0) -> torch.Tensor:
        """D (n, n) = max(0, 1 - E E^T), symmetric bit for bit, +inf on the diagonal; needs ``reserve(n, d)``."""
        lde = self._ld(E, "distances E")
        n, d = E.shape
        D = self.empty((n, n)) if out is None else out
        ldd = self._ld(D, "distances out")
        if tuple(D.shape) != (n, n):
            raise ValueError("distances: out has the wrong shape")
        _check(self.lib, self.lib.range_cluster_distances(self._h, E.data_ptr(), n, d, lde, D.data_ptr(), ldd,
                                                          max_grid, self._stream()))
        return D

    def linkage(self, D: torch.Tensor, max_grid: int = 0) -> Tuple[torch.Tensor, torch.Tensor, int]:
        """(merges (n - 1, 2) int32, heights (n - 1,), rounds) of the symmetric distance matrix D (n, n), which is
        destroyed; the merges are in emission order (``cut`` sorts them).  Needs ``reserve(n, d)``."""
        ldd = self._ld(D, "linkage D")
        n = D.shape[0]
        if D.shape[1] != n:
            raise ValueError(f"linkage: D must be square, got {tuple(D.shape)}")
        merges = torch.empty((max(n - 1, 0), 2), dtype=torch.int32, device=self.device)
        heights = self.empty(max(n - 1, 0))
        rounds = C.c_int32(0)
        _check(self.lib, self.lib.range_cluster_linkage(self._h, D.data_ptr(), n, ldd, merges.data_ptr(),
                                                        heights.data_ptr(), C.addressof(rounds), max_grid,
                                                        self._stream()))
        return merges, heights, int(rounds.value)

    def stage_times(self) -> Tuple[float, float]:
        """Host-clock milliseconds of the last ``linkage``: (the first round, i.e. the scan of all rows; the rest)."""
        out = np.zeros(2, dtype=np.float64)
        _check(self.lib, self.lib.range_cluster_stage_times(self._h, out.ctypes.data))
        return float(out[0]), float(out[1])
