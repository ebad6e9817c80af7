"""ctypes binding of include/range_neighbors.h (the neighbour / grid geo priors of librange_hip.so).

``NeighborEngine`` is a ``HipEngine`` (same context, same helpers) that owns one installed training set, with one
method per ``range_neighbor_*`` entry point.  No arithmetic happens here; there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _native
from ._native import CSP_IMG_F32, CSP_IMG_F64, CSP_IMG_NONE, HipEngine, RangeNativeError, _check, _ptr  # noqa: F401

# every symbol include/range_neighbors.h declares
SYMBOLS = (
    "range_neighbor_plan", "range_set_neighbors", "range_neighbor_points", "range_neighbor_classes",
    "range_neighbor_select", "range_neighbor_select_grid", "range_neighbor_rank", "range_neighbor_rank_grid",
    "range_neighbor_prior", "range_neighbor_prior_grid",
)
#: the KDE prior's entry points in the same header
KDE_SYMBOLS = (
    "range_kde_plan", "range_set_kde_points", "range_kde_scale_bits", "range_kde_rank", "range_kde_rank_grid",
    "range_kde_prior", "range_kde_prior_grid",
)
RADIUS, KNN, CELL = 0, 1, 2
MAX_CLASSES = 32768
KDE_MAX_CLASSES = 16384
CELL_UNIFORM, CELL_OUTSIDE = -1, -2      # a query that takes the uniform prior; a training point that never votes

_bound = False


def load_library() -> C.CDLL:
    global _bound
    lib = _native.load_library()
    if _bound:
        return lib
    vp, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    pred = [i32, i64, f64, f64, f64]                    # mode, k, thr, pc, cpc
    lib.range_neighbor_plan.argtypes = [i64, i64, i32, i64, i64, i32, vp]
    lib.range_set_neighbors.argtypes = [vp, vp, vp, vp, i64, i32, i32]
    lib.range_neighbor_points.argtypes = [vp]
    lib.range_neighbor_points.restype = i64
    lib.range_neighbor_classes.argtypes = [vp]
    lib.range_neighbor_classes.restype = i32
    lib.range_neighbor_select.argtypes = [vp, vp, i64, i64, vp, vp, vp]
    lib.range_neighbor_select_grid.argtypes = [vp, vp, i64, i64, vp, vp, i64, vp]
    lib.range_neighbor_rank.argtypes = [vp, vp, vp, i64] + pred + [vp, i32, vp, vp, vp, vp, vp]
    lib.range_neighbor_rank_grid.argtypes = [vp, vp, vp, i64] + pred + [vp, i32, vp, vp, vp, vp, i64, i32, vp]
    lib.range_neighbor_prior.argtypes = [vp, vp, vp, i64] + pred + [vp, vp]
    lib.range_neighbor_prior_grid.argtypes = [vp, vp, vp, i64] + pred + [vp, vp, i64, i32, vp]
    kde = [vp, vp, vp, vp, i64]                         # ctx, q, thr, two_h2, B
    lib.range_kde_plan.argtypes = [i64, i64, i32, i64, i64, i32, vp]
    lib.range_set_kde_points.argtypes = [vp, vp, vp, vp, i64, i32, i32]
    lib.range_kde_scale_bits.argtypes = [vp]
    lib.range_kde_scale_bits.restype = i32
    lib.range_kde_rank.argtypes = kde + [vp, i32, vp, vp, vp, vp, vp]
    lib.range_kde_rank_grid.argtypes = kde + [vp, i32, vp, vp, vp, vp, i64, i32, vp]
    lib.range_kde_prior.argtypes = kde + [vp, vp]
    lib.range_kde_prior_grid.argtypes = kde + [vp, vp, i64, i32, vp]
    for name in SYMBOLS + KDE_SYMBOLS:
        getattr(lib, name)
    _bound = True
    return lib


def _plan(entry: str, args: Tuple[int, ...], own_keys: Tuple[str, str]) -> Dict[str, int]:
    lib = load_library()
    out = np.zeros(8, dtype=np.int64)
    _check(lib, getattr(lib, entry)(*args, out.ctypes.data))
    keys = ("group", "groups", "grid", "chunks", "lds_bytes", "ws_bytes") + own_keys
    return dict(zip(keys, (int(v) for v in out)))


def plan(B: int, N: int, num_classes: int, k: int = 0, max_grid: int = 0, chunks: int = 0) -> Dict[str, int]:
    """The launch plan (host_plan.h: neighbor_plan); needs no GPU."""
    return _plan("range_neighbor_plan", (B, N, num_classes, k, max_grid, chunks), ("digit_bits", "passes"))


def kde_plan(B: int, M: int, num_classes: int, total_count: int, max_grid: int = 0, chunks: int = 0) -> Dict[str, int]:
    """The KDE prior's launch plan (host_plan.h: kde_plan); needs no GPU."""
    return _plan("range_kde_plan", (B, M, num_classes, total_count, max_grid, chunks), ("scale_bits", "tiles"))


class NeighborEngine(HipEngine):
    """One context on one GPU with one training set of the neighbour / grid priors installed."""

    def __init__(self, device: torch.device | int | str = 0):
        load_library()
        super().__init__(device)
        self.haversine = False

    def set_neighbors(self, lonlat: np.ndarray, classes: np.ndarray, num_classes: int, haversine: bool,
                      cells: Optional[np.ndarray] = None) -> None:
        """``lonlat`` (N, 2) float64 (lon, lat) - radians with ``haversine``, else degrees -, ``classes`` (N,) in
        ``[0, num_classes)``, ``cells`` (N,) int32 grid cells (< 0: none) or None: host arrays."""
        ll = np.ascontiguousarray(lonlat, dtype=np.float64)
        cls = np.ascontiguousarray(classes, dtype=np.int32)
        if ll.ndim != 2 or ll.shape[1] != 2 or cls.shape != (ll.shape[0],):
            raise ValueError(f"lonlat (N, 2) and classes (N,), got {ll.shape} and {cls.shape}")
        cell = None
        if cells is not None:
            cell = np.ascontiguousarray(cells, dtype=np.int32)
            if cell.shape != cls.shape:
                raise ValueError(f"cells (N,), got {cell.shape}")
        _check(self.lib, self.lib.range_set_neighbors(self._h, ll.ctypes.data, cls.ctypes.data,
                                                      None if cell is None else cell.ctypes.data, ll.shape[0],
                                                      int(num_classes), int(bool(haversine))))
        self.haversine = bool(haversine)

    @property
    def neighbor_points(self) -> int:
        return int(self.lib.range_neighbor_points(self._h))

    @property
    def neighbor_classes(self) -> int:
        return int(self.lib.range_neighbor_classes(self._h))

    def neighbor_select(self, q: torch.Tensor, k: int, max_grid: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """(``red_k`` (B,) float64, ``j_last`` (B,) int64) of ``q`` (B, 2) float64 (range_neighbor_select)."""
        self._t(q, torch.float64, (2,))
        B = q.shape[0]
        red_k, j_last = self._empty((B,), torch.float64), self._empty((B,), torch.int64)
        if B:
            _check(self.lib, self.lib.range_neighbor_select_grid(self._h, q.data_ptr(), B, int(k), red_k.data_ptr(),
                                                                 j_last.data_ptr(), int(max_grid), self._stream()))
        return red_k, j_last

    def _queries(self, q: Optional[torch.Tensor], qcell: Optional[torch.Tensor], mode: int) -> int:
        if (qcell if mode == CELL else q) is None:
            raise ValueError("the cell predicate takes qcell, the others q")
        if mode == CELL:
            self._t(qcell, torch.int32, ())
            return qcell.shape[0]
        self._t(q, torch.float64, (2,))
        return q.shape[0]

    def neighbor_rank(self, q: Optional[torch.Tensor], qcell: Optional[torch.Tensor], mode: int, labels: torch.Tensor,
                      img: Optional[torch.Tensor] = None, k: int = 0, thr: float = 0.0, pc: float = 0.0, cpc: float = 0.0,
                      max_grid: int = 0, chunks: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(``greater``, ``tied_after``, ``argmax``), (B,) int32 each, as ``HipEngine.csp_rank`` gives them, over
        the scores ``img.double() * prior`` (range_neighbor_rank_grid)."""
        B = self._queries(q, qcell, mode)
        kind, out = self._rank_args(B, self.neighbor_classes, img, labels)
        if B:
            _check(self.lib, self.lib.range_neighbor_rank_grid(
                self._h, _ptr(q), _ptr(qcell), B, mode, int(k), float(thr), float(pc), float(cpc), _ptr(img), kind,
                labels.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), int(max_grid), int(chunks),
                self._stream()))
        return out

    def neighbor_prior(self, q: Optional[torch.Tensor], qcell: Optional[torch.Tensor], mode: int, k: int = 0,
                       thr: float = 0.0, pc: float = 0.0, cpc: float = 0.0, want_counts: bool = False,
                       max_grid: int = 0, chunks: int = 0):
        """The (B, num_classes) float64 priors (range_neighbor_prior_grid); with ``want_counts`` also the int32 votes."""
        B = self._queries(q, qcell, mode)
        C_ = self.neighbor_classes
        prior = self._empty((B, C_), torch.float64)
        counts = self._empty((B, C_), torch.int32) if want_counts else None
        if B:
            _check(self.lib, self.lib.range_neighbor_prior_grid(
                self._h, _ptr(q), _ptr(qcell), B, mode, int(k), float(thr), float(pc), float(cpc), prior.data_ptr(),
                _ptr(counts), int(max_grid), int(chunks), self._stream()))
        return (prior, counts) if want_counts else prior

    # ---- the KDE prior (a weighted set in the same slot)

    def set_kde_points(self, lonlat: np.ndarray, classes: np.ndarray, counts: np.ndarray, num_classes: int,
                       haversine: bool) -> None:
        """``lonlat`` (M, 2) float64 (lon, lat) of the bins - radians with ``haversine``, else degrees -, ``classes``
        (M,) in ``[0, num_classes)``, ``counts`` (M,) >= 1: host arrays (range_set_kde_points)."""
        ll = np.ascontiguousarray(lonlat, dtype=np.float64)
        cls = np.ascontiguousarray(classes, dtype=np.int32)
        cnt64 = np.asarray(counts, dtype=np.int64)
        if ll.ndim != 2 or ll.shape[1] != 2 or cls.shape != (ll.shape[0],) or cnt64.shape != cls.shape:
            raise ValueError(f"lonlat (M, 2), classes (M,) and counts (M,), got {ll.shape}, {cls.shape} and {cnt64.shape}")
        if cnt64.size and (cnt64.max() > 2 ** 31 - 1 or cnt64.min() < -2 ** 31):
            raise ValueError("a count beyond int32")
        cnt = np.ascontiguousarray(cnt64, dtype=np.int32)
        _check(self.lib, self.lib.range_set_kde_points(self._h, ll.ctypes.data, cls.ctypes.data, cnt.ctypes.data, ll.shape[0],
                                                       int(num_classes), int(bool(haversine))))
        self.haversine = bool(haversine)

    @property
    def kde_scale_bits(self) -> int:
        return int(self.lib.range_kde_scale_bits(self._h))

    def _kde_inputs(self, q: torch.Tensor, thr: torch.Tensor, two_h2: torch.Tensor) -> int:
        self._t(q, torch.float64, (2,))
        B = q.shape[0]
        for t in (thr, two_h2):
            self._t(t, torch.float64, ())
            if t.shape[0] != B:
                raise ValueError(f"{t.shape[0]} thresholds / bandwidths for {B} rows")
        return B

    def kde_rank(self, q: torch.Tensor, thr: torch.Tensor, two_h2: torch.Tensor, labels: torch.Tensor,
                 img: Optional[torch.Tensor] = None, max_grid: int = 0, chunks: int = 0):
        """(``greater``, ``tied_after``, ``argmax``), (B,) int32 each, over ``img.double() * prior``
        (range_kde_rank_grid)."""
        B = self._kde_inputs(q, thr, two_h2)
        kind, out = self._rank_args(B, self.neighbor_classes, img, labels)
        if B:
            _check(self.lib, self.lib.range_kde_rank_grid(
                self._h, q.data_ptr(), thr.data_ptr(), two_h2.data_ptr(), B, _ptr(img), kind, labels.data_ptr(),
                out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), int(max_grid), int(chunks), self._stream()))
        return out

    def kde_prior(self, q: torch.Tensor, thr: torch.Tensor, two_h2: torch.Tensor, want_sums: bool = False,
                  max_grid: int = 0, chunks: int = 0):
        """The (B, num_classes) float64 priors (range_kde_prior_grid); with ``want_sums`` also the fixed-point sums,
        (B, num_classes) int64 holding the kernel's uint64 (below 2^62)."""
        B = self._kde_inputs(q, thr, two_h2)
        C_ = self.neighbor_classes
        prior = self._empty((B, C_), torch.float64)
        sums = self._empty((B, C_), torch.int64) if want_sums else None
        if B:
            _check(self.lib, self.lib.range_kde_prior_grid(
                self._h, q.data_ptr(), thr.data_ptr(), two_h2.data_ptr(), B, prior.data_ptr(), _ptr(sums), int(max_grid),
                int(chunks), self._stream()))
        return (prior, sums) if want_sums else prior
