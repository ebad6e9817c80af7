"""ctypes binding of include/range_map.h (the embedding-map entry points of librange_hip.so).

``MapEngine`` is a ``ProbeEngine`` (same context, same helpers) with one method per ``range_map_*`` entry
point.  No arithmetic happens here; there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _probe_native
from ._native import RangeNativeError, _check  # noqa: F401
from ._probe_native import ProbeEngine

# every symbol include/range_map.h declares
SYMBOLS = (
    "range_map_plan", "range_map_reserve", "range_map_project", "range_map_ica_step", "range_map_sources",
    "range_map_equalize",
)
MAX_C = 8
MAX_BINS = 1024

_bound = False


def load_library() -> C.CDLL:
    global _bound
    lib = _probe_native.load_library()
    if _bound:
        return lib
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    lib.range_map_plan.argtypes = [i64, i32, i64, vp]
    lib.range_map_reserve.argtypes = [vp, i64, i32]
    lib.range_map_project.argtypes = [vp, vp, i64, i32, i64, vp, vp, i32, vp, i64, i64, vp]
    lib.range_map_ica_step.argtypes = [vp, vp, i64, i64, i32, vp, vp, i64, vp]
    lib.range_map_sources.argtypes = [vp, vp, i64, i64, i32, vp, vp, i64, vp]
    lib.range_map_equalize.argtypes = [vp, vp, i64, i64, vp, i32, vp, vp, i64, i64, vp]
    for name in SYMBOLS:
        getattr(lib, name)
    _bound = True
    return lib


def plan(n: int, c: int, max_grid: int = 0) -> Dict[str, int]:
    """The launch plan of n rows and c components (host_plan.h: map_plan); needs no GPU."""
    lib = load_library()
    out = np.zeros(8, dtype=np.int64)
    _check(lib, lib.range_map_plan(n, c, max_grid, out.ctypes.data))
    keys = ("chunk", "slabs", "step_grid", "ws_bytes", "proj_rows", "proj_grid", "eq_rows", "eq_grid")
    return dict(zip(keys, (int(v) for v in out)))


class MapEngine(ProbeEngine):
    """One probe context on one GPU, with the embedding map's entry points."""

    def __init__(self, device: torch.device | int | str = 0):
        load_library()
        super().__init__(device)

    def _mat(self, M, c: int) -> np.ndarray:
        M = np.ascontiguousarray(M, dtype=np.float64)
        if M.shape != (c, c):
            raise ValueError(f"expected a ({c}, {c}) matrix, got {M.shape}")
        return M

    def _comp_major(self, Y: torch.Tensor) -> Tuple[int, int, int]:
        """(c, n, ldy) of a component-major float64 (c, n) tensor with unit-stride rows."""
        ldy = self._ld(Y, "Y")
        return Y.shape[0], Y.shape[1], ldy

    def reserve(self, n: int, c: int) -> None:
        _check(self.lib, self.lib.range_map_reserve(self._h, n, c))

    def project(self, X: torch.Tensor, K: torch.Tensor, mean: Optional[torch.Tensor] = None,
                max_grid: int = 0) -> torch.Tensor:
        """Y (c, n) = K (X - mean)^T for X (n, d) contiguous or row-strided, K (c, d), mean (d,)."""
        ldx = self._ld(X, "project X")
        n, d = X.shape
        c = self._chk(K, torch.float64, 2).shape[0]
        if K.shape[1] != d or (mean is not None and tuple(self._chk(mean, torch.float64, 1).shape) != (d,)):
            raise ValueError("project: K / mean do not match X")
        Y = self.empty((c, n))
        _check(self.lib, self.lib.range_map_project(self._h, X.data_ptr(), n, d, ldx, _probe_native._p(mean),
                                                    K.data_ptr(), c, Y.data_ptr(), n, max_grid, self._stream()))
        return Y

    def ica_step(self, Y: torch.Tensor, W, max_grid: int = 0) -> torch.Tensor:
        """(c*c + c,) device tensor: A (c, c) = tanh(W Y) Y^T row-major, then b (c,) = sum(1 - tanh^2(W Y))."""
        c, n, ldy = self._comp_major(Y)
        W = self._mat(W, c)
        out = self.empty(c * c + c)
        _check(self.lib, self.lib.range_map_ica_step(self._h, Y.data_ptr(), n, ldy, c, W.ctypes.data,
                                                     out.data_ptr(), max_grid, self._stream()))
        return out

    def sources(self, Y: torch.Tensor, M, max_grid: int = 0) -> torch.Tensor:
        """S (n, c) = (M Y)^T."""
        c, n, ldy = self._comp_major(Y)
        M = self._mat(M, c)
        S = self.empty((n, c))
        _check(self.lib, self.lib.range_map_sources(self._h, Y.data_ptr(), n, ldy, c, M.ctypes.data,
                                                    S.data_ptr(), max_grid, self._stream()))
        return S

    def equalize(self, x: torch.Tensor, edges: torch.Tensor, out: Optional[torch.Tensor] = None,
                 max_grid: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """(out, counts) of one column: x and out are 1-d float64 views of any positive stride, edges the
        (nbins + 1,) bin edges; counts (nbins,) int64 is numpy.histogram's."""
        if x.device != self.device or x.dtype != torch.float64 or x.dim() != 1 or x.numel() == 0:
            raise ValueError("equalize: a non-empty 1-d float64 tensor on the engine device")
        nbins = self._chk(edges, torch.float64, 1).shape[0] - 1
        if out is None:
            out = self.empty(x.shape[0])
        if out.device != self.device or out.dtype != torch.float64 or tuple(out.shape) != tuple(x.shape):
            raise ValueError("equalize: out does not match x")
        ldx, ldo = (max(x.stride(0), 1), max(out.stride(0), 1))
        counts = torch.empty(max(nbins, 0), dtype=torch.int64, device=self.device)
        _check(self.lib, self.lib.range_map_equalize(self._h, x.data_ptr(), x.shape[0], ldx, edges.data_ptr(),
                                                     nbins, counts.data_ptr(), out.data_ptr(), ldo, max_grid,
                                                     self._stream()))
        return out, counts
