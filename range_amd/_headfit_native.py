"""ctypes binding of include/range_headfit.h (the fit of the CSP class head in librange_hip.so).

``HeadFit`` holds the one fit of a ``HipEngine``'s context - the engine of a loaded model, so that the background
embeddings of a step come from the same context's ``csp_encode``, or an engine of its own - with one method per
``range_headfit_*`` entry point.  Shapes, dtypes, labels and row ids are validated here, on the host; no arithmetic
happens here and there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple, Union

import numpy as np
import torch

from . import _native
from ._native import HipEngine, RangeNativeError, _check, _ptr  # noqa: F401

# every symbol include/range_headfit.h declares
SYMBOLS = (
    "range_headfit_plan", "range_headfit_begin", "range_headfit_classes", "range_headfit_width", "range_headfit_steps",
    "range_headfit_step", "range_headfit_step_grid", "range_headfit_grad", "range_headfit_grad_grid",
    "range_headfit_loss", "range_headfit_loss_grid", "range_headfit_weights",
)
MAX_CLASSES, MAX_WIDTH, MAX_ROWS = 32768, 1024, 8192
#: torch.optim.Adam's defaults
ADAM_DEFAULTS = dict(beta1=0.9, beta2=0.999, eps=1e-8)

_bound = False


def load_library() -> C.CDLL:
    global _bound
    lib = _native.load_library()
    if _bound:
        return lib
    vp, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    rows = [vp, vp, i64, vp, vp, i32, vp, i32, f64]        # ctx, feats, N, rows, labels, B, bg, Bg, weight
    adam = [f64, f64, f64, f64, f64]                       # lr, beta1, beta2, eps, weight_decay
    lib.range_headfit_plan.argtypes = [i32, i32, i64, i64, i32, vp]
    lib.range_headfit_begin.argtypes = [vp, i32, i32, vp]
    lib.range_headfit_classes.argtypes = [vp]
    lib.range_headfit_classes.restype = i32
    lib.range_headfit_width.argtypes = [vp]
    lib.range_headfit_width.restype = i32
    lib.range_headfit_steps.argtypes = [vp]
    lib.range_headfit_steps.restype = i64
    lib.range_headfit_step.argtypes = rows + adam + [vp, vp]
    lib.range_headfit_step_grid.argtypes = rows + adam + [vp, i64, i32, vp]
    lib.range_headfit_grad.argtypes = rows + [vp, vp, vp]
    lib.range_headfit_grad_grid.argtypes = rows + [vp, vp, i64, i32, vp]
    lib.range_headfit_loss.argtypes = rows + [vp, vp]
    lib.range_headfit_loss_grid.argtypes = rows + [vp, i64, i32, vp]
    lib.range_headfit_weights.argtypes = [vp, vp, vp]
    for name in SYMBOLS:
        getattr(lib, name)
    _bound = True
    return lib


def plan(num_classes: int, width: int, rows: int, max_grid: int = 0, panel_cols: int = 0) -> Dict[str, int]:
    """The launch plan of a step on ``rows`` = B + Bg rows (host_plan.h: headfit_plan); needs no GPU."""
    lib = load_library()
    out = np.zeros(8, dtype=np.int64)
    _check(lib, lib.range_headfit_plan(int(num_classes), int(width), int(rows), int(max_grid), int(panel_cols), out.ctypes.data))
    keys = ("panel_cols", "n_panels", "tile_rows", "cols_per_pass", "grad_grid", "update_grid", "lds_bytes", "ws_bytes")
    return dict(zip(keys, (int(v) for v in out)))


def step_rows(fit, noun: str, have: str, dtype: torch.dtype, trail: tuple, data: torch.Tensor, rows: Optional[torch.Tensor],
              labels: torch.Tensor, bg: Optional[torch.Tensor], weight: float, validate: bool) -> list:
    """The checks of a step's rows and the leading arguments of its call, for ``HeadFit`` and ``_cspfit_native.CspFit``:
    ``data`` and ``bg`` are ``dtype`` tensors (n,) + ``trail``; ``noun`` names the fit and ``have`` what ``data`` has
    in the messages."""
    e, C_ = fit.engine, fit.num_classes
    if not C_:
        raise RangeNativeError(f"no {noun} fit begun on this engine (begin)")
    e._t(data, dtype, trail)
    e._t(labels, torch.int32, ())
    N, B = data.shape[0], labels.shape[0]
    if rows is not None:
        e._t(rows, torch.int32, ())
        if rows.shape[0] != B:
            raise ValueError(f"{rows.shape[0]} row ids for {B} labels")
    elif N < B:
        raise ValueError(f"{B} labels without row ids: " + have.format(N))
    Bg = 0
    if bg is not None:
        e._t(bg, dtype, trail)
        Bg = bg.shape[0]
    if B < 1 or B + Bg > MAX_ROWS:
        raise ValueError(f"B = {B}, Bg = {Bg}: 1 <= B and B + Bg <= {MAX_ROWS}")
    if validate:
        # (device reads: a synchronisation; the fitting loops validate their host arrays once instead)
        if bool(((labels < 0) | (labels >= C_)).any()):
            raise ValueError(f"a label outside 0 .. {C_ - 1}")
        if rows is not None and bool(((rows < 0) | (rows >= N)).any()):
            raise ValueError(f"a row id outside 0 .. {N - 1}")
    return [fit._h, data.data_ptr(), N, _ptr(rows), labels.data_ptr(), B, _ptr(bg if Bg else None), Bg, float(weight)]


class HeadFit:
    """The class-head fit of one engine context."""

    def __init__(self, engine: Union[HipEngine, torch.device, int, str] = 0):
        self.lib = load_library()
        self.engine = engine if isinstance(engine, HipEngine) else HipEngine(engine)

    @property
    def _h(self):
        return self.engine._h

    def begin(self, num_classes: int, width: int, w0: Optional[np.ndarray] = None) -> None:
        """Start a fit of a (num_classes, width) head from ``w0`` (float32, host) or zeros (range_headfit_begin)."""
        w = None
        if w0 is not None:
            w = np.ascontiguousarray(w0, dtype=np.float32)
            if w.shape != (int(num_classes), int(width)):
                raise ValueError(f"w0 {w.shape} is not ({num_classes}, {width})")
            if not np.isfinite(w).all():
                raise ValueError("w0 has non-finite entries")
        _check(self.lib, self.lib.range_headfit_begin(self._h, int(num_classes), int(width), None if w is None else w.ctypes.data))

    @property
    def num_classes(self) -> int:
        return int(self.lib.range_headfit_classes(self._h))

    @property
    def width(self) -> int:
        return int(self.lib.range_headfit_width(self._h))

    @property
    def steps(self) -> int:
        return int(self.lib.range_headfit_steps(self._h))

    def _rows(self, feats: torch.Tensor, rows: Optional[torch.Tensor], labels: torch.Tensor, bg: Optional[torch.Tensor],
              weight: float, validate: bool):
        return step_rows(self, "class-head", "the feature matrix has {} rows", torch.float32, (self.width,), feats, rows, labels, bg,
                         weight, validate)

    def step(self, feats: torch.Tensor, rows: Optional[torch.Tensor], labels: torch.Tensor, bg: Optional[torch.Tensor],
             lr: float, weight: float = 1.0, weight_decay: float = 0.0, beta1: float = 0.9, beta2: float = 0.999,
             eps: float = 1e-8, want_loss: bool = True, validate: bool = False, max_grid: int = 0,
             panel_cols: int = 0) -> Optional[torch.Tensor]:
        """One Adam step (range_headfit_step_grid); the (3,) float32 loss scalars at the weights it started from."""
        args = self._rows(feats, rows, labels, bg, weight, validate)
        loss = self.engine._empty((3,), torch.float32) if want_loss else None
        _check(self.lib, self.lib.range_headfit_step_grid(*args, float(lr), float(beta1), float(beta2), float(eps),
                                                          float(weight_decay), _ptr(loss), int(max_grid), int(panel_cols),
                                                          self.engine._stream()))
        return loss

    def grad(self, feats: torch.Tensor, rows: Optional[torch.Tensor], labels: torch.Tensor, bg: Optional[torch.Tensor],
             weight: float = 1.0, validate: bool = False, max_grid: int = 0, panel_cols: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """(dW (C, F) float32, loss scalars (3,)) at the current weights (range_headfit_grad_grid)."""
        args = self._rows(feats, rows, labels, bg, weight, validate)
        dW = self.engine._empty((self.num_classes, self.width), torch.float32)
        loss = self.engine._empty((3,), torch.float32)
        _check(self.lib, self.lib.range_headfit_grad_grid(*args, dW.data_ptr(), loss.data_ptr(), int(max_grid), int(panel_cols),
                                                          self.engine._stream()))
        return dW, loss

    def loss(self, feats: torch.Tensor, rows: Optional[torch.Tensor], labels: torch.Tensor, bg: Optional[torch.Tensor],
             weight: float = 1.0, validate: bool = False, max_grid: int = 0, panel_cols: int = 0) -> torch.Tensor:
        """The (3,) float32 loss scalars - loss, its batch part, the mean label term (range_headfit_loss_grid)."""
        args = self._rows(feats, rows, labels, bg, weight, validate)
        loss = self.engine._empty((3,), torch.float32)
        _check(self.lib, self.lib.range_headfit_loss_grid(*args, loss.data_ptr(), int(max_grid), int(panel_cols),
                                                          self.engine._stream()))
        return loss

    def weights(self) -> torch.Tensor:
        """The current W, (C, F) float32 on the GPU (range_headfit_weights)."""
        if not self.num_classes:
            raise RangeNativeError("no class-head fit begun on this engine (begin)")
        W = self.engine._empty((self.num_classes, self.width), torch.float32)
        _check(self.lib, self.lib.range_headfit_weights(self._h, W.data_ptr(), self.engine._stream()))
        return W
