"""ctypes binding of include/range_cspfit.h (training a CSP location encoder and its class head in librange_hip.so).

``CspFit`` holds the one fit of a ``HipEngine``'s context with one method per ``range_cspfit_*`` entry point.  Shapes,
dtypes, labels and row ids are validated here, on the host; no arithmetic happens here and there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _native
from ._headfit_native import step_rows
from ._native import HipEngine, RangeNativeError, _check, _ptr  # noqa: F401
from .csp import ACTIVATIONS, CspParams

# every symbol include/range_cspfit.h declares
SYMBOLS = (
    "range_cspfit_plan", "range_cspfit_begin", "range_cspfit_classes", "range_cspfit_width", "range_cspfit_steps",
    "range_cspfit_param_count", "range_cspfit_step", "range_cspfit_step_grid", "range_cspfit_grad", "range_cspfit_grad_grid",
    "range_cspfit_loss", "range_cspfit_params",
)
MAX_CLASSES, MAX_WIDTH, MAX_ROWS = 32768, 1024, 8192
PLAN_KEYS = ("panel_cols", "n_panels", "tile_rows", "ln_lanes", "feat_grid", "row_grid", "back_grid", "grad_grid", "update_grid",
             "lds_bytes", "ws_bytes", "n_params", "store_floats", "widest")

_bound = False


def load_library() -> C.CDLL:
    global _bound
    lib = _native.load_library()
    if _bound:
        return lib
    vp, i32, i64, u64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_double
    rows = [vp, vp, i64, vp, vp, i32, vp, i32, f64]        # ctx, lonlat, N, rows, labels, B, bg, Bg, weight
    adam = [f64, f64, f64, f64, f64]                       # lr, beta1, beta2, eps, weight_decay
    drop = [f64, u64]                                      # dropout_p, dropout_seed
    lib.range_cspfit_plan.argtypes = [i32, i32, i32, vp, i32, i32, i32, i64, i64, i32, vp]
    lib.range_cspfit_begin.argtypes = [vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, i32, i32, i32, vp, i32]
    for name, res in (("classes", i32), ("width", i32), ("steps", i64), ("param_count", i64)):
        fn = getattr(lib, "range_cspfit_" + name)
        fn.argtypes, fn.restype = [vp], res
    lib.range_cspfit_step.argtypes = rows + adam + drop + [vp, vp]
    lib.range_cspfit_step_grid.argtypes = rows + adam + drop + [vp, i64, i32, vp]
    lib.range_cspfit_grad.argtypes = rows + drop + [vp, vp, vp]
    lib.range_cspfit_grad_grid.argtypes = rows + drop + [vp, vp, i64, i32, vp]
    lib.range_cspfit_loss.argtypes = rows + drop + [vp, vp, vp]
    lib.range_cspfit_params.argtypes = [vp, vp, vp]
    for name in SYMBOLS:
        getattr(lib, name)
    _bound = True
    return lib


def plan(kind: int, F: int, widths: Sequence[int], skip: bool, use_layn: bool, num_classes: int, rows: int, max_grid: int = 0,
         panel_cols: int = 0) -> Dict[str, int]:
    """The launch plan of a step on ``rows`` = B + Bg rows (host_plan.h: cspfit_plan); needs no GPU."""
    lib = load_library()
    out = np.zeros(16, dtype=np.int64)
    wd = np.ascontiguousarray(widths, dtype=np.int32)
    _check(lib, lib.range_cspfit_plan(int(kind), int(F), len(wd), wd.ctypes.data, int(bool(skip)), int(bool(use_layn)),
                                      int(num_classes), int(rows), int(max_grid), int(panel_cols), out.ctypes.data))
    return dict(zip(PLAN_KEYS, (int(v) for v in out)))


def unpacked_layout(p: CspParams, num_classes: int) -> List[Tuple[str, int, tuple]]:
    """(name, offset, shape) of every tensor in the unpacked order of ``grad`` / ``params``."""
    out, off, d_in = [], 0, p.input_dim
    for i, d_out in enumerate(p.widths):
        entries = [(f"w{i}", (d_out, d_in)), (f"b{i}", (d_out,))]
        if p.use_layn and i + 1 < len(p.widths):
            entries += [(f"g{i}", (d_out,)), (f"be{i}", (d_out,))]
        for name, shape in entries:
            out.append((name, off, shape))
            off += int(np.prod(shape))
        d_in = d_out
    out.append(("class_emb", off, (int(num_classes), p.num_filts)))
    return out


def split_unpacked(flat, p: CspParams, num_classes: int) -> Dict[str, object]:
    """The flat vector of ``grad`` / ``params`` as a dict of views name -> tensor / array of its shape."""
    return {name: flat[off:off + int(np.prod(shape))].reshape(shape) for name, off, shape in unpacked_layout(p, num_classes)}


class CspFit:
    """The CSP encoder fit of one engine context."""

    def __init__(self, engine: Union[HipEngine, torch.device, int, str] = 0):
        self.lib = load_library()
        self.engine = engine if isinstance(engine, HipEngine) else HipEngine(engine)
        self.params: Optional[CspParams] = None

    @property
    def _h(self):
        return self.engine._h

    def begin(self, p: CspParams, num_classes: int, class_emb: Optional[np.ndarray] = None) -> None:
        """Start a fit of the network ``p`` with a (num_classes, num_filts) head from ``class_emb`` (float32, host) or
        zeros (range_cspfit_begin)."""
        n = len(p.widths)
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)   # noqa: E731
        ws, bs, gs, bes = ([f32(a) for a in arrs] for arrs in (p.weights, p.biases, p.ln_gamma, p.ln_beta))
        d_in = p.input_dim
        for i, d_out in enumerate(p.widths):
            if ws[i].shape != (d_out, d_in) or bs[i].shape != (d_out,):
                raise ValueError(f"layer {i}: weight {ws[i].shape} / bias {bs[i].shape} do not match ({d_out},{d_in})")
            if any(a is not None and a.shape != (d_out,) for a in (gs[i], bes[i])):
                raise ValueError(f"layer {i}: LayerNorm parameters do not match ({d_out},)")
            d_in = d_out
        w = None
        if class_emb is not None:
            w = np.ascontiguousarray(class_emb, dtype=np.float32)
            if w.shape != (int(num_classes), p.num_filts):
                raise ValueError(f"class_emb {w.shape} is not ({num_classes}, {p.num_filts})")
        for a in ws + bs + gs + bes + [w]:
            if a is not None and not np.isfinite(a).all():
                raise ValueError("a parameter has non-finite entries")
        freq = np.ascontiguousarray(p.freq_list, dtype=np.float64)
        wd = np.ascontiguousarray(p.widths, dtype=np.int32)
        arr = lambda xs: (C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in xs])   # noqa: E731
        _check(self.lib, self.lib.range_cspfit_begin(self._h, int(p.kind), freq.ctypes.data, freq.shape[0], n, wd.ctypes.data, arr(ws),
                                                     arr(bs), arr(gs), arr(bes), ACTIVATIONS[p.activation],
                                                     int(bool(p.skip_connection)), int(bool(p.use_layn)),
                                                     None if w is None else w.ctypes.data, int(num_classes)))
        self.params = p

    @property
    def num_classes(self) -> int:
        return int(self.lib.range_cspfit_classes(self._h))

    @property
    def width(self) -> int:
        return int(self.lib.range_cspfit_width(self._h))

    @property
    def steps(self) -> int:
        return int(self.lib.range_cspfit_steps(self._h))

    @property
    def param_count(self) -> int:
        return int(self.lib.range_cspfit_param_count(self._h))

    def _rows(self, lonlat: torch.Tensor, rows: Optional[torch.Tensor], labels: torch.Tensor, bg: Optional[torch.Tensor],
              weight: float, validate: bool):
        return step_rows(self, "CSP", "there are {} locations", torch.float64, (2,), lonlat, rows, labels, bg, weight, validate)

    def step(self, lonlat: torch.Tensor, rows: Optional[torch.Tensor], labels: torch.Tensor, bg: Optional[torch.Tensor],
             lr: float, weight: float = 1.0, weight_decay: float = 0.0, beta1: float = 0.9, beta2: float = 0.999,
             eps: float = 1e-8, dropout: float = 0.0, seed: int = 0, want_loss: bool = True, validate: bool = False,
             max_grid: int = 0, panel_cols: int = 0) -> Optional[torch.Tensor]:
        """One Adam step (range_cspfit_step_grid); the (3,) float32 loss scalars at the parameters it started from."""
        args = self._rows(lonlat, rows, labels, bg, weight, validate)
        loss = self.engine._empty((3,), torch.float32) if want_loss else None
        _check(self.lib, self.lib.range_cspfit_step_grid(*args, float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
                                                         float(dropout), int(seed), _ptr(loss), int(max_grid), int(panel_cols),
                                                         self.engine._stream()))
        return loss

    def grad(self, lonlat: torch.Tensor, rows: Optional[torch.Tensor], labels: torch.Tensor, bg: Optional[torch.Tensor],
             weight: float = 1.0, dropout: float = 0.0, seed: int = 0, validate: bool = False, max_grid: int = 0,
             panel_cols: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """(every gradient, flat float32 in the unpacked order; loss scalars (3,)) (range_cspfit_grad_grid)."""
        args = self._rows(lonlat, rows, labels, bg, weight, validate)
        g = self.engine._empty((self.param_count,), torch.float32)
        loss = self.engine._empty((3,), torch.float32)
        _check(self.lib, self.lib.range_cspfit_grad_grid(*args, float(dropout), int(seed), g.data_ptr(), loss.data_ptr(), int(max_grid),
                                                         int(panel_cols), self.engine._stream()))
        return g, loss

    def loss(self, lonlat: torch.Tensor, rows: Optional[torch.Tensor], labels: torch.Tensor, bg: Optional[torch.Tensor],
             weight: float = 1.0, dropout: float = 0.0, seed: int = 0, validate: bool = False,
             want_emb: bool = False):
        """The (3,) float32 loss scalars (range_cspfit_loss); with ``want_emb`` also the (B + Bg, num_filts) embeddings."""
        args = self._rows(lonlat, rows, labels, bg, weight, validate)
        loss = self.engine._empty((3,), torch.float32)
        emb = self.engine._empty((args[5] + args[7], self.width), torch.float32) if want_emb else None
        _check(self.lib, self.lib.range_cspfit_loss(*args, float(dropout), int(seed), loss.data_ptr(), _ptr(emb), self.engine._stream()))
        return (loss, emb) if want_emb else loss

    def flat_params(self) -> torch.Tensor:
        """Every current parameter, flat float32 on the GPU in the unpacked order (range_cspfit_params)."""
        if not self.num_classes:
            raise RangeNativeError("no CSP fit begun on this engine (begin)")
        out = self.engine._empty((self.param_count,), torch.float32)
        _check(self.lib, self.lib.range_cspfit_params(self._h, out.data_ptr(), self.engine._stream()))
        return out

    def trained(self) -> CspParams:
        """The current parameters as a ``CspParams`` (the network ``begin`` got, with the trained tensors and head)."""
        import dataclasses
        p, C_ = self.params, self.num_classes
        t = split_unpacked(self.flat_params().cpu().numpy(), p, C_)
        n = len(p.widths)
        has = [p.use_layn and i + 1 < n for i in range(n)]
        return dataclasses.replace(
            p, weights=[t[f"w{i}"].copy() for i in range(n)], biases=[t[f"b{i}"].copy() for i in range(n)],
            ln_gamma=[t[f"g{i}"].copy() if has[i] else None for i in range(n)],
            ln_beta=[t[f"be{i}"].copy() if has[i] else None for i in range(n)], num_classes=C_, class_emb=t["class_emb"].copy())
