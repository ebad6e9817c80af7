"""CSP checkpoint reader for the 'CSP' / 'CSP_INat' models (reference: range/range.py:141-150 ->
location_models/csp/load_csp.py ``get_csp`` -> csp/main/utils.py ``get_model`` / ``get_spa_encoder`` /
``get_ffn``).

The reference rebuilds the whole ``LocationImageEncoder`` (class and user heads, the image decoder) and
calls ``forward(coords, return_feats=True)``; only the feed-forward net behind the spatial encoder
matters on that path, so only ``params`` and the ``loc_enc.spa_enc.ffn.layers.*`` tensors are read.
numpy / torch-CPU only: importable, and testable, without a GPU.  The kernel: range_amd/csrc/csp_kernel.h.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from . import posenc
from .ckpt import _load_file

# range_set_csp(act), include/range_hip.h (csp/main/module.py:33-45)
ACTIVATIONS = {"sigmoid": 0, "relu": 1, "leakyrelu": 2, "tanh": 3, "gelu": 4}
#: spa_enc_type -> kernel kind (the feature layouts posenc_kernel.h's arithmetic produces)
SPA_ENC_KINDS = {"gridcell": posenc.KIND_GRID, "theory": posenc.KIND_THEORY}
#: what csp/main/utils.py:get_spa_enc_list and get_model know beyond those two
UNSUPPORTED_SPA_ENC = ("gridcellnorm", "hexagridcell", "theorynorm", "theorydiag", "naive", "rbf", "rff",
                       "geo_net", "geo_net_fft")
MAX_FREQ, MAX_WIDTH, MAX_HIDDEN_LAYERS = 64, 1024, 8     # the kernel's envelope (host_plan.h: csp_plan)
MAX_CLASSES = 32768                                      # ... of the class head (host_plan.h: csp_head_plan)
_PREFIX = "loc_enc.spa_enc.ffn.layers."
_CLASS_EMB = "loc_enc.class_emb"


@dataclass
class CspParams:
    spa_enc_type: str
    kind: int                      # posenc.KIND_GRID / KIND_THEORY
    frequency_num: int
    min_radius: float
    max_radius: float
    freq_init: str
    freq_list: np.ndarray          # (F,) float64
    num_hidden_layer: int
    hidden_dim: int
    num_filts: int
    activation: str                # params['spa_f_act']
    use_layn: bool
    skip_connection: bool
    widths: List[int]              # output width of every linear layer; the last is num_filts
    weights: List[np.ndarray]      # float32 (out, in)
    biases: List[np.ndarray]       # float32 (out,)
    ln_gamma: List[Optional[np.ndarray]]   # float32 (out,) for the hidden layers with use_layn, else None
    ln_beta: List[Optional[np.ndarray]]
    num_classes: int = 0                     # read_csp_checkpoint(class_head=True): params['num_classes']
    class_emb: Optional[np.ndarray] = None   # ... and float32 (num_classes, num_filts), bias-free
    dropout: float = 0.0                     # params['dropout']: train mode only (range_amd.csp_fit)

    @property
    def input_dim(self) -> int:
        return posenc.PER_FREQ[self.kind] * self.frequency_num


def cal_freq_list(freq_init: str, frequency_num: int, max_radius, min_radius) -> np.ndarray:
    """``_cal_freq_list`` (csp/main/SpatialRelationEncoder.py:18-49) in its expression order.  'random' draws
    from ``np.random`` when the model is BUILT and is not stored in the checkpoint: it cannot be reproduced."""
    if freq_init == "geometric":
        if frequency_num < 2:
            raise ValueError("freq_init='geometric' needs frequency_num >= 2 (the reference divides by frequency_num - 1)")
        return posenc.cal_freq_list(frequency_num, max_radius, min_radius)
    if freq_init == "nerf":
        return np.pi * np.exp2(np.arange(frequency_num).astype(float))
    raise NotImplementedError(
        f"freq_init={freq_init!r}: " + ("the reference draws these frequencies at random when it builds the model and "
                                       "does not store them" if freq_init == "random" else "unknown"))


def _np32(t, what: str, shape) -> np.ndarray:
    a = np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t))
    if a.shape != tuple(shape):
        raise ValueError(f"{what}: shape {a.shape}, params say {tuple(shape)}")
    if a.dtype != np.float32:
        raise ValueError(f"{what}: dtype {a.dtype}, the reference's network is float32")
    return a


def read_csp_checkpoint(path: str, class_head: bool = False) -> CspParams:
    """``{'params', 'state_dict'}`` as csp/main/trainer.py saves it -> ``CspParams``.  ``params['device']``,
    the heads (``class_emb``, ``user_emb``, ``img_dec`` / ``loc_dec``) and the ``spa_enc.*`` aliases of the
    same tensors are ignored.  NotImplementedError names an unsupported ``spa_enc_type`` / ``freq_init``;
    ValueError: a tensor whose shape is not what ``params`` say, or a network outside the kernel's envelope.
    ``class_head=True`` also reads the class head (models.py:187-190: ``class_emb``, a bias-free
    ``Linear(num_filts, num_classes)``) from ``loc_enc.class_emb.weight`` into ``class_emb`` / ``num_classes``;
    ValueError: the key missing, a ``class_emb.bias`` present, ``num_classes`` outside 1 .. 32768."""
    ck = _load_file(path)
    params, sd = ck["params"], ck["state_dict"]
    spa = params["spa_enc_type"]
    if spa not in SPA_ENC_KINDS:
        raise NotImplementedError(f"CSP spa_enc_type={spa!r}: only {sorted(SPA_ENC_KINDS)} are implemented")
    kind = SPA_ENC_KINDS[spa]
    F = int(params["frequency_num"])
    act = params["spa_f_act"]
    if act not in ACTIVATIONS:
        raise NotImplementedError(f"CSP spa_f_act={act!r} activation not recognized")   # module.py:45
    freq_init = params["freq_init"]
    n_hidden, hidden, num_filts = int(params["num_hidden_layer"]), int(params["hidden_dim"]), int(params["num_filts"])
    if not 1 <= F <= MAX_FREQ:
        raise ValueError(f"CSP frequency_num={F}: 1 .. {MAX_FREQ} are supported")
    if n_hidden > MAX_HIDDEN_LAYERS:
        raise ValueError(f"CSP num_hidden_layer={n_hidden}: at most {MAX_HIDDEN_LAYERS} are supported")
    freqs = np.ascontiguousarray(cal_freq_list(freq_init, F, params["max_radius"], params["min_radius"]), dtype=np.float64)
    widths = [hidden] * max(n_hidden, 0) + [num_filts]          # module.py:177-209
    for w in widths:
        if not 1 <= w <= MAX_WIDTH:
            raise ValueError(f"CSP layer width {w}: 1 .. {MAX_WIDTH} are supported")
    use_layn, skip = bool(params["use_layn"]), bool(params["skip_connection"])
    ws, bs, gs, bes = [], [], [], []
    d_in = posenc.PER_FREQ[kind] * F
    for i, d_out in enumerate(widths):
        pre = f"{_PREFIX}{i}."
        ws.append(_np32(sd[pre + "linear.weight"], pre + "linear.weight", (d_out, d_in)))
        bs.append(_np32(sd[pre + "linear.bias"], pre + "linear.bias", (d_out,)))
        has_ln = use_layn and i + 1 < len(widths)
        if has_ln != (pre + "layernorm.weight" in sd):
            raise ValueError(f"{pre}layernorm.*: {'missing' if has_ln else 'present'} although use_layn={use_layn}")
        gs.append(_np32(sd[pre + "layernorm.weight"], pre + "layernorm.weight", (d_out,)) if has_ln else None)
        bes.append(_np32(sd[pre + "layernorm.bias"], pre + "layernorm.bias", (d_out,)) if has_ln else None)
        d_in = d_out
    if f"{_PREFIX}{len(widths)}.linear.weight" in sd:
        raise ValueError("state_dict has more layers than params['num_hidden_layer'] says")
    p = CspParams(spa, kind, F, float(params["min_radius"]), float(params["max_radius"]), freq_init, freqs,
                  n_hidden, hidden, num_filts, act, use_layn, skip, widths, ws, bs, gs, bes)
    p.dropout = float(params.get("dropout", 0.0))
    if class_head:
        C = int(params["num_classes"])
        if not 1 <= C <= MAX_CLASSES:
            raise ValueError(f"CSP num_classes={C}: 1 .. {MAX_CLASSES} are supported")
        if _CLASS_EMB + ".weight" not in sd:
            raise ValueError(f"{_CLASS_EMB}.weight: missing from the state_dict (class_head=True)")
        if _CLASS_EMB + ".bias" in sd:
            raise ValueError(f"{_CLASS_EMB}.bias: present although the reference's class head has no bias")
        p.num_classes = C
        p.class_emb = _np32(sd[_CLASS_EMB + ".weight"], _CLASS_EMB + ".weight", (C, num_filts))
    return p


def save_csp_checkpoint(path: str, p: CspParams) -> str:
    """Write ``p`` - a trained network (range_amd.csp_fit) - as the ``{'params', 'state_dict'}`` file csp/main/trainer.py
    saves, under the reference's key names (``loc_enc.spa_enc.ffn.layers.{i}.linear.*`` / ``.layernorm.*`` and their
    ``spa_enc.*`` aliases, ``loc_enc.class_emb.weight`` / ``class_emb.weight`` when ``p.class_emb`` is set):
    ``read_csp_checkpoint(path, class_head=p.class_emb is not None)`` returns the same tensors bit for bit.  ``params``
    holds what the reader and the reference's ``get_model`` / ``get_ffn`` read of the network; the user head and the
    image decoder, which a fit here does not train, are not written."""
    import torch

    if p.spa_enc_type not in SPA_ENC_KINDS or p.activation not in ACTIVATIONS:
        raise NotImplementedError(f"CSP spa_enc_type={p.spa_enc_type!r} / spa_f_act={p.activation!r}")
    n = len(p.widths)
    if not (len(p.weights) == len(p.biases) == len(p.ln_gamma) == len(p.ln_beta) == n):
        raise ValueError("one weight, bias, gamma and beta entry per layer")
    sd = {}
    d_in = p.input_dim
    for i, d_out in enumerate(p.widths):
        has_ln = p.use_layn and i + 1 < n
        entries = [("linear.weight", p.weights[i], (d_out, d_in)), ("linear.bias", p.biases[i], (d_out,))]
        if has_ln:
            entries += [("layernorm.weight", p.ln_gamma[i], (d_out,)), ("layernorm.bias", p.ln_beta[i], (d_out,))]
        for name, a, shape in entries:
            t = torch.from_numpy(_np32(a, f"layer {i} {name}", shape).copy())
            sd[f"{_PREFIX}{i}.{name}"] = t
            sd[f"spa_enc.ffn.layers.{i}.{name}"] = t
        d_in = d_out
    params = {"spa_enc_type": p.spa_enc_type, "num_loc_feats": 2, "num_filts": int(p.num_filts), "num_users": 1,
              "frequency_num": int(p.frequency_num), "max_radius": p.max_radius, "min_radius": p.min_radius,
              "spa_f_act": p.activation, "freq_init": p.freq_init, "num_hidden_layer": int(p.num_hidden_layer),
              "hidden_dim": int(p.hidden_dim), "dropout": float(p.dropout), "use_layn": bool(p.use_layn),
              "skip_connection": bool(p.skip_connection), "device": "cpu", "num_classes": int(p.num_classes)}
    if p.class_emb is not None:
        t = torch.from_numpy(_np32(p.class_emb, _CLASS_EMB + ".weight", (p.num_classes, p.num_filts)).copy())
        sd[_CLASS_EMB + ".weight"] = t
        sd["class_emb.weight"] = t
    torch.save({"params": params, "state_dict": sd}, path)
    return path
