"""numpy float64 restatement of the reference's CSP location encoders (csp/main/SpatialRelationEncoder.py
'gridcell' / 'theory' features -> module.py's feed-forward net): what the GPU tests compare csp_kernel.h
with.  The features are formed in float64 and rounded ONCE to float32, as the reference does
(torch.FloatTensor of a numpy float64 array); the network then runs in float64 on those float32 features
and the float32 parameters - the exact value both float32 evaluations (the reference's, the kernel's)
approximate.  tests/test_csp_cpu.py measures the reference's distance to it from the fixture (``e_ref``).

``defect``: a planted mistake (None: none), for the tests that show the bound catches it -
'noskip' (skip connection dropped), 'unbiased_var' (LayerNorm's variance over N - 1), 'eps_outside'
(eps added to the standard deviation instead of under the root), 'tanh_gelu' (GELU's tanh approximation),
'no_out_act' (the output layer's activation dropped), 'f32_angles' (coordinate * frequency formed in
float32), 'pad_in_layernorm' (the zero columns that pad a width to a multiple of 32 counted in LayerNorm's
mean and variance).
"""
from __future__ import annotations

import hashlib
import json
import math

import numpy as np

import posenc_refs as P

DEFECTS = ("noskip", "unbiased_var", "eps_outside", "tanh_gelu", "no_out_act", "f32_angles", "pad_in_layernorm")
CASES = ("a_design", "b_theory", "c_odd", "d_nohidden", "e_sigmoid", "f_tanh")
KIND_OF = {"gridcell": "grid", "theory": "theory"}
_erf = np.vectorize(math.erf, otypes=[np.float64])


def features(spa_enc_type: str, lonlat, freq, defect=None) -> np.ndarray:
    """(B, 4F | 6F) float32: the reference's ``make_input_embeds`` rounded as ``torch.FloatTensor`` rounds."""
    q, f = np.asarray(lonlat, dtype=np.float64), np.asarray(freq, dtype=np.float64)
    if defect == "f32_angles":
        # the angle as a float32 product (of the float32 coordinate and frequency), the sine of that
        kind = KIND_OF[spa_enc_type]
        q32, f32 = q.astype(np.float32), f.astype(np.float32)
        with np.errstate(invalid="ignore"):
            if kind == "grid":
                al, at = (q32[:, 0:1] * f32[None, :]).astype(np.float64), (q32[:, 1:2] * f32[None, :]).astype(np.float64)
                return np.concatenate([np.stack([np.sin(al), np.cos(al)], -1).reshape(len(q), -1),
                                       np.stack([np.sin(at), np.cos(at)], -1).reshape(len(q), -1)], 1).astype(np.float32)
            s3h = np.float32(P.S3H)
            ang = [q32[:, 0:1] * np.float32(ux) + q32[:, 1:2] * np.float32(uy) for ux, uy in ((1, 0), (-0.5, s3h), (-0.5, -s3h))]
            cols = []
            for a in ang:
                t = (a * f32[None, :]).astype(np.float64)
                cols += [np.sin(t), np.cos(t)]
            return np.stack(cols, -1).reshape(len(q), -1).astype(np.float32)
    return P.encode(KIND_OF[spa_enc_type], q, f).astype(np.float32)


def activation(name: str, v: np.ndarray, defect=None) -> np.ndarray:
    with np.errstate(over="ignore", invalid="ignore"):
        if name == "sigmoid":
            return 1.0 / (1.0 + np.exp(-v))
        if name == "relu":
            return np.where(v < 0.0, 0.0, v)                       # (NaN stays NaN, as torch's)
        if name == "leakyrelu":
            return np.where(v > 0.0, v, 0.2 * v)
        if name == "tanh":
            return np.tanh(v)
        if name == "gelu":
            if defect == "tanh_gelu":
                return 0.5 * v * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))
            return v * 0.5 * (1.0 + _erf(v * math.sqrt(0.5)))
    raise ValueError(name)


def layer_norm(y: np.ndarray, gamma, beta, defect=None) -> np.ndarray:
    n = y.shape[1]
    if defect == "pad_in_layernorm":
        n_pad = -(-n // 32) * 32
        mean = y.sum(1, keepdims=True) / n_pad
        var = (((y - mean) ** 2).sum(1, keepdims=True) + (n_pad - n) * mean ** 2) / n_pad
    else:
        mean = y.mean(1, keepdims=True)
        var = ((y - mean) ** 2).sum(1, keepdims=True) / (n - 1 if defect == "unbiased_var" else n)
    with np.errstate(invalid="ignore"):
        inv = 1.0 / (np.sqrt(var) + 1e-5) if defect == "eps_outside" else 1.0 / np.sqrt(var + 1e-5)
    return (y - mean) * inv * gamma.astype(np.float64) + beta.astype(np.float64)


def network(feat32: np.ndarray, net: dict, defect=None) -> np.ndarray:
    """``net``: the dict of ``case_network`` -> (B, num_filts) float64."""
    x = feat32.astype(np.float64)
    n = len(net["weights"])
    with np.errstate(invalid="ignore"):
        for i in range(n):
            w, b = net["weights"][i].astype(np.float64), net["biases"][i].astype(np.float64)
            y = x @ w.T + b
            last = i + 1 == n
            if not (last and defect == "no_out_act"):
                y = activation(net["act"], y, defect)
            if not last:
                if net["skip"] and w.shape[0] == w.shape[1] and defect != "noskip":
                    y = y + x
                if net["use_layn"]:
                    y = layer_norm(y, net["ln_gamma"][i], net["ln_beta"][i], defect)
            x = y
    return x


def encode(net: dict, lonlat, defect=None) -> np.ndarray:
    return network(features(net["spa_enc_type"], lonlat, net["freq_list"], defect), net, defect)


def case_network(golden, case: str) -> dict:
    """The network of a fixture case: settings, frequency table, float32 tensors - from the fixture where it
    stores them, else regenerated (tools/synth.py: make_csp_checkpoint) and checked against its digest."""
    from tools import synth
    s = json.loads(str(golden[case + "_settings"]))
    n = max(s["layers"], 0) + 1
    layn = [s["use_layn"] and i + 1 < n for i in range(n)]
    if f"{case}_w0" in golden.files:
        get = lambda k: golden[f"{case}_{k}"]                      # noqa: E731
    else:
        sd = synth.make_csp_checkpoint(**s)["state_dict"]
        names = {"w": "linear.weight", "b": "linear.bias", "g": "layernorm.weight", "be": "layernorm.bias"}

        def get(k):
            kind, i = k.rstrip("0123456789"), k[len(k.rstrip("0123456789")):]
            return sd[f"loc_enc.spa_enc.ffn.layers.{i}.{names[kind]}"].numpy()
    net = dict(settings=s, name=str(golden[case + "_name"]), spa_enc_type=s["spa_enc_type"], act=s["act"],
               skip=s["skip"], use_layn=s["use_layn"], freq_list=golden[case + "_freq_list"],
               weights=[get(f"w{i}") for i in range(n)], biases=[get(f"b{i}") for i in range(n)],
               ln_gamma=[get(f"g{i}") if layn[i] else None for i in range(n)],
               ln_beta=[get(f"be{i}") if layn[i] else None for i in range(n)])
    h = hashlib.sha256()
    for i in range(n):
        for a in (net["weights"][i], net["biases"][i], net["ln_gamma"][i], net["ln_beta"][i]):
            if a is not None:
                assert a.dtype == np.float32
                h.update(np.ascontiguousarray(a).tobytes())
    assert h.hexdigest() == str(golden[case + "_sha256"]), f"{case}: the network's tensors are not the fixture's"
    return net


def finite_rows(ref: np.ndarray) -> np.ndarray:
    return ~np.isnan(ref).any(axis=1)


def e_ref(golden, case: str, net: dict) -> float:
    """max |reference float32 - restatement float64| over the fixture's finite rows."""
    ref = golden[case + "_out"]
    rows = finite_rows(ref)
    return float(np.abs(ref[rows].astype(np.float64) - encode(net, golden["lonlat"][rows])).max())


def gpu_bound(golden, case: str, net: dict) -> float:
    """What the kernel may differ from the restatement by: 4 * max(E_ref, 2^-23 * max |out|) - two float32
    evaluations in different summation orders, each about E_ref from the exact value (x 2), and the device's
    erff / expf / tanhf against the host's (x 2); never below four float32 half-ulps of the largest output."""
    ref = golden[case + "_out"]
    return 4.0 * max(e_ref(golden, case, net), 2.0 ** -23 * float(np.nanmax(np.abs(ref))))
