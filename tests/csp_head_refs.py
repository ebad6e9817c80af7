"""numpy float64 restatement of the reference's CSP class head (csp/main/models.py:135-173: ``class_emb``, a
bias-free ``Linear(num_filts, num_classes)``, then a sigmoid), of ``model(x).sum(1)`` and of the range map of
grid_predictor.py - what the tests compare csp_head_kernel.h and range_amd/grid_predictor.py with.

The head is restated ON the float32 embeddings it is given (the reference's own, recorded in
tests/golden/csp_encoders.npz): float32 embeddings and float32 weights widened exactly, the products, sums
and the sigmoid in float64 - the exact value both float32 evaluations (the reference's, the kernel's)
approximate.  The map is restated from the coordinates (csp_refs.encode, then the head).

``defect``: a planted mistake (None: none) for the tests that show the bounds catch it - 'bias' (a bias
added to the logits), 'no_sigmoid' (the probabilities left as logits), 'sigmoid_in_eval' (eval_single_class
squashed), 'row_plus' / 'row_minus' (class c + 1 / c - 1), 'transposed' (W^T indexed as W, where num_filts =
num_classes), 'sum_padded' (the sum runs over the columns that pad num_classes to a multiple of 32).

Fixture: tests/golden/csp_head.npz (make_golden_csp_head.py).  Per case ``<c>``: ``<c>_settings``,
``<c>_name``, ``<c>_sha256`` (of class_emb), ``<c>_cols`` (the class ids whose columns ``<c>_probs`` holds),
``<c>_probs`` (24, len(cols)), ``<c>_classes`` (the ids asked for one at a time), ``<c>_single`` (24, n)
``loc_model(q, class_of_interest=c)``, ``<c>_logits`` (24, n) ``eval_single_class(feats, c)``, ``<c>_sums`` (24,)
over ALL classes; ``grid_*``: the 7 x 12 map."""
from __future__ import annotations

import hashlib
import json

import numpy as np

import csp_refs as R

DEFECTS = ("bias", "no_sigmoid", "sigmoid_in_eval", "row_plus", "row_minus", "transposed", "sum_padded")
# head case -> the case of csp_encoders.npz whose network (and recorded embeddings) it sits behind
CASES = {"design": "a_design", "c_odd": "c_odd", "theory": "b_theory", "d_nohidden": "d_nohidden", "e_square": "c_odd"}
# what make_csp_checkpoint gets beyond the encoder case's settings.  class_scale: class_emb ~ N(0, 1) would
# put |logits| far beyond 3 - the sigmoid saturates and hides a defect; make_golden_csp_head.py asserts that
# at least a quarter of every case's recorded probabilities lie in [0.05, 0.95]
HEAD_SETTINGS = {"design": dict(num_classes=8142, class_scale=0.25), "c_odd": dict(num_classes=5, class_scale=0.5),
                 "theory": dict(num_classes=33, class_scale=0.125), "d_nohidden": dict(num_classes=1, class_scale=0.5),
                 "e_square": dict(num_classes=24, class_scale=0.5)}
DESIGN_COLS_PER_PASS = 256      # csp_head_plan(256, ...).cols_per_pass: the design case's stored columns sit around its multiples
GRID_CASE, GRID_CLASS, GRID_SHAPE = "theory", 7, (7, 12)
KINDS = ("probs", "single", "logits", "sums")


def stored_columns(C: int, per_pass: int = DESIGN_COLS_PER_PASS, edge: int = 40) -> np.ndarray:
    """All columns of a small head; of a large one the first and last ``edge`` and the two on either side of
    every multiple of ``per_pass``."""
    if C <= 4 * edge:
        return np.arange(C, dtype=np.int32)
    cols = set(range(edge)) | set(range(C - edge, C))
    for m in range(per_pass, C, per_pass):
        cols |= {m - 1, m}
    return np.array(sorted(cols), dtype=np.int32)


def single_classes(C: int) -> np.ndarray:
    """The classes asked for one at a time: the first, the last, and a few between."""
    return np.array(sorted({0, C - 1, C // 2, min(C - 1, 31), min(C - 1, 32), min(C - 1, DESIGN_COLS_PER_PASS)}), dtype=np.int32)


def sigmoid(v: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore", invalid="ignore"):
        return 1.0 / (1.0 + np.exp(-v))


def _bias(ids: np.ndarray) -> np.ndarray:
    return 0.01 * (1 + ids % 3)


def logits(feats32, W32, ids=None, defect=None) -> np.ndarray:
    """(B, M) float64: column j is class ids[j] (None: all classes)."""
    x, W = np.asarray(feats32).astype(np.float64), np.asarray(W32).astype(np.float64)
    C = W.shape[0]
    ids = np.arange(C) if ids is None else np.asarray(ids, dtype=np.int64)
    if defect == "row_plus":
        ids = (ids + 1) % C
    elif defect == "row_minus":
        ids = (ids - 1) % C
    if defect == "transposed" and W.shape[0] == W.shape[1]:
        W = W.T
    with np.errstate(invalid="ignore"):
        out = x @ W[ids].T
    return out + _bias(ids)[None, :] if defect == "bias" else out


def probs(feats32, W32, ids=None, defect=None) -> np.ndarray:
    """``loc_model(x)`` / ``loc_model(x, class_of_interest=ids)``, (B, M) float64."""
    z = logits(feats32, W32, ids, defect)
    return z if defect == "no_sigmoid" else sigmoid(z)


def eval_single_class(feats32, W32, ids, defect=None) -> np.ndarray:
    """``eval_single_class(feats, c)``: raw logits, (B, M) float64."""
    z = logits(feats32, W32, ids, defect)
    return sigmoid(z) if defect == "sigmoid_in_eval" else z


def sums(feats32, W32, defect=None) -> np.ndarray:
    """``loc_model(x).sum(1)``, (B,) float64."""
    p = probs(feats32, W32, None, defect)
    s = p.sum(1)
    if defect == "sum_padded":
        s = s + 0.5 * (-W32.shape[0] % 32)           # sigmoid(0) for every padding column
    return s


def grid_coords(H: int, W: int):
    """numpy's restatement of the reference's grid: float32 linspace, the product in float32, widened."""
    import torch
    lon = (torch.linspace(-1, 1, W) * 180).numpy().astype(np.float64)
    lat = (torch.linspace(1, -1, H) * 90).numpy().astype(np.float64)
    return lon, lat


def grid_map(net: dict, W32, cls: int, H: int, Wd: int, defect=None) -> np.ndarray:
    """The (H, W) float64 map of class ``cls``: the encoder's restatement at every grid point, then the head."""
    lon, lat = grid_coords(H, Wd)
    q = np.stack([np.tile(lon[None, :], (H, 1)), np.tile(lat[:, None], (1, Wd))], -1).reshape(-1, 2)
    emb32 = R.encode(net, q).astype(np.float32)
    return probs(emb32, W32, [cls], defect)[:, 0].reshape(H, Wd)


def grid_sums(net: dict, W32, H: int, Wd: int) -> np.ndarray:
    """The (H, W) float64 sum of all classes' probabilities at every grid point."""
    lon, lat = grid_coords(H, Wd)
    q = np.stack([np.tile(lon[None, :], (H, 1)), np.tile(lat[:, None], (1, Wd))], -1).reshape(-1, 2)
    return sums(R.encode(net, q).astype(np.float32), W32).reshape(H, Wd)


def mask_lines(mask: np.ndarray) -> np.ndarray:
    g = np.gradient(mask)
    lines = g[0] ** 2 + g[1] ** 2
    lines[lines > 0.0] = 1.0
    return lines


def case_settings(enc_golden, case: str) -> dict:
    return dict(json.loads(str(enc_golden[CASES[case] + "_settings"])), **HEAD_SETTINGS[case])


def case_head(enc_golden, head_golden, case: str) -> dict:
    """The head of a fixture case: its settings, class_emb (regenerated from the numpy seed, tools/synth.py, and
    checked against the fixture's digest), the encoder case's network and the reference's recorded embeddings."""
    from tools import synth
    s = case_settings(enc_golden, case)
    assert json.loads(str(head_golden[case + "_settings"])) == s
    W = synth.make_csp_checkpoint(**s)["state_dict"]["loc_enc.class_emb.weight"].numpy()
    assert W.dtype == np.float32 and W.shape == (s["num_classes"], s["num_filts"])
    assert hashlib.sha256(np.ascontiguousarray(W).tobytes()).hexdigest() == str(head_golden[case + "_sha256"]), \
        f"{case}: class_emb is not the fixture's"
    enc_case = CASES[case]
    return dict(settings=s, name=str(head_golden[case + "_name"]), W=W, C=s["num_classes"], enc_case=enc_case,
                feats=enc_golden[enc_case + "_out"], cols=head_golden[case + "_cols"], classes=head_golden[case + "_classes"])


def finite_rows(feats: np.ndarray) -> np.ndarray:
    return ~np.isnan(feats).any(axis=1)


def restated(head: dict, kind: str, defect=None) -> np.ndarray:
    """The restatement of one recorded output kind, on the fixture's embeddings (all 24 rows)."""
    f, W = head["feats"], head["W"]
    if kind == "probs":
        return probs(f, W, head["cols"], defect)
    if kind == "single":
        return probs(f, W, head["classes"], defect)
    if kind == "logits":
        return eval_single_class(f, W, head["classes"], defect)
    if kind == "sums":
        return sums(f, W, defect)
    raise ValueError(kind)


def e_ref(head_golden, case: str, head: dict, kind: str) -> float:
    """max |reference float32 - restatement float64| over the fixture's finite rows."""
    rows = finite_rows(head["feats"])
    ref = head_golden[f"{case}_{kind}"]
    return float(np.abs(ref[rows].astype(np.float64) - restated(head, kind)[rows]).max())


def gpu_bound(head_golden, case: str, head: dict, kind: str) -> float:
    """What the kernel may differ from the restatement by.  probs / single / logits: 4 * max(E_ref, 2^-23 max|out|)
    - two float32 evaluations in different orders (x 2), the device's expf against the host's (x 2) - as
    csp_refs.gpu_bound.  sums: C times the bound of 'probs' (every term may be off by it) plus (C - 1) 2^-24
    sum|p| for the float32 additions, sum|p| the largest recorded row sum."""
    rows = finite_rows(head["feats"])
    if kind == "sums":
        C = head["C"]
        s = float(np.abs(head_golden[case + "_sums"][rows]).max())
        return C * gpu_bound(head_golden, case, head, "probs") + (C - 1) * 2.0 ** -24 * s
    ref = head_golden[f"{case}_{kind}"]
    return 4.0 * max(e_ref(head_golden, case, head, kind), 2.0 ** -23 * float(np.abs(ref[rows]).max()))


def grid_e_ref(head_golden, net: dict, head: dict) -> float:
    H, Wd = GRID_SHAPE
    return float(np.abs(head_golden["grid_map"].astype(np.float64) - grid_map(net, head["W"], GRID_CLASS, H, Wd)).max())


def grid_bound(head_golden, net: dict, head: dict) -> float:
    return 4.0 * max(grid_e_ref(head_golden, net, head), 2.0 ** -23 * float(np.abs(head_golden["grid_map"]).max()))


def grid_sum_bound(head_golden, net: dict, head: dict) -> float:
    """The rule of 'sums' on the grid: C times the map's bound plus the float32 additions."""
    C = head["C"]
    return C * grid_bound(head_golden, net, head) + (C - 1) * 2.0 ** -24 * float(np.abs(head_golden["grid_sum"]).max())
