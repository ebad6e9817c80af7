"""numpy float64 restatement of the CSP evaluation (reference: csp/main/eval_helper.py ``compute_acc_batch`` /
``get_label_rank``) - what the tests compare csp_rank_kernel.h and range_amd/csp_eval.py with.

The rule (``rank_rule``), with scores s = p.astype(float64) * img.astype(float64) and label t:

    greater    = #{c != t : s_c > s_t or s_c is NaN}
    tied_after = #{c > t : s_c == s_t}
    rank       = 1 + greater + tied_after        argmax = np.argmax(s)

all -1 where s_t is NaN, -2 where t is outside [0, C).  ``defect``: a planted mistake for the tests that show the
checks catch it - 'ge' (>= for >), 'ties_before' (the ties before the label count, not those after), 'last_argmax'
(the last index of the maximum), 'f32_product' (the product formed in float32).

The interval (``rank_interval``): the restatement's probabilities are exact (float64 on the float32 embeddings);
a float32 evaluation - the reference's, the kernel's - is within delta (csp_head_refs.gpu_bound, 'probs') of them,
so its s_c - s_t is within delta (img_c + img_t) of the restatement's.  ``lo`` counts the classes whose score
exceeds the label's by more than that, ``hi`` those not below it by more than that: any such evaluation's rank
lies in [1 + lo, 1 + hi].  A row with lo == hi is decided.

Fixture: tests/golden/csp_rank.npz (make_golden_csp_rank.py).  Per case ``<c>`` of csp_head_refs.CASES:
``<c>_labels`` (24,) int32, ``<c>_img_kind`` ('f32', 'f64', 'none'), ``<c>_img_sha256`` (of the image predictions,
which ``inputs`` regenerates from the numpy seed), ``<c>_ranks`` (24,) int64 and ``<c>_argmax`` (24,) int64 by the
rule on the REFERENCE's probabilities (0 / -1 on the rows of a NaN location), ``<c>_topk`` (4,) the rows with rank
<= 1, 3, 5, 10."""
from __future__ import annotations

import hashlib

import numpy as np

import csp_head_refs as H

DEFECTS = ("ge", "ties_before", "last_argmax", "f32_product")
TOP_KS = (1, 3, 5, 10)
IMG_KINDS = {"design": "f32", "c_odd": "f32", "theory": "f64", "d_nohidden": "f32", "e_square": "none"}
SEEDS = {"design": 4125, "c_odd": 4102, "theory": 4103, "d_nohidden": 4104, "e_square": 4105}
MIN_DECIDED = 0.9      # of a case's finite rows: lo == hi


def inputs(case: str, C: int, B: int = 24):
    """-> (image predictions (B, C) or None, labels (B,) int32) of a fixture case, from its numpy seed: a float32
    softmax of random logits - the label's logit raised on every second row, so that the ranks spread from 1 up -
    with about a tenth of the entries set to exactly 0 (never the label's), widened to float64 for the 'f64' case."""
    rng = np.random.default_rng(SEEDS[case])
    labels = rng.integers(0, C, size=B).astype(np.int32)
    labels[0], labels[1] = 0, C - 1
    z = rng.standard_normal((B, C)) * 2.0
    z[np.arange(0, B, 2), labels[0::2]] += rng.uniform(2.0, 6.0, size=len(labels[0::2]))
    e = np.exp(z - z.max(1, keepdims=True))
    img = (e / e.sum(1, keepdims=True)).astype(np.float32)
    zero = rng.random((B, C)) < 0.1
    zero[np.arange(B), labels] = False
    img[zero] = 0.0
    kind = IMG_KINDS[case]
    if kind == "none":
        return None, labels
    return (img.astype(np.float64) if kind == "f64" else img), labels


def img_sha256(img) -> str:
    return "" if img is None else hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest()


def scores(p32, img, defect=None) -> np.ndarray:
    """(B, C) float64 scores of float32 probabilities and image predictions (None: the probabilities alone)."""
    p32 = np.asarray(p32)
    if img is None:
        return p32.astype(np.float64)
    if defect == "f32_product":
        return (p32.astype(np.float32) * np.asarray(img).astype(np.float32)).astype(np.float64)
    return p32.astype(np.float64) * np.asarray(img).astype(np.float64)


def rank_rule(s, labels, defect=None):
    """-> (greater, tied_after, argmax) int64 (B,) each, row by row in plain loops."""
    s = np.asarray(s, dtype=np.float64)
    B, C = s.shape
    out = np.zeros((3, B), dtype=np.int64)
    for b in range(B):
        t = int(labels[b])
        if t < 0 or t >= C:
            out[:, b] = -2
            continue
        row, st = s[b], s[b, t]
        if np.isnan(st):
            out[:, b] = -1
            continue
        others = np.arange(C) != t
        with np.errstate(invalid="ignore"):
            gt = (row >= st) if defect == "ge" else (row > st)
        out[0, b] = int(((gt | np.isnan(row)) & others).sum())
        eq = row == st
        out[1, b] = int(eq[:t].sum() if defect == "ties_before" else eq[t + 1:].sum())
        if np.isnan(row).any():
            out[2, b] = int(np.flatnonzero(np.isnan(row))[0])
        else:
            best = np.flatnonzero(row == row.max())
            out[2, b] = int(best[-1] if defect == "last_argmax" else best[0])
    return out[0], out[1], out[2]


def ranks_of(greater, tied_after) -> np.ndarray:
    """1 + greater + tied_after; 0 where the row is flagged."""
    g, e = np.asarray(greater).astype(np.int64), np.asarray(tied_after).astype(np.int64)
    return np.where(g < 0, 0, 1 + g + e)


def argsort_ranks(s, labels) -> np.ndarray:
    """eval_helper.py's two argsorts, as written there (the default sort)."""
    idx = np.argsort(s, axis=-1)[:, ::-1]
    return (np.argsort(idx, axis=-1) + 1)[np.arange(s.shape[0]), labels]


def stable_argsort_ranks(s, labels) -> np.ndarray:
    idx = np.argsort(s, axis=-1, kind="stable")[:, ::-1]
    return (np.argsort(idx, axis=-1, kind="stable") + 1)[np.arange(s.shape[0]), labels]


def tie_free(s) -> np.ndarray:
    """Rows of ``s`` without two equal scores and without NaN."""
    srt = np.sort(s, axis=1)
    return ~np.isnan(s).any(1) & ~(np.diff(srt, axis=1) == 0).any(1)


def rank_interval(p64, img, labels, delta: float):
    """-> (lo, hi) int64 (B,): see the module docstring.  Rows with a NaN label score: (0, C - 1)."""
    p64 = np.asarray(p64, dtype=np.float64)
    B, C = p64.shape
    g = np.ones((B, C)) if img is None else np.asarray(img).astype(np.float64)
    s = p64 * g
    rows = np.arange(B)
    st, gt_ = s[rows, labels][:, None], g[rows, labels][:, None]
    margin = delta * (g + gt_)
    others = np.arange(C)[None, :] != np.asarray(labels)[:, None]
    with np.errstate(invalid="ignore"):
        lo = ((s - st > margin) & others).sum(1)
        hi = ((s - st >= -margin) & others).sum(1)
    nan = np.isnan(st[:, 0])
    lo[nan], hi[nan] = 0, C - 1
    return lo.astype(np.int64), hi.astype(np.int64)


def argmax_decided(p64, img, delta: float) -> np.ndarray:
    """Rows whose two best restated scores differ by more than delta times the sum of their image predictions
    (a single class: decided)."""
    p64 = np.asarray(p64, dtype=np.float64)
    B, C = p64.shape
    g = np.ones((B, C)) if img is None else np.asarray(img).astype(np.float64)
    s = p64 * g
    if C == 1:
        return ~np.isnan(s[:, 0])
    with np.errstate(invalid="ignore"):
        order = np.argsort(np.where(np.isnan(s), -np.inf, s), axis=1)
    a, b = order[:, -1], order[:, -2]
    rows = np.arange(B)
    return ~np.isnan(s).any(1) & (s[rows, a] - s[rows, b] > delta * (g[rows, a] + g[rows, b]))


def topk_counts(ranks) -> np.ndarray:
    r = np.asarray(ranks)
    return np.array([int(((r >= 1) & (r <= k)).sum()) for k in TOP_KS], dtype=np.int64)


def case_inputs(rank_golden, case: str, head: dict):
    """The image predictions and labels of a fixture case, regenerated and checked against the fixture."""
    img, labels = inputs(case, head["C"])
    assert str(rank_golden[case + "_img_kind"]) == IMG_KINDS[case]
    assert img_sha256(img) == str(rank_golden[case + "_img_sha256"]), f"{case}: the image predictions are not the fixture's"
    assert np.array_equal(labels, rank_golden[case + "_labels"])
    return img, labels


def case_delta(head_golden, case: str, head: dict) -> float:
    return H.gpu_bound(head_golden, case, head, "probs")


class NumpyPrior:
    """A stand-in for ``CspLocationModel`` on the host: ``label_ranks`` by the rule on a fixed (N, C) float32 prior,
    looked up by the first coordinate (the row number); a NaN coordinate gives a NaN row."""

    def __init__(self, prior32, spa_enc_type="gridcell"):
        self.prior, self.spa_enc_type, self.calls = np.asarray(prior32, dtype=np.float32), spa_enc_type, 0

    def label_ranks(self, coords, labels, img_preds=None):
        coords = np.asarray(coords, dtype=np.float64)
        self.calls += 1
        p = np.full((len(coords), self.prior.shape[1]), np.nan, dtype=np.float32)
        ok = ~np.isnan(coords[:, 0])
        p[ok] = self.prior[coords[ok, 0].astype(np.int64)]
        g, e, a = rank_rule(scores(p, img_preds), labels)
        return ranks_of(g, e), np.where(g < 0, -1, a)
