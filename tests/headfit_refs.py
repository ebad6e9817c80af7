"""float64 restatement of the class-head fit (range_amd/csrc/headfit_kernels.h, range_amd/head_fit.py) and the
DERIVED error bounds its tests use.  numpy only.

The arithmetic (reference: csp/main/losses.py:395-470 embedding_loss without 'user', torch.optim.Adam):

    z = x W^T, p = sigmoid(z);  loss = mean_{B x C}(Lpos) + weight * mean_{Bg x C}(Lbg)
    Lbg = -log(1 - p + 1e-5);   Lpos the same, at the label's column -C log(p + 1e-5)

``defect``: a planted mistake for the tests that show the bounds catch it - 'no_label' (the label's column is not
overwritten), 'no_eps' (the 1e-5 dropped), 'div_B' (mean over B instead of B C), 'weight_on_batch' (the background
weight applied to the batch rows instead), 'no_bias_correction' (Adam without its bias corrections).

BOUNDS, u = 2^-24 (float32 unit roundoff), all first order in u with the constants written out:

* logit: a chain of K fused multiply-adds from 0 has |z32 - z| <= (K + 1) u sum_k |x_k w_k| (``logit_bound``).
* h(z), the factor of dL/dz behind the scale (``h_terms``): p = 1 / (1 + exp(-z)) in float32 is off by at most 4 u p
  (exp 2 ulp, the addition, the division), q = 1 - p by that plus u q, den = q + 1e-5 (or p + 1e-5) by that plus
  u den, the quotient p q / den by the three relative errors plus 3 u.  The logit's error moves h by at most
  max |h(z +- dz) - h(z)|, evaluated with the restatement itself (h is monotone between its extremum and either side;
  the extremum lies at |z| > 5.7 for the negatives, and the three-point maximum is what the saturated test spans).
* G = s h: one more rounding.  dW = G^T X is a chain of R fmas: sum_r e_G |x| + (R + 1) u sum_r |G x| (``grad_bound``).
* loss: a term -log(den) is off by e_den / den (the argument) + 2 u |L| (logf) + max |L(z +- dz) - L(z)|; the sums
  are float32 additions in a fixed order whose longest chain is 5 (lane tree) + C / 32 (tiles) + R / 256 + 8 (rows):
  depth * u * sum |terms|; the scales and the final additions 6 u (``loss_bound``).
* Adam (``AdamRef``): the handful of float32 operations of one element, propagated to first order, and carried over
  the steps through the moments.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

U = 2.0 ** -24
EPS = 1e-5
DEFECTS = ("no_label", "no_eps", "div_B", "weight_on_batch", "no_bias_correction")


def sigmoid(z: np.ndarray) -> np.ndarray:
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def one_minus_sigmoid(z: np.ndarray) -> np.ndarray:
    return sigmoid(-np.asarray(z, dtype=np.float64))


def label_mask(labels: np.ndarray, R: int, C: int) -> np.ndarray:
    """(R, C) bool: the label's column of the batch rows (a label outside 0 .. C - 1 matches no column)."""
    labels = np.asarray(labels)
    mask = np.zeros((R, C), dtype=bool)
    ok = (labels >= 0) & (labels < C)
    mask[np.nonzero(ok)[0], labels[ok]] = True
    return mask


def h_terms(z: np.ndarray, mask: np.ndarray, eps: float = EPS) -> Tuple[np.ndarray, np.ndarray]:
    """(h, L) elementwise: dLterm/dz up to the scale's sign and the loss term, negatives and (``mask``) label columns:
    negatives h = p q / (q + eps), L = -log(q + eps); label h = p q / (p + eps), L = -log(p + eps)."""
    p, q = sigmoid(z), one_minus_sigmoid(z)
    den = np.where(mask, p, q) + eps
    return p * q / den, -np.log(den)


def scales(B: int, Bg: int, C: int, weight: float, defect: Optional[str] = None) -> Tuple[np.ndarray, float]:
    """(per-row scale of the negatives (B + Bg,), scale of the label column): dL/dz = scale * h."""
    n_pos = float(B) if defect == "div_B" else float(B) * C
    w_pos, w_bg = (weight, 1.0) if defect == "weight_on_batch" else (1.0, weight)
    s = np.concatenate([np.full(B, w_pos / n_pos), np.full(Bg, w_bg / (float(Bg) * C) if Bg else 0.0)])
    return s, -float(C) * w_pos / n_pos


def loss_and_grad(X, labels, Xbg, W, weight: float = 1.0, defect: Optional[str] = None, z_shift=None):
    """float64: dict(loss, loss_pos, label_mean, dW (C, F), G (R, C), z (R, C), L (R, C) weighted loss terms' raw values).
    ``X`` (B, F), ``Xbg`` (Bg, F) or None, ``W`` (C, F); ``z_shift``: added to the logits (the saturated test)."""
    X = np.asarray(X, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    B, C = X.shape[0], W.shape[0]
    Xall = X if Xbg is None or len(Xbg) == 0 else np.concatenate([X, np.asarray(Xbg, dtype=np.float64)])
    R = Xall.shape[0]
    Bg = R - B
    z = Xall @ W.T
    if z_shift is not None:
        z = z + z_shift
    mask = label_mask(labels, R, C) if defect != "no_label" else np.zeros((R, C), dtype=bool)
    h, L = h_terms(z, mask, 0.0 if defect == "no_eps" else EPS)
    s_neg, s_lab = scales(B, Bg, C, weight, defect)
    G = np.where(mask, s_lab * h, s_neg[:, None] * h)
    Lw = np.where(mask, C * L, L)
    n_pos = float(B) if defect == "div_B" else float(B) * C
    w_pos, w_bg = (weight, 1.0) if defect == "weight_on_batch" else (1.0, weight)
    loss_pos = Lw[:B].sum() / n_pos
    loss_bg = Lw[B:].sum() / (float(Bg) * C) if Bg else 0.0
    lab_rows = mask[:B].any(axis=1)
    label_mean = float(np.where(mask[:B], L[:B], 0.0).sum() / B)
    return dict(loss=w_pos * loss_pos + w_bg * loss_bg, loss_pos=loss_pos, label_mean=label_mean, dW=G.T @ Xall, G=G, z=z,
                L=L, mask=mask, Xall=Xall, s_neg=s_neg, s_lab=s_lab, lab_rows=lab_rows)


def logit_bound(Xall: np.ndarray, W: np.ndarray) -> np.ndarray:
    """(R, C): |z32 - z| of a K-term float32 fma chain."""
    K = Xall.shape[1]
    return (K + 1) * U * (np.abs(Xall) @ np.abs(np.asarray(W, dtype=np.float64)).T)


def _moved(z, dz, mask, which: int):
    """max |f(z +- dz) - f(z)| of h (which = 0) or L (1), with the restatement's own functions."""
    f0 = h_terms(z, mask)[which]
    return np.maximum(np.abs(h_terms(z + dz, mask)[which] - f0), np.abs(h_terms(z - dz, mask)[which] - f0))


def _dz(ref: dict, W, e_W=None) -> np.ndarray:
    """The logit's error: the chain's, plus |x| e_W^T where the float32 run's weights are only known within e_W."""
    dz = logit_bound(ref["Xall"], W)
    return dz if e_W is None else dz + np.abs(ref["Xall"]) @ np.asarray(e_W).T


def g_bound(ref: dict, W, e_W=None) -> np.ndarray:
    """(R, C): bound on |G32 - G| (module docstring)."""
    z, mask = ref["z"], ref["mask"]
    dz = _dz(ref, W, e_W)
    p, q = sigmoid(z), one_minus_sigmoid(z)
    h, _ = h_terms(z, mask)
    e_p = 4 * U * p
    e_q = e_p + U * q
    base, e_base = np.where(mask, p, q), np.where(mask, e_p, e_q)
    den = base + EPS
    e_den = e_base + U * den
    e_h = h * (e_p / p + e_q / q + e_den / den + 3 * U) + _moved(z, dz, mask, 0)
    s = np.where(mask, abs(ref["s_lab"]), ref["s_neg"][:, None])
    return s * e_h + U * np.abs(ref["G"])


def grad_bound(ref: dict, W, e_W=None) -> np.ndarray:
    """(C, F): bound on |dW32 - dW|; ``e_W``: the float32 run's weights differ from ``W`` by at most this."""
    R = ref["Xall"].shape[0]
    ax = np.abs(ref["Xall"])
    return g_bound(ref, W, e_W).T @ ax + (R + 1) * U * (np.abs(ref["G"]).T @ ax)


def loss_bound(ref: dict, W, B: int, weight: float, e_W=None) -> float:
    """Bound on |loss32 - loss| (the same rule bounds loss_pos; label_mean: its own terms only, covered too)."""
    z, mask, L = ref["z"], ref["mask"], ref["L"]
    R, C = z.shape
    dz = _dz(ref, W, e_W)
    p, q = sigmoid(z), one_minus_sigmoid(z)
    e_base = np.where(mask, 4 * U * p, 4 * U * p + U * q)
    den = np.where(mask, p, q) + EPS
    e_L = (e_base + U * den) / den + 2 * U * np.abs(L) + _moved(z, dz, mask, 1)
    depth = 5 + (C + 31) // 32 + (R + 255) // 256 + 8
    Lw, e_Lw = np.where(mask, C * np.abs(L), np.abs(L)), np.where(mask, C * e_L + U * C * np.abs(L), e_L)
    rows = e_Lw.sum(axis=1) + depth * U * Lw.sum(axis=1)
    Bg = R - B
    tot = rows[:B].sum() / (float(B) * C) + (abs(weight) * rows[B:].sum() / (float(Bg) * C) if Bg else 0.0)
    mag = Lw[:B].sum() / (float(B) * C) + (abs(weight) * Lw[B:].sum() / (float(Bg) * C) if Bg else 0.0)
    return float(tot + 6 * U * mag)


class AdamRef:
    """torch.optim.Adam (no amsgrad) in float64 on one tensor, with the first-order bound of a float32 run of the same
    steps carried along: ``e_w``, ``e_m``, ``e_v`` bound |float32 state - this state| elementwise."""

    def __init__(self, W, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, defect: Optional[str] = None):
        self.w = np.array(W, dtype=np.float64)
        self.m, self.v = np.zeros_like(self.w), np.zeros_like(self.w)
        self.e_w, self.e_m, self.e_v = np.zeros_like(self.w), np.zeros_like(self.w), np.zeros_like(self.w)
        self.lr, self.b1, self.b2, self.eps, self.wd, self.t, self.defect = lr, beta1, beta2, eps, weight_decay, 0, defect

    def step(self, g, e_g=None, lr: Optional[float] = None) -> None:
        """``g``: the gradient (float64 view of what the float32 run used, or the restatement's); ``e_g``: bound on the
        difference between the float32 run's gradient and ``g`` (None: 0 - the same bits)."""
        lr = self.lr if lr is None else lr
        g = np.asarray(g, dtype=np.float64)
        e_g = np.zeros_like(g) if e_g is None else e_g
        self.t += 1
        if self.wd:
            e_g = e_g + self.wd * self.e_w + 2 * U * (np.abs(g) + self.wd * np.abs(self.w))
            g = g + self.wd * self.w
        m = self.m + (g - self.m) * (1 - self.b1)
        e_m = self.b1 * self.e_m + (1 - self.b1) * e_g + 3 * U * (np.abs(g) + np.abs(self.m))
        v = self.v * self.b2 + (1 - self.b2) * g * g
        e_v = self.b2 * self.e_v + (1 - self.b2) * (2 * np.abs(g) * e_g + e_g * e_g) + 4 * U * v
        bc1 = bc2 = 1.0
        if self.defect != "no_bias_correction":
            bc1, bc2 = 1 - self.b1 ** self.t, 1 - self.b2 ** self.t
        step_size, bc2s = lr / bc1, np.sqrt(bc2)
        sq = np.sqrt(v)
        # |sqrt(v32) - sqrt(v)| <= e_v / sqrt(v) where v > e_v, else sqrt(v + e_v)
        e_sq = np.where(v > 4 * e_v, e_v / np.maximum(sq, 1e-300), np.sqrt(v + e_v)) + U * sq
        denom = sq / bc2s + self.eps
        e_den = e_sq / bc2s + 3 * U * denom
        den_lo = np.maximum(denom - e_den, self.eps * (1 - 4 * U))          # the float32 denominator is at least this
        upd = step_size * m / denom
        e_upd = step_size * (e_m / den_lo + np.abs(m) * e_den / (denom * den_lo)) + 4 * U * np.abs(upd)
        # no Adam step is longer than lr max(1, (1 - b1) / sqrt(1 - b2)) (Kingma & Ba, section 2.1), so two runs' steps
        # differ by at most twice that - what is left of the bound where a gradient entry is too small to have a sign
        e_upd = np.minimum(e_upd, 2.0 * (1 + 8 * U) * lr * max(1.0, (1 - self.b1) / np.sqrt(1 - self.b2)))
        self.w = self.w - upd
        self.e_w = self.e_w + e_upd + U * (np.abs(self.w) + np.abs(upd))
        self.m, self.v, self.e_m, self.e_v = m, v, e_m, e_v


def balanced_epoch_stats(indices: np.ndarray, classes: np.ndarray, num_per_class: int) -> bool:
    """What one pass of the reference's BalancedSampler (csp/main/utils.py:275-325, no replacement) guarantees: per
    class min(count, num_per_class) DISTINCT members, nothing else."""
    indices, classes = np.asarray(indices), np.asarray(classes)
    if len(np.unique(indices)) != len(indices):
        return False
    got = np.bincount(classes[indices], minlength=classes.max() + 1)
    want = np.minimum(np.bincount(classes, minlength=classes.max() + 1), num_per_class)
    return bool((got == want).all())


def rand_locations64(u: np.ndarray, neg_rand_type: str) -> np.ndarray:
    """float64 restatement of what losses.py:18-72 rand_samples returns for the encoders of get_spa_enc_list, from
    the (n, 3) uniforms of the draw it uses: 'spherical' keeps the RAW uniforms (the longitude and latitude it
    computes from them are dropped), so lon = 180 u0, lat = 90 u1."""
    u = np.asarray(u, dtype=np.float64)
    if neg_rand_type == "spherical":
        return np.stack([u[:, 0] * 180.0, u[:, 1] * 90.0], axis=1)
    s = u * 2.0 - 1.0
    if neg_rand_type == "sphericalold":
        theta = (s[:, 1] + 1.0) / 2.0 * (2.0 * np.pi)
        r = np.sqrt(1.0 - s[:, 0] ** 2)
        return np.stack([r * np.cos(theta) * 180.0, r * np.sin(theta) * 90.0], axis=1)
    if neg_rand_type == "sphere":           # the project's extension: area-uniform on the sphere
        return np.stack([s[:, 0] * 180.0, np.degrees(np.arcsin(s[:, 1]))], axis=1)
    return np.stack([s[:, 0] * 180.0, s[:, 1] * 90.0], axis=1)          # 'uniform'
