"""float64 restatement of the CSP encoder fit (range_amd/csrc/cspfit_kernels.h, range_amd/csp_fit.py) - forward,
backward, Adam and the dropout mix - and the DERIVED error bounds its tests use.  numpy only.

The arithmetic (reference: csp/main/module.py:104-132, losses.py:395-470 embedding_loss without 'user',
torch.optim.Adam), R = B + Bg rows of float32 features X_0 (tests/csp_refs.py: features):

    layer l:  Z = X W^T + b, A = act(Z), D = A * mask / (1 - p), S = D + X (live skip), Y = LayerNorm(S) (hidden, use_layn)
    head:     tests/headfit_refs.py on the embeddings E = Y of the last layer
    backward: dE = G W_c;  LayerNorm: dgamma = sum_r dY xhat, dbeta = sum_r dY, dS = rstd (g dY - mean(g dY) - xhat mean(g dY xhat));
              dX += dS (skip); dZ = dS * mask / (1 - p) * act'(Z); db = sum_r dZ; dW = dZ^T X; dX += dZ W

``defect``: a planted mistake - 'no_skip_grad' (the skip's dS not added to dX), 'act_prime_at_a' (act' evaluated at A
instead of Z), 'tanh_gelu' (GELU's tanh form, forward and derivative), 'ln_no_mean' (LayerNorm backward without the
mean(g dY) term), 'unbiased_var', 'db_mean' (db averaged over the rows), 'no_out_act' (the last layer's activation
skipped), 'mask_unscaled' (dropout without the 1 / (1 - p)), 'no_bias_correction' (Adam; headfit_refs.AdamRef).

BOUNDS, u = 2^-24, first order in u with the constants written out; every quantity x carries e_x >= |x32 - x|:

* a product chain of K fmas from 0 over operands known within e_a, e_b: (K + 1) u sum |a b| + sum (e_a |b| + |a| e_b).
* Z = chain + b: + e_b + u |Z|.  A = act(Z): L1 e_Z + 4 u |A| (+ 3 u |Z| for gelu, whose 1 + erf cancels), L1 the
  activation's Lipschitz constant (sigmoid 1/4, relu / leakyrelu / tanh 1, gelu 1.13).  D, S: one rounding each.
* LayerNorm: a sum of n float32 terms in ANY order is off by at most (n + 2) u sum |terms|; mean, the deviations d, the
  variance, rstd = (var + eps)^(-1/2) (e_var rstd / (2 (var + eps)) + 3 u rstd), xhat = d rstd, Y = xhat g + beta follow
  term by term (``_ln_forward``).
* act'(Z): L2 e_Z + 12 u, L2 bounding the second derivative (sigmoid 0.1, tanh 0.77, gelu 0.8); relu / leakyrelu: exact
  unless |Z| <= e_Z, where the two runs may sit on different sides of the kink (1, resp. 0.8).
* the backward's products and sums: the chain rule above with R (row sums), C (dE) or n (dX) terms; LayerNorm backward
  term by term (``_ln_backward``).
* head: headfit_refs' derivation with the logit's error widened by the embeddings' (``_head``).
* Adam: headfit_refs.AdamRef per tensor, its e_w fed back into the next step's forward as the parameters' uncertainty.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import numpy as np

import csp_refs
import headfit_refs as H

U = H.U
DEFECTS = ("no_skip_grad", "act_prime_at_a", "tanh_gelu", "ln_no_mean", "unbiased_var", "db_mean", "no_out_act",
           "mask_unscaled", "no_bias_correction")
LIP1 = {"sigmoid": 0.25, "relu": 1.0, "leakyrelu": 1.0, "tanh": 1.0, "gelu": 1.13}
LIP2 = {"sigmoid": 0.1, "tanh": 0.77, "gelu": 0.8}
_erf = np.vectorize(math.erf, otypes=[np.float64])


# ---- the dropout mix (include/range_cspfit.h)
def mix(x):
    x = np.asarray(x, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x


def drop_keep(seed: int, step: int, layer: int, R: int, n: int, p: float) -> np.ndarray:
    """(R, n) bool: the entries dropout keeps."""
    key = mix(mix(mix(mix(seed & 0xFFFFFFFF) ^ np.uint64((seed >> 32) & 0xFFFFFFFF)) ^ np.uint64(step & 0xFFFFFFFF)) ^ np.uint64(layer))
    rows = mix(key ^ np.arange(R, dtype=np.uint64))
    h = mix(rows[:, None] ^ np.arange(n, dtype=np.uint64)[None, :])
    return (h >> np.uint64(8)) < np.uint64(math.floor((1.0 - p) * 16777216.0))


def drop_factors(seed: int, step: int, widths, R: int, p: float, defect=None) -> Optional[List[np.ndarray]]:
    """Per layer the (R, n) factors 0 or float32(1 / (1 - p)); None for p = 0."""
    if p == 0.0:
        return None
    scale = 1.0 if defect == "mask_unscaled" else float(np.float32(1.0 / (1.0 - p)))
    return [drop_keep(seed, step, l, R, n, p) * scale for l, n in enumerate(widths)]


# ---- activations
def act(name, z, defect=None):
    return csp_refs.activation(name, z, "tanh_gelu" if defect == "tanh_gelu" else None)


def act_prime(name, z, defect=None):
    with np.errstate(over="ignore", invalid="ignore"):
        if name == "sigmoid":
            p = H.sigmoid(z)
            return p * H.one_minus_sigmoid(z)
        if name == "relu":
            return np.where(z <= 0.0, 0.0, 1.0)
        if name == "leakyrelu":
            return np.where(z > 0.0, 1.0, 0.2)
        if name == "tanh":
            return 1.0 - np.tanh(z) ** 2
        if name == "gelu":
            if defect == "tanh_gelu":
                c = math.sqrt(2.0 / math.pi)
                t = np.tanh(c * (z + 0.044715 * z ** 3))
                return 0.5 * (1.0 + t) + 0.5 * z * (1.0 - t * t) * c * (1.0 + 3 * 0.044715 * z * z)
            return 0.5 * (1.0 + _erf(z * math.sqrt(0.5))) + z * np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    raise ValueError(name)


def _e_act(name, z, a, e_z):
    return LIP1[name] * e_z + 4 * U * np.abs(a) + (3 * U * np.abs(z) if name == "gelu" else 0.0)


def _e_act_prime(name, z, e_z):
    if name in LIP2:
        return LIP2[name] * e_z + 12 * U
    return np.where(np.abs(z) <= e_z, 1.0 if name == "relu" else 0.8, 0.0)


def _chain(a, b_t, e_a, e_b_t, K):
    """Bound of the float32 chain a @ b_t over K terms."""
    return (K + 1) * U * (np.abs(a) @ np.abs(b_t)) + e_a @ np.abs(b_t) + np.abs(a) @ e_b_t


# ---- the network as the fit sees it
def net_of(p) -> dict:
    """``range_amd.csp.CspParams`` (or a csp_refs network dict) -> the dict this module works on."""
    if isinstance(p, dict):
        return p
    return dict(spa_enc_type=p.spa_enc_type, act=p.activation, skip=p.skip_connection, use_layn=p.use_layn, freq_list=p.freq_list,
                weights=p.weights, biases=p.biases, ln_gamma=p.ln_gamma, ln_beta=p.ln_beta)


def param_names(net) -> List[str]:
    n = len(net["weights"])
    out = []
    for i in range(n):
        out += [f"w{i}", f"b{i}"] + ([f"g{i}", f"be{i}"] if net["ln_gamma"][i] is not None else [])
    return out + ["class_emb"]


def get_params(net, Wc) -> Dict[str, np.ndarray]:
    out = {}
    for i in range(len(net["weights"])):
        out[f"w{i}"], out[f"b{i}"] = net["weights"][i], net["biases"][i]
        if net["ln_gamma"][i] is not None:
            out[f"g{i}"], out[f"be{i}"] = net["ln_gamma"][i], net["ln_beta"][i]
    out["class_emb"] = Wc
    return {k: np.asarray(v, dtype=np.float64) for k, v in out.items()}


def flatten(d: Dict[str, np.ndarray], net) -> np.ndarray:
    return np.concatenate([np.asarray(d[k], dtype=np.float64).ravel() for k in param_names(net)])


def _ln_forward(S, e_S, g, be, e_g, e_be, defect=None):
    n = S.shape[1]
    tree = (n + 2) * U
    mean = S.mean(1, keepdims=True)
    e_mean = e_S.mean(1, keepdims=True) + tree * np.abs(S).mean(1, keepdims=True)
    d = S - mean
    e_d = e_S + e_mean + U * np.abs(d)
    var = (d * d).sum(1, keepdims=True) / (n - 1 if defect == "unbiased_var" else n)
    e_var = (2 * np.abs(d) * e_d).mean(1, keepdims=True) + tree * var
    with np.errstate(invalid="ignore"):
        rstd = 1.0 / np.sqrt(var + 1e-5)
    e_rstd = e_var * rstd / (2 * (var + 1e-5)) + 3 * U * rstd
    xhat = d * rstd
    e_xhat = e_d * rstd + np.abs(d) * e_rstd + U * np.abs(xhat)
    Y = xhat * g + be
    e_Y = e_xhat * np.abs(g) + np.abs(xhat) * e_g + e_be + 2 * U * (np.abs(xhat * g) + np.abs(Y))
    return Y, e_Y, dict(xhat=xhat, e_xhat=e_xhat, rstd=rstd, e_rstd=e_rstd)


def _ln_backward(dY, e_dY, g, e_g, c, defect=None):
    xhat, e_xhat, rstd, e_rstd = c["xhat"], c["e_xhat"], c["rstd"], c["e_rstd"]
    n = dY.shape[1]
    tree = (n + 2) * U
    gdy = g * dY
    e_gdy = np.abs(g) * e_dY + e_g * np.abs(dY) + U * np.abs(gdy)
    m1 = gdy.mean(1, keepdims=True)
    e_m1 = e_gdy.mean(1, keepdims=True) + tree * np.abs(gdy).mean(1, keepdims=True)
    if defect == "ln_no_mean":
        m1 = np.zeros_like(m1)
    m2 = (gdy * xhat).mean(1, keepdims=True)
    e_m2 = (e_gdy * np.abs(xhat) + np.abs(gdy) * e_xhat).mean(1, keepdims=True) + tree * np.abs(gdy * xhat).mean(1, keepdims=True)
    inner = gdy - m1 - xhat * m2
    e_inner = e_gdy + e_m1 + e_xhat * np.abs(m2) + np.abs(xhat) * e_m2 + 3 * U * (np.abs(gdy) + np.abs(m1) + np.abs(xhat * m2))
    dS = rstd * inner
    e_dS = e_rstd * np.abs(inner) + rstd * e_inner + U * np.abs(dS)
    R = dY.shape[0]
    t = dY * xhat
    e_t = e_dY * np.abs(xhat) + np.abs(dY) * e_xhat + U * np.abs(t)
    dgamma, e_dgamma = t.sum(0), e_t.sum(0) + (R + 1) * U * np.abs(t).sum(0)
    dbeta, e_dbeta = dY.sum(0), e_dY.sum(0) + (R + 1) * U * np.abs(dY).sum(0)
    return dS, e_dS, dgamma, e_dgamma, dbeta, e_dbeta


def forward(net, X0, drop=None, defect=None, e_par: Optional[Dict[str, np.ndarray]] = None):
    """(E, e_E, per-layer caches): the embeddings of float32 features ``X0`` (R, in0) in float64 with their bound."""
    X = np.asarray(X0, dtype=np.float64)
    e_X = np.zeros_like(X)
    n_layers = len(net["weights"])
    caches = []
    zero = lambda a: np.zeros_like(np.asarray(a, dtype=np.float64))      # noqa: E731
    ep = e_par or {}
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(n_layers):
            W, b = np.asarray(net["weights"][l], dtype=np.float64), np.asarray(net["biases"][l], dtype=np.float64)
            e_W, e_b = ep.get(f"w{l}", zero(W)), ep.get(f"b{l}", zero(b))
            last = l + 1 == n_layers
            K = W.shape[1]
            Z = X @ W.T + b
            e_Z = _chain(X, W.T, e_X, e_W.T, K) + e_b + U * np.abs(Z)
            if last and defect == "no_out_act":
                A, e_A = Z, e_Z
            else:
                A = act(net["act"], Z, defect)
                e_A = _e_act(net["act"], Z, A, e_Z)
            m = drop[l] if drop is not None else None
            D, e_D = (A * m, m * e_A + U * np.abs(A * m)) if m is not None else (A, e_A)
            skip = (not last) and net["skip"] and W.shape[0] == W.shape[1]
            S, e_S = (D + X, e_D + e_X + U * np.abs(D + X)) if skip else (D, e_D)
            c = dict(X=X, e_X=e_X, Z=Z, e_Z=e_Z, A=A, m=m, skip=skip, W=W, e_W=e_W, last=last, ln=None)
            if not last and net["use_layn"]:
                g, be = np.asarray(net["ln_gamma"][l], dtype=np.float64), np.asarray(net["ln_beta"][l], dtype=np.float64)
                e_g, e_be = ep.get(f"g{l}", zero(g)), ep.get(f"be{l}", zero(be))
                Y, e_Y, ln = _ln_forward(S, e_S, g, be, e_g, e_be, defect)
                c.update(ln=ln, g=g, e_g=e_g)
            else:
                Y, e_Y = S, e_S
            caches.append(c)
            X, e_X = Y, e_Y
    return X, e_X, caches


def _head(E, e_E, labels, B, Wc, e_Wc, weight):
    """headfit_refs on the embeddings: its float64 results and its bounds with the logit's error widened by e_E."""
    ref = H.loss_and_grad(E[:B], labels, E[B:], Wc, weight)
    z, mask = ref["z"], ref["mask"]
    R, C = z.shape
    Wc = np.asarray(Wc, dtype=np.float64)
    dz = H.logit_bound(E, Wc) + e_E @ np.abs(Wc).T + np.abs(E) @ e_Wc.T
    p, q = H.sigmoid(z), H.one_minus_sigmoid(z)
    h, L = H.h_terms(z, mask)
    e_p = 4 * U * p
    e_q = e_p + U * q
    base, e_base = np.where(mask, p, q), np.where(mask, e_p, e_q)
    den = base + H.EPS
    e_den = e_base + U * den
    e_h = h * (e_p / p + e_q / q + e_den / den + 3 * U) + H._moved(z, dz, mask, 0)
    s = np.where(mask, abs(ref["s_lab"]), ref["s_neg"][:, None])
    G = ref["G"]
    e_G = s * e_h + U * np.abs(G)
    aE = np.abs(E)
    e_dWc = e_G.T @ aE + np.abs(G).T @ e_E + (R + 1) * U * (np.abs(G).T @ aE)
    # the loss (headfit_refs.loss_bound with this dz)
    e_L = (e_base + U * den) / den + 2 * U * np.abs(L) + H._moved(z, dz, mask, 1)
    depth = 5 + (C + 31) // 32 + (R + 255) // 256 + 8
    Lw, e_Lw = np.where(mask, C * np.abs(L), np.abs(L)), np.where(mask, C * e_L + U * C * np.abs(L), e_L)
    rows = e_Lw.sum(axis=1) + depth * U * Lw.sum(axis=1)
    Bg = R - B
    tot = rows[:B].sum() / (float(B) * C) + (abs(weight) * rows[B:].sum() / (float(Bg) * C) if Bg else 0.0)
    mag = Lw[:B].sum() / (float(B) * C) + (abs(weight) * Lw[B:].sum() / (float(Bg) * C) if Bg else 0.0)
    e_loss = float(tot + 6 * U * mag)
    dE = G @ Wc
    e_dE = e_G @ np.abs(Wc) + np.abs(G) @ e_Wc + (C + 1) * U * (np.abs(G) @ np.abs(Wc))
    return ref, dict(dWc=ref["dW"], e_dWc=e_dWc, dE=dE, e_dE=e_dE, e_loss=e_loss)


def loss_and_grads(net, Wc, X0, labels, B: int, weight: float = 1.0, drop=None, defect=None,
                   e_par: Optional[Dict[str, np.ndarray]] = None) -> dict:
    """float64: dict(loss, loss_pos, label_mean, e_loss, E, e_E, grads {name: array}, bounds {name: array})."""
    net = net_of(net)
    E, e_E, caches = forward(net, X0, drop, defect, e_par)
    Wc = np.asarray(Wc, dtype=np.float64)
    e_Wc = (e_par or {}).get("class_emb", np.zeros_like(Wc))
    ref, hd = _head(E, e_E, labels, B, Wc, e_Wc, weight)
    grads, bounds = {"class_emb": hd["dWc"]}, {"class_emb": hd["e_dWc"]}
    dY, e_dY = hd["dE"], hd["e_dE"]
    R = E.shape[0]
    name = net["act"]
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(len(caches) - 1, -1, -1):
            c = caches[l]
            if c["ln"] is not None:
                dS, e_dS, dg, e_dg, dbe, e_dbe = _ln_backward(dY, e_dY, c["g"], c["e_g"], c["ln"], defect)
                grads[f"g{l}"], bounds[f"g{l}"], grads[f"be{l}"], bounds[f"be{l}"] = dg, e_dg, dbe, e_dbe
            else:
                dS, e_dS = dY, e_dY
            if c["last"] and defect == "no_out_act":
                ap, e_ap = np.ones_like(c["Z"]), np.zeros_like(c["Z"])
            else:
                ap = act_prime(name, c["A"] if defect == "act_prime_at_a" else c["Z"], defect)
                e_ap = _e_act_prime(name, c["Z"], c["e_Z"])
            m = c["m"] if c["m"] is not None else 1.0
            dZ = dS * m * ap
            e_dZ = m * (e_dS * np.abs(ap) + np.abs(dS) * e_ap) + 2 * U * np.abs(dZ)
            X, e_X, W, e_W = c["X"], c["e_X"], c["W"], c["e_W"]
            db = dZ.sum(0)
            grads[f"b{l}"] = db / R if defect == "db_mean" else db
            bounds[f"b{l}"] = e_dZ.sum(0) + (R + 1) * U * np.abs(dZ).sum(0)
            grads[f"w{l}"] = dZ.T @ X
            bounds[f"w{l}"] = e_dZ.T @ np.abs(X) + np.abs(dZ).T @ e_X + (R + 1) * U * (np.abs(dZ).T @ np.abs(X))
            dX = dZ @ W
            e_dX = e_dZ @ np.abs(W) + np.abs(dZ) @ e_W + (W.shape[0] + 1) * U * (np.abs(dZ) @ np.abs(W))
            if c["skip"] and defect != "no_skip_grad":
                dX = dX + dS
                e_dX = e_dX + e_dS + U * np.abs(dX)
            dY, e_dY = dX, e_dX
    return dict(loss=ref["loss"], loss_pos=ref["loss_pos"], label_mean=ref["label_mean"], e_loss=hd["e_loss"], E=E, e_E=e_E,
                grads=grads, bounds=bounds, z=ref["z"], caches=caches)


def float64_loss(net, Wc, X0, labels, B, weight=1.0, drop=None) -> float:
    """The loss alone (for central differences)."""
    E, _, _ = forward(net_of(net), X0, drop)
    return H.loss_and_grad(E[:B], labels, E[B:], Wc, weight)["loss"]


class Trajectory:
    """Adam on every tensor (headfit_refs.AdamRef), the bounds carried from step to step."""

    def __init__(self, net, Wc, lr=1e-3, weight_decay=0.0, defect=None):
        self.net = dict(net_of(net))
        self.names = param_names(self.net)
        self.adam = {k: H.AdamRef(v, lr=lr, weight_decay=weight_decay, defect=defect) for k, v in get_params(self.net, Wc).items()}

    def current(self):
        n = len(self.net["weights"])
        net = dict(self.net)
        net["weights"] = [self.adam[f"w{i}"].w for i in range(n)]
        net["biases"] = [self.adam[f"b{i}"].w for i in range(n)]
        net["ln_gamma"] = [self.adam[f"g{i}"].w if f"g{i}" in self.adam else None for i in range(n)]
        net["ln_beta"] = [self.adam[f"be{i}"].w if f"be{i}" in self.adam else None for i in range(n)]
        return net, self.adam["class_emb"].w

    def e_par(self):
        return {k: a.e_w for k, a in self.adam.items()}

    def step(self, X0, labels, B, weight=1.0, drop=None, lr=None):
        net, Wc = self.current()
        r = loss_and_grads(net, Wc, X0, labels, B, weight, drop, e_par=self.e_par())
        for k, a in self.adam.items():
            a.step(r["grads"][k], r["bounds"][k], lr=lr)
        return r

    def apply(self, grads: Dict[str, np.ndarray], lr=None):
        """Adam on GIVEN float32 gradients (the same bits the float32 run used)."""
        for k, a in self.adam.items():
            a.step(grads[k], None, lr=lr)
