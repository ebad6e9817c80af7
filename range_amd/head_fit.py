"""Fitting the CSP class head on the GPU from a frozen location encoder.

The reference's supervised stage (csp/main/trainer.py:753-797 -> trainer_helper.py:113-174) is ``embedding_loss``
(losses.py:395-470, without 'user') under ``torch.optim.Adam`` with a balanced sampler and random background
locations.  With the encoder frozen - as every encoder RANGE loads is (range/range.py:201-203) - it is a fit of the one
matrix ``class_emb``; the kernels are range_amd/csrc/headfit_kernels.h (include/range_headfit.h).  The defaults
are the reference's (trainer.py:68, 131, 191-203).

Fidelity limits, stated once:

* the SAMPLER restates ``BalancedSampler`` (utils.py:275-325: per class ``min(count, max_num_exs_per_class)`` members
  without replacement, then one shuffle) on a seeded ``numpy.random.Generator``.  The reference draws from numpy's
  GLOBAL legacy stream, and its background locations from torch's global stream; neither can be followed from
  here, so a fit reproduces the reference's distribution of batches, not its batches.  ``batches=`` takes explicit
  batches - the reference's own, recorded - and then the trajectory is the reference's within float32 rounding.
* the NEGATIVES of ``neg_rand_type='spherical'``, the reference's default, are what its code really draws: see
  ``rand_locations``.
* float32 on the GPU in the kernels' fixed orders; bounds: DESIGN.md section 3.6.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

NEG_RAND_TYPES = ("spherical", "sphericalold", "uniform", "sphere")


def rand_locations(u, neg_rand_type: str = "spherical") -> np.ndarray:
    """``rand_samples`` (losses.py:18-72) for the encoders of ``get_spa_enc_list`` on GIVEN uniforms: ``u`` (n, 3)
    float32 in [0, 1) - what the ``torch.rand(batch_size, 3)`` it uses returned (the third column, the date, is not
    used) - -> (n, 2) float32 (lon, lat) degrees, in the reference's float32 operations.

    * ``'spherical'`` (the reference's default) - what the code really does: it computes a longitude and a latitude
      on the sphere from the uniforms, DROPS them and scales the raw uniforms: lon = 180 u0 in [0, 180), lat = 90 u1 in
      [0, 90).  The negatives cover one octant of the globe.  That is reproduced here because it is the reference's
      behaviour.  (It also draws a first ``torch.rand(batch_size, 3)`` that it discards; ``u`` is the second.)
    * ``'sphericalold'``: s = 2 u - 1, theta = (s1 + 1) / 2 * 2 pi, lon = 180 sqrt(1 - s0^2) cos theta, lat = 90 sqrt(1 -
      s0^2) sin theta.
    * ``'uniform'`` (any other string there): lon = 180 (2 u0 - 1), lat = 90 (2 u1 - 1).
    * ``'sphere'`` - an EXTENSION, not in the reference: the area-uniform draw its comment describes, lon = 180 (2 u0 -
      1), lat = asin(2 u1 - 1) in degrees."""
    u = np.asarray(u)
    if u.dtype != np.float32 or u.ndim != 2 or u.shape[1] != 3:
        raise ValueError(f"u: float32 (n, 3) uniforms, got {u.dtype} {u.shape}")
    if neg_rand_type not in NEG_RAND_TYPES:
        raise ValueError(f"neg_rand_type {neg_rand_type!r}: one of {NEG_RAND_TYPES}")
    f = np.float32
    if neg_rand_type == "spherical":
        return np.stack([u[:, 0] * f(180), u[:, 1] * f(90)], axis=1)
    s = u * f(2) - f(1)
    if neg_rand_type == "sphericalold":
        theta = ((s[:, 1] + f(1)) / f(2.0)) * f(2 * np.pi)
        r = np.sqrt(f(1.0) - s[:, 0] ** 2)
        return np.stack([(r * np.cos(theta)) * f(180), (r * np.sin(theta)) * f(90)], axis=1).astype(f)
    if neg_rand_type == "sphere":
        return np.stack([s[:, 0] * f(180), np.degrees(np.arcsin(s[:, 1].astype(np.float64))).astype(f)], axis=1)
    return np.stack([s[:, 0] * f(180), s[:, 1] * f(90)], axis=1)


def balanced_indices(classes: np.ndarray, num_per_class: int, rng: np.random.Generator) -> np.ndarray:
    """One pass of ``BalancedSampler`` (utils.py:275-325, ``use_replace=False``): per class, in the order of
    ``np.unique``, ``min(count, num_per_class)`` members without replacement; then one shuffle.  On ``rng``, not on
    numpy's global stream (module docstring)."""
    classes = np.asarray(classes)
    order = np.argsort(classes, kind="stable")
    _, starts, counts = np.unique(classes[order], return_index=True, return_counts=True)
    picked = [rng.choice(order[s:s + n], min(int(n), int(num_per_class)), replace=False) for s, n in zip(starts, counts)]
    idx = np.concatenate(picked) if picked else np.zeros(0, dtype=np.int64)
    rng.shuffle(idx)
    return idx.astype(np.int64)


@dataclass
class HeadFitResult:
    weights: np.ndarray                      # (num_classes, F) float32
    train_losses: List[float]                # per epoch, the mean of the steps' losses weighted by their rows
    val_losses: Optional[List[float]]        # per epoch, trainer_helper.py's test(): mean -log(p_label + 1e-5)
    steps: int


def _labels(labels, n: int, num_classes: Optional[int]) -> Tuple[np.ndarray, int]:
    lab = labels.detach().cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
    if lab.shape != (n,) or lab.dtype.kind not in "iu":
        raise ValueError(f"labels: {n} integers, got {lab.dtype} {lab.shape}")
    C = int(lab.max()) + 1 if num_classes is None else int(num_classes)
    if n and (lab.min() < 0 or lab.max() >= C):
        raise ValueError(f"labels outside 0 .. {C - 1}: min {lab.min()}, max {lab.max()}")
    return lab.astype(np.int64), C


def _locs64(locs, what: str) -> np.ndarray:
    """``locs`` as a contiguous (n, 2) float64 array of finite (lon, lat) degrees; ``what`` names them in the refusals."""
    a = locs.detach().cpu().numpy() if torch.is_tensor(locs) else np.asarray(locs)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"{what}: (n, 2) lon / lat degrees, got {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError(f"{what}: non-finite entries")
    return np.ascontiguousarray(a, dtype=np.float64)


def _run_epochs(step: Callable, val_loss: Optional[Callable], n_val: int, N: int, lab: np.ndarray, dev, *, epochs: int,
                batch_size: int, batches, balanced: bool, max_num_exs_per_class: int, lr: float, lr_decay: float,
                rng: np.random.Generator, logger) -> Tuple[List[float], Optional[List[float]]]:
    """The epochs of a fit - this module's and csp_fit.py's: per epoch the batches (``batches[epoch]``, or the sampler
    on ``rng``), ``step(row ids on the GPU, spec, the epoch's lr)`` -> its (3,) loss scalars for each - it draws the
    step's negatives from ``rng``, behind the sampler's draw -, the mean of the losses weighted by rows, the same of
    ``val_loss(i, j)`` over the ``n_val`` validation rows in slices of ``batch_size`` (or no ``val_loss``), and the
    logger's line.  -> (train losses, validation losses or None)."""
    from ._headfit_native import MAX_ROWS
    train_losses, val_losses = [], ([] if val_loss is not None else None)
    for epoch in range(epochs):
        if batches is not None:
            plan = [(np.asarray(r, dtype=np.int64), spec) for r, spec in batches[epoch]]
        else:
            idx = balanced_indices(lab, max_num_exs_per_class, rng) if balanced else rng.permutation(N)
            plan = [(idx[i:i + batch_size], None) for i in range(0, len(idx), batch_size)]
        losses, sizes = [], []
        for rows, spec in plan:
            if rows.ndim != 1 or not 1 <= len(rows) <= MAX_ROWS or rows.min() < 0 or rows.max() >= N:
                raise ValueError(f"a batch's row ids: 1 .. {MAX_ROWS} integers in 0 .. {N - 1}")
            losses.append(step(torch.from_numpy(rows.astype(np.int32)).to(dev), spec, lr * lr_decay ** epoch))
            sizes.append(len(rows))
        per_step = torch.stack(losses)[:, 0].double().cpu().numpy()
        train_losses.append(float(np.average(per_step, weights=np.asarray(sizes, dtype=np.float64))))
        if val_loss is not None:
            vs, vn = [], []
            for i in range(0, n_val, batch_size):
                j = min(n_val, i + batch_size)
                vs.append(val_loss(i, j))
                vn.append(j - i)
            v = torch.stack(vs)[:, 2].double().cpu().numpy()
            val_losses.append(float(np.average(v, weights=np.asarray(vn, dtype=np.float64))))
        if logger is not None:
            logger.info("Epoch {}\tLoss  : {:.4f}".format(epoch, train_losses[-1]) +
                        ("\tTest loss   : {:.4f}".format(val_losses[-1]) if val_loss is not None else ""))
    return train_losses, val_losses


def fit_head_on_features(feats_dev: torch.Tensor, labels, bg_feats_fn: Callable, num_classes: Optional[int] = None, *,
                         engine=None, epochs: int = 30, batch_size: int = 1024, lr: float = 1e-3, lr_decay: float = 0.98,
                         weight_decay: float = 0.0, rand_sample_weight: float = 1.0, max_num_exs_per_class: int = 100,
                         balanced: bool = True, init="zeros", seed: int = 0, val=None, batches=None,
                         logger=None) -> HeadFitResult:
    """The loop of ``fit_class_head`` for any (N, F <= 1024) float32 features on the GPU.  ``bg_feats_fn(n, spec, rng)``
    returns the (n', F) float32 background features of a step on that GPU (or None: no background term): ``spec`` is
    the second entry of the step's pair in ``batches``, or None when the sampler drew the batch - then ``n`` background
    rows are expected, as many as the batch has (the reference's ``Bg = B``).  ``engine``: the ``HipEngine`` whose
    context holds the fit (default: one of its own on the features' GPU).  ``init``: 'zeros' or a (C, F) array.
    ``val``: (features on the GPU, labels) or None.  ``batches``: per epoch a sequence of (row ids, spec) pairs."""
    from ._headfit_native import MAX_ROWS, HeadFit
    if not torch.is_tensor(feats_dev) or feats_dev.dtype != torch.float32 or feats_dev.dim() != 2 or not feats_dev.is_cuda:
        raise ValueError("feats_dev: a (N, F) float32 tensor on the GPU")
    feats_dev = feats_dev.contiguous()
    N, F_ = feats_dev.shape
    lab, C = _labels(labels, N, num_classes)
    if batch_size < 1 or 2 * batch_size > MAX_ROWS:
        raise ValueError(f"batch_size {batch_size}: 1 .. {MAX_ROWS // 2} (batch and background rows of a step: at most {MAX_ROWS})")
    if batches is not None and len(batches) != epochs:
        raise ValueError(f"batches: {len(batches)} epochs of pairs for epochs={epochs}")
    w0 = None
    if not (isinstance(init, str) and init == "zeros"):
        if isinstance(init, str):
            raise ValueError(f"init {init!r}: 'zeros' or a ({C}, {F_}) array")
        w0 = np.asarray(init, dtype=np.float32)
    fit = HeadFit(engine if engine is not None else feats_dev.device)
    dev = fit.engine.device
    fit.begin(C, F_, w0)
    lab_dev = torch.from_numpy(lab.astype(np.int32)).to(dev)
    rng = np.random.default_rng(seed)
    val_feats = val_lab = None
    if val is not None:
        val_feats = val[0].contiguous()
        vl, _ = _labels(val[1], val_feats.shape[0], C)
        val_lab = torch.from_numpy(vl.astype(np.int32)).to(dev)

    def step(rows_dev, spec, lr_epoch):
        bg = bg_feats_fn(len(rows_dev), spec, rng)
        return fit.step(feats_dev, rows_dev, lab_dev[rows_dev.long()], bg, lr_epoch, weight=rand_sample_weight, weight_decay=weight_decay)

    train_losses, val_losses = _run_epochs(
        step, None if val is None else lambda i, j: fit.loss(val_feats[i:j], None, val_lab[i:j], None),
        0 if val is None else val_feats.shape[0], N, lab, dev, epochs=epochs, batch_size=batch_size, batches=batches, balanced=balanced,
        max_num_exs_per_class=max_num_exs_per_class, lr=lr, lr_decay=lr_decay, rng=rng, logger=logger)
    return HeadFitResult(fit.weights().cpu().numpy(), train_losses, val_losses, fit.steps)


def fit_class_head(model, train_locs, train_classes, num_classes: Optional[int] = None, *, epochs: int = 30,
                   batch_size: int = 1024, lr: float = 1e-3, lr_decay: float = 0.98, weight_decay: float = 0.0,
                   rand_sample_weight: float = 1.0, neg_rand_type: str = "spherical", max_num_exs_per_class: int = 100,
                   balanced: bool = True, init="checkpoint", seed: int = 0, val=None, batches=None,
                   logger=None) -> HeadFitResult:
    """Fit the class head of a loaded CSP model (``load_model('CSP' | 'CSP_INat', ...)`` or its ``loc_model``) on
    ``train_locs`` (N, 2) (lon, lat) degrees with ``train_classes`` (N,) and return the weights (``HeadFitResult``);
    ``model.set_class_head(result.weights)`` installs them.  The training embeddings are computed once with the
    frozen encoder, the background embeddings per step.  ``init``: 'checkpoint' (the ``class_emb`` the model was loaded
    with - ``class_head=True`` -, as the reference starts from), 'zeros', or a (C, num_filts) array.  ``val``: (locs,
    classes) or None.  ``batches``: per epoch a sequence of (row ids, background (n, 2) lon / lat degrees) pairs.
    Sampler and negatives: the module docstring."""
    if neg_rand_type not in NEG_RAND_TYPES:
        raise ValueError(f"neg_rand_type {neg_rand_type!r}: one of {NEG_RAND_TYPES}")
    loc_model = getattr(model, "loc_model", model)
    eng = loc_model._engine[0]
    dev = eng.device

    def embed(locs) -> torch.Tensor:
        return loc_model.encode(torch.from_numpy(_locs64(locs, "locations")).to(dev))

    if isinstance(init, str) and init == "checkpoint":
        head = getattr(loc_model.loc_enc, "class_emb", None)
        if head is None:
            raise ValueError("init='checkpoint': the model was loaded without class_head=True; pass init='zeros' or an array")
        init = head.weight.detach().cpu().numpy()
        if num_classes is None:
            num_classes = init.shape[0]

    def bg_feats(n, spec, rng):
        locs = spec if spec is not None else rand_locations(rng.random((n, 3), dtype=np.float32), neg_rand_type)
        return embed(locs) if len(locs) else None

    feats = embed(train_locs)
    v = None if val is None else (embed(val[0]), val[1])
    return fit_head_on_features(feats, train_classes, bg_feats, num_classes, engine=eng, epochs=epochs, batch_size=batch_size,
                                lr=lr, lr_decay=lr_decay, weight_decay=weight_decay, rand_sample_weight=rand_sample_weight,
                                max_num_exs_per_class=max_num_exs_per_class, balanced=balanced, init=init, seed=seed, val=v,
                                batches=batches, logger=logger)
