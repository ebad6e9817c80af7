"""Training a CSP location encoder and its class head on the GPU.

The reference's supervised stage (csp/main/trainer.py:753-797 -> trainer_helper.py:113-174) is ``embedding_loss``
(losses.py:395-470, without 'user') under ``torch.optim.Adam`` on the whole ``LocationImageEncoder``: the feed-forward
net behind the 'gridcell' / 'theory' features and ``class_emb``.  The kernels are range_amd/csrc/cspfit_kernels.h
(include/range_cspfit.h); range_amd/head_fit.py fits the head alone behind a frozen encoder.

Fidelity limits, stated once:

* the SAMPLER and the NEGATIVES are head_fit.py's (its module docstring): a fit reproduces the reference's distribution
  of batches, not its batches; ``batches=`` takes explicit ones, and then - with ``dropout=0`` - the trajectory is the
  reference's within float32 rounding.
* DROPOUT masks come from the kernels' own counter-based generator (include/range_cspfit.h), a function of (seed,
  step, layer, row of the step, column) alone.  The reference's come from torch's global stream and cannot be followed.
* ``init='xavier'`` draws what the reference's constructors draw - ``xavier_uniform`` weights (module.py:98), torch's
  default ``Linear`` biases and ``class_emb`` U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)), LayerNorm 1 / 0 - on a seeded
  ``numpy.random.Generator``, not on torch's stream.
* float32 on the GPU in the kernels' fixed orders; bounds: DESIGN.md section 3.6j.
"""
from __future__ import annotations

import dataclasses
import math
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from .csp import CspParams
from .head_fit import NEG_RAND_TYPES, _labels, _locs64, _run_epochs, rand_locations


@dataclass
class CspFitResult:
    params: CspParams                        # the trained network and class_emb (CspLocationModel.set_network, save_csp_checkpoint)
    train_losses: List[float]                # per epoch, the mean of the steps' losses weighted by their rows
    val_losses: Optional[List[float]]        # per epoch, trainer_helper.py's test(): mean -log(p_label + 1e-5)
    steps: int


def xavier_params(p: CspParams, num_classes: int, seed: int) -> CspParams:
    """``p``'s architecture with freshly drawn tensors (module docstring: init='xavier')."""
    rng = np.random.default_rng(seed)
    n, d_in = len(p.widths), p.input_dim
    ws, bs, gs, bes = [], [], [], []
    for i, d_out in enumerate(p.widths):
        a = math.sqrt(6.0 / (d_in + d_out))
        ws.append(rng.uniform(-a, a, size=(d_out, d_in)).astype(np.float32))
        bs.append(rng.uniform(-1.0 / math.sqrt(d_in), 1.0 / math.sqrt(d_in), size=(d_out,)).astype(np.float32))
        has = p.use_layn and i + 1 < n
        gs.append(np.ones(d_out, dtype=np.float32) if has else None)
        bes.append(np.zeros(d_out, dtype=np.float32) if has else None)
        d_in = d_out
    a = 1.0 / math.sqrt(p.num_filts)
    head = rng.uniform(-a, a, size=(num_classes, p.num_filts)).astype(np.float32)
    return dataclasses.replace(p, weights=ws, biases=bs, ln_gamma=gs, ln_beta=bes, num_classes=num_classes, class_emb=head)


def fit_location_model(model, train_locs, train_classes, num_classes: Optional[int] = None, *, epochs: int = 30,
                       batch_size: int = 1024, lr: float = 1e-3, lr_decay: float = 0.98, weight_decay: float = 0.0,
                       rand_sample_weight: float = 1.0, neg_rand_type: str = "spherical", max_num_exs_per_class: int = 100,
                       balanced: bool = True, dropout: Optional[float] = None, init="checkpoint", seed: int = 0, val=None,
                       batches=None, logger=None) -> CspFitResult:
    """Train the network of a loaded CSP model (``load_model('CSP' | 'CSP_INat', ...)`` or its ``loc_model``) and its
    class head on ``train_locs`` (N, 2) (lon, lat) degrees with ``train_classes`` (N,); ``model.loc_model.set_network(
    result.params)`` installs the result, ``save_csp_checkpoint`` writes it.  The model itself is not changed.
    ``init``: 'checkpoint' (the tensors the model holds; its ``class_emb`` when it was loaded with ``class_head=True``,
    else a zero head) or 'xavier' (module docstring).  ``dropout``: None - the checkpoint's ``params['dropout']``.
    ``val``: (locs, classes) or None.  ``batches``: per epoch a sequence of (row ids, background (n, 2) lon / lat
    degrees) pairs.  ``seed`` drives three things at once: the sampler and the negatives' draw (one Generator), the draw of
    ``init='xavier'`` (another Generator of the same seed) and the dropout masks (with the step counter).  Sampler,
    negatives, dropout masks: the module docstring."""
    from ._cspfit_native import MAX_ROWS, CspFit
    if neg_rand_type not in NEG_RAND_TYPES:
        raise ValueError(f"neg_rand_type {neg_rand_type!r}: one of {NEG_RAND_TYPES}")
    if init not in ("checkpoint", "xavier"):
        raise ValueError(f"init {init!r}: 'checkpoint' or 'xavier'")
    loc_model = getattr(model, "loc_model", model)
    p0: CspParams = loc_model.csp_params
    eng = loc_model._engine[0]
    dev = eng.device
    locs = _locs64(train_locs, "train_locs")
    N = locs.shape[0]
    if num_classes is None and init == "checkpoint" and p0.class_emb is not None:
        num_classes = p0.num_classes
    lab, C = _labels(train_classes, N, num_classes)
    if batch_size < 1 or 2 * batch_size > MAX_ROWS:
        raise ValueError(f"batch_size {batch_size}: 1 .. {MAX_ROWS // 2} (batch and background rows of a step: at most {MAX_ROWS})")
    if batches is not None and len(batches) != epochs:
        raise ValueError(f"batches: {len(batches)} epochs of pairs for epochs={epochs}")
    drop = float(p0.dropout if dropout is None else dropout)
    if not 0.0 <= drop < 1.0:
        raise ValueError(f"dropout {drop}: in [0, 1)")
    if init == "xavier":
        start = xavier_params(p0, C, seed)
    else:
        if p0.class_emb is not None and p0.num_classes != C:
            raise ValueError(f"init='checkpoint': the model's head has {p0.num_classes} classes, the fit {C}")
        start = p0
    fit = CspFit(eng)
    fit.begin(start, C, start.class_emb)
    locs_dev = torch.from_numpy(locs).to(dev)
    lab_dev = torch.from_numpy(lab.astype(np.int32)).to(dev)
    rng = np.random.default_rng(seed)
    val_locs = val_lab = None
    if val is not None:
        val_locs = torch.from_numpy(_locs64(val[0], "val locations")).to(dev)
        vl, _ = _labels(val[1], val_locs.shape[0], C)
        val_lab = torch.from_numpy(vl.astype(np.int32)).to(dev)

    def step(rows_dev, spec, lr_epoch):
        bg = spec if spec is not None else rand_locations(rng.random((len(rows_dev), 3), dtype=np.float32), neg_rand_type)
        bg_dev = torch.from_numpy(_locs64(bg, "background locations")).to(dev) if len(bg) else None
        return fit.step(locs_dev, rows_dev, lab_dev[rows_dev.long()], bg_dev, lr_epoch, weight=rand_sample_weight,
                        weight_decay=weight_decay, dropout=drop, seed=seed)

    train_losses, val_losses = _run_epochs(          # (validation in eval mode: no dropout)
        step, None if val is None else lambda i, j: fit.loss(val_locs[i:j], None, val_lab[i:j], None),
        0 if val is None else val_locs.shape[0], N, lab, dev, epochs=epochs, batch_size=batch_size, batches=batches, balanced=balanced,
        max_num_exs_per_class=max_num_exs_per_class, lr=lr, lr_decay=lr_decay, rng=rng, logger=logger)
    return CspFitResult(fit.trained(), train_losses, val_losses, fit.steps)
