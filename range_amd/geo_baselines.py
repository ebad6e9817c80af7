"""The location-only baselines of the CSP evaluation (reference: location_models/csp/main/baselines.py
``compute_neighbor_prior`` / ``GridPrior``, trainer.py's train-frequency prior, eval_helper.py
``get_cross_val_hyper_params``): ``train_freq``, ``nn_dist``, ``nn_knn``, ``grid`` and ``kde``
(``create_kde_grid`` / ``kde_prior``: ``KdePrior``, csrc/kde_kernel.h - per-class sums of Gaussian weights as 64-bit
fixed-point integers, so that the result depends on no order).

Locations are (lon, lat) DEGREES, as everywhere in this project.  ``NeighborPrior`` plays the part of the
reference's ``BallTree``: it installs the training set on the GPU once and answers queries with one scan
(csrc/neighbor_kernel.h) - class votes in LDS, three integers per sample for the ranks, the (B, num_classes)
prior only on request.  The host forms what is formed once: radians (``np.deg2rad``), the radius threshold on the
reduced distance (``sin(dist_thresh / 2) ** 2`` for haversine, ``dist_thresh ** 2`` otherwise) and the grid cells,
with numpy and in the reference's expressions.  There is no CPU path for the scans.

Deviations: among equally distant training points ``nn_knn`` takes the lower index (``BallTree``
leaves it unspecified); a grid query outside the grid raises ValueError naming the row (the reference raises
IndexError, or wraps a negative index silently); a NaN longitude gives the uniform prior as in the reference, a
NaN latitude with a valid longitude the uniform prior for the neighbour priors and ValueError for the grid."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _neighbors_native as _nn

PTYPES = {"distance": _nn.RADIUS, "knn": _nn.KNN}

#: eval_helper.py ``get_cross_val_hyper_params``: (dataset, meta_type or None) -> settings
CROSS_VAL_HYPER_PARAMS = {
    ("inat_2018", None): dict(num_neighbors=1500, dist_type="euclidean", dist_thresh=2.0, gp_size=[180, 60], pseudo_count=2,
                              kde_dist_type="euclidean", kde_quant=5.0, kde_nb=700),
    ("inat_2017", None): dict(num_neighbors=1450, dist_type="euclidean", dist_thresh=5.0, gp_size=[45, 30], pseudo_count=2,
                              kde_dist_type="euclidean", kde_quant=5.0, kde_nb=700),
    ("birdsnap", "ebird_meta"): dict(num_neighbors=700, dist_type="euclidean", dist_thresh=5.0, gp_size=[30, 30],
                                     pseudo_count=2, kde_dist_type="euclidean", kde_quant=0.001, kde_nb=500),
    ("birdsnap", "orig_meta"): dict(num_neighbors=100, dist_type="euclidean", dist_thresh=9.0, gp_size=[225, 60],
                                    pseudo_count=2, kde_dist_type="euclidean", kde_quant=0.001, kde_nb=600),
    ("nabirds", None): dict(num_neighbors=500, dist_type="euclidean", dist_thresh=6.0, gp_size=[45, 60], pseudo_count=2,
                            kde_dist_type="euclidean", kde_quant=0.001, kde_nb=600),
    ("yfcc", None): dict(num_neighbors=75, dist_type="haversine", dist_thresh=2.0 / 6371.4, gp_size=[540, 150],
                         pseudo_count=3, kde_dist_type="euclidean", kde_quant=0.001, kde_nb=300),
}


def get_cross_val_hyper_params(dataset, meta_type: Optional[str] = None) -> Dict:
    """The reference's table; ``dataset`` a name or its ``eval_params`` dict.  An unknown dataset gives {}."""
    if isinstance(dataset, dict):
        dataset, meta_type = dataset["dataset"], dataset.get("meta_type")
    key = (dataset, meta_type if dataset == "birdsnap" else None)
    return {k: (list(v) if isinstance(v, list) else v) for k, v in CROSS_VAL_HYPER_PARAMS.get(key, {}).items()}


def train_freq_prior(train_classes, num_classes: int) -> np.ndarray:
    """trainer.py's train-frequency prior: ``(1 + count) / sum`` over the classes, (num_classes,) float64."""
    cls_id, cls_cnt = np.unique(np.asarray(train_classes), return_counts=True)
    prior = np.ones(num_classes)
    prior[cls_id] += cls_cnt
    prior /= prior.sum()
    return prior


def radius_threshold(dist_thresh: float, haversine: bool) -> float:
    """What ``query_radius(r)`` compares the reduced distance with."""
    r = np.float64(dist_thresh)
    return float(np.sin(0.5 * r) ** 2) if haversine else float(r * r)


def train_cells(locs, lon_bins: int, lat_bins: int) -> np.ndarray:
    """The cell ``lat_bin * lon_bins + lon_bin`` into which ``np.histogram2d`` with the reference's edges bins a
    training point: the last edge closed, -2 for a point outside (or NaN)."""
    locs = np.asarray(locs, dtype=np.float64)
    x = (locs[:, 0] + 180) / 360.0
    x *= lon_bins
    y = (locs[:, 1] + 90) / 180.0
    y *= lat_bins
    with np.errstate(invalid="ignore"):
        inside = (x >= 0) & (x <= lon_bins) & (y >= 0) & (y <= lat_bins)
        xi = np.minimum(np.floor(np.where(inside, x, 0.0)).astype(np.int64), lon_bins - 1)
        yi = np.minimum(np.floor(np.where(inside, y, 0.0)).astype(np.int64), lat_bins - 1)
    return np.where(inside, yi * lon_bins + xi, _nn.CELL_OUTSIDE).astype(np.int32)


def query_cells(locs, lon_bins: int, lat_bins: int) -> np.ndarray:
    """The cell ``GridPrior.eval`` reads for a query: ``int()`` of the scaled coordinates; -1 (the uniform prior) for
    a NaN longitude.  ValueError: a cell outside the grid (names the first such row), a NaN latitude."""
    locs = np.asarray(locs, dtype=np.float64).reshape(-1, 2)
    x = (locs[:, 0] + 180) / 360.0
    x *= lon_bins
    y = (locs[:, 1] + 90) / 180.0
    y *= lat_bins
    uniform = np.isnan(locs[:, 0])
    with np.errstate(invalid="ignore"):
        xi, yi = np.trunc(x), np.trunc(y)
        bad = ~uniform & ~((xi >= 0) & (xi < lon_bins) & (yi >= 0) & (yi < lat_bins))
    if bad.any():
        row = int(np.flatnonzero(bad)[0])
        raise ValueError(f"grid prior: query row {row} {tuple(locs[row])} falls outside the {lon_bins} x {lat_bins} grid")
    cells = np.where(uniform, 0.0, yi) * lon_bins + np.where(uniform, 0.0, xi)
    return np.where(uniform, _nn.CELL_UNIFORM, cells).astype(np.int32)


def _device(device) -> torch.device:
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError(f"the neighbour / grid priors run on the GPU only; there is no CPU path (device={dev})")
    return dev


def _ranks(out) -> Tuple[np.ndarray, np.ndarray]:
    """The kernel's three integers -> (ranks int64 from 1, 0 where the label's score is NaN; predicted classes, -1
    there), as ``CspLocationModel.label_ranks`` returns them."""
    g, e, am = (t.cpu().numpy() for t in out)
    if (g == -2).any():
        raise ValueError("labels outside the classes of the prior")
    ok = g >= 0
    ranks = np.where(ok, 1 + g.astype(np.int64) + e.astype(np.int64), 0)
    return ranks, np.where(ok, am, -1).astype(np.int64)


class _PriorBase:
    def _inputs(self, labels, preds, B):
        dev = self.engine.device
        lab = torch.as_tensor(np.asarray(labels.detach().cpu() if hasattr(labels, "detach") else labels)
                              .reshape(-1).astype(np.int32)).to(dev)
        if lab.shape[0] != B:
            raise ValueError(f"{lab.shape[0]} labels for {B} locations")
        img = None
        if preds is not None:
            img = preds if hasattr(preds, "detach") else torch.from_numpy(np.ascontiguousarray(preds))
            if img.dtype not in (torch.float32, torch.float64):
                img = img.to(torch.float64)
            img = img.to(dev).contiguous()
        return lab, img


class NeighborPrior(_PriorBase):
    """``nn_dist`` / ``nn_knn``: ``train_locs`` (N, 2) (lon, lat) degrees, ``train_classes`` (N,); ``hyper_params``
    gives ``dist_type`` ('haversine' or anything else for euclidean degrees), ``dist_thresh`` (radians / degrees) and
    ``num_neighbors``."""

    def __init__(self, train_locs, train_classes, num_classes: int, hyper_params: Dict, device=None):
        self.num_classes = int(num_classes)
        self.haversine = hyper_params.get("dist_type", "euclidean") == "haversine"
        self.dist_thresh = hyper_params.get("dist_thresh")
        self.num_neighbors = hyper_params.get("num_neighbors")
        locs = np.asarray(train_locs, dtype=np.float64)
        if locs.ndim != 2 or locs.shape[1] != 2 or locs.shape[0] < 1:
            raise ValueError(f"train_locs (N, 2) with N > 0, got {locs.shape}")
        self.num_points = locs.shape[0]
        self.engine = _nn.NeighborEngine(_device(device))
        self.engine.set_neighbors(np.deg2rad(locs) if self.haversine else locs, train_classes, self.num_classes,
                                  self.haversine)

    def _q(self, locs) -> torch.Tensor:
        q = np.asarray(locs.detach().cpu() if hasattr(locs, "detach") else locs, dtype=np.float64).reshape(-1, 2)
        return torch.from_numpy(np.ascontiguousarray(np.deg2rad(q) if self.haversine else q)).to(self.engine.device)

    def _pred(self, ptype: str) -> Dict:
        if ptype not in PTYPES:
            raise ValueError(f"ptype {ptype!r}: 'distance' or 'knn'")
        if ptype == "distance":
            if self.dist_thresh is None:
                raise ValueError("hyper_params['dist_thresh'] is missing")
            return dict(mode=_nn.RADIUS, thr=radius_threshold(self.dist_thresh, self.haversine))
        if self.num_neighbors is None:
            raise ValueError("hyper_params['num_neighbors'] is missing")
        k = int(self.num_neighbors)
        if k < 1 or k > self.num_points:
            raise ValueError(f"num_neighbors = {k} of {self.num_points} training points (1 .. N, as BallTree.query)")
        return dict(mode=_nn.KNN, k=k)

    def prior(self, locs, ptype: str) -> np.ndarray:
        """(B, num_classes) float64: ``compute_neighbor_prior`` of every row."""
        return self.engine.neighbor_prior(self._q(locs), None, **self._pred(ptype)).cpu().numpy()

    def label_ranks(self, locs, labels, preds=None, ptype: str = "distance") -> Tuple[np.ndarray, np.ndarray]:
        """(ranks, predicted classes) of ``preds * prior(locs)`` (``preds`` (B, num_classes) float32 / float64 or
        None); no row is dropped: a NaN location has the uniform prior."""
        q = self._q(locs)
        lab, img = self._inputs(labels, preds, q.shape[0])
        return _ranks(self.engine.neighbor_rank(q, None, labels=lab, img=img, **self._pred(ptype)))

    def kth_distance(self, locs, k: int) -> np.ndarray:
        """The distance to the k-th nearest training point, as ``BallTree.query(k)`` gives it: radians
        (``2 arcsin(sqrt(a))``) or degrees (``sqrt(d2)``); NaN for a NaN location."""
        red_k, _ = self.engine.neighbor_select(self._q(locs), int(k))
        red_k = red_k.cpu().numpy()
        with np.errstate(invalid="ignore"):
            return 2 * np.arcsin(np.sqrt(red_k)) if self.haversine else np.sqrt(red_k)


class GridPrior(_PriorBase):
    """``grid``: per-cell class counts with a pseudo-count; ``hyper_params`` gives ``gp_size`` = [lon_bins, lat_bins]
    and ``pseudo_count``."""

    def __init__(self, locs, classes, num_classes: int, hyper_params: Dict, device=None):
        self.num_classes = int(num_classes)
        self.lon_bins, self.lat_bins = (int(v) for v in hyper_params["gp_size"])
        if self.lon_bins < 1 or self.lat_bins < 1 or self.lon_bins * self.lat_bins >= 2 ** 31:
            raise ValueError(f"gp_size {hyper_params['gp_size']}")
        self.pseudo_count = hyper_params["pseudo_count"]
        # numpy's scalars, as GridPrior.__init__ forms the denominator's constant
        self._pc = float(np.float64(self.pseudo_count))
        self._cpc = float(np.float64(self.num_classes * self.pseudo_count))
        locs = np.asarray(locs, dtype=np.float64)
        if locs.ndim != 2 or locs.shape[1] != 2 or locs.shape[0] < 1:
            raise ValueError(f"locs (N, 2) with N > 0, got {locs.shape}")
        self.engine = _nn.NeighborEngine(_device(device))
        self.engine.set_neighbors(locs, classes, self.num_classes, False, cells=train_cells(locs, self.lon_bins, self.lat_bins))

    def _qcell(self, locs) -> torch.Tensor:
        q = np.asarray(locs.detach().cpu() if hasattr(locs, "detach") else locs, dtype=np.float64).reshape(-1, 2)
        return torch.from_numpy(query_cells(q, self.lon_bins, self.lat_bins)).to(self.engine.device)

    def eval(self, locs) -> np.ndarray:
        """``GridPrior.eval`` of one location (2,) -> (num_classes,), or of (B, 2) -> (B, num_classes); float64."""
        single = np.ndim(locs) == 1
        out = self.engine.neighbor_prior(None, self._qcell(locs), _nn.CELL, pc=self._pc, cpc=self._cpc).cpu().numpy()
        return out[0] if single else out

    def label_ranks(self, locs, labels, preds=None) -> Tuple[np.ndarray, np.ndarray]:
        qc = self._qcell(locs)
        lab, img = self._inputs(labels, preds, qc.shape[0])
        return _ranks(self.engine.neighbor_rank(None, qc, _nn.CELL, labels=lab, img=img, pc=self._pc, cpc=self._cpc))


#: kde_prior's message for a zero bandwidth
KDE_ZERO_BANDWIDTH = "All data points are at the same location - try reducing quantization."


def create_kde_grid(train_classes, train_locs, hyper_params) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """baselines.py ``create_kde_grid``, vectorised: the training set quantised with ``np.floor(locs / q) * q`` and
    reduced to the unique (class, ``hashable_loc``) pairs in first-occurrence order -> (``binned_classes`` (M,),
    ``binned_locs`` (M, 2) - the quantised location of a pair's first occurrence -, ``counts`` (M,) int64), the
    reference's three arrays bit for bit.  ``hashable_loc`` is ``floor(quantised / q)`` per axis, evaluated on the
    ALREADY quantised value as there (it can differ from ``floor(x / q)`` by one).  AssertionError: ``kde_quant <=
    0``; ValueError: a training location that is not finite."""
    q = hyper_params["kde_quant"]
    assert q > 0
    locs = np.asarray(train_locs)
    classes = np.asarray(train_classes)
    if locs.ndim != 2 or locs.shape[1] != 2 or classes.shape != (locs.shape[0],):
        raise ValueError(f"train_locs (N, 2) and train_classes (N,), got {locs.shape} and {classes.shape}")
    if not np.isfinite(locs).all():
        row = int(np.flatnonzero(~np.isfinite(locs).all(axis=1))[0])
        raise ValueError(f"kde prior: training location {row} {tuple(locs[row])} is not finite")
    quantized = np.floor(locs / q) * q
    key = np.floor(quantized / q).astype(np.int64)
    _, cls_id = np.unique(classes, return_inverse=True)
    rows = np.stack([cls_id.reshape(-1).astype(np.int64), key[:, 0], key[:, 1]], axis=1)
    _, first, counts = np.unique(rows, axis=0, return_index=True, return_counts=True)
    order = np.argsort(first, kind="stable")
    first = first[order]
    return classes[first], quantized[first], counts[order].astype(np.int64)


class KdePrior(_PriorBase):
    """``kde``: ``train_locs`` (N, 2) (lon, lat) degrees, ``train_classes`` (N,); ``hyper_params`` gives ``kde_quant``,
    ``kde_nb`` and ``kde_dist_type`` ('haversine' or anything else for euclidean degrees).  Bins the training set on
    the host once (``create_kde_grid``), installs the bins with their counts, and answers a batch with one selection
    (the ``kde_nb``-th bin's distance), the reference's bandwidth arithmetic on the host in numpy scalars, and one
    scan.  A NaN coordinate - longitude or latitude - gives the uniform prior; an infinite one, ``kde_nb`` outside
    1 .. M and a zero bandwidth raise ValueError."""

    def __init__(self, train_locs, train_classes, num_classes: int, hyper_params: Dict, device=None):
        self.num_classes = int(num_classes)
        self.haversine = hyper_params.get("kde_dist_type", "euclidean") == "haversine"
        self.kde_nb = hyper_params.get("kde_nb")
        locs = np.asarray(train_locs, dtype=np.float64)
        if locs.ndim != 2 or locs.shape[1] != 2 or locs.shape[0] < 1:
            raise ValueError(f"train_locs (N, 2) with N > 0, got {locs.shape}")
        dev = _device(device)
        self.binned_classes, self.binned_locs, self.counts = create_kde_grid(np.asarray(train_classes).reshape(-1), locs, hyper_params)
        self.num_bins = len(self.counts)
        self.engine = _nn.NeighborEngine(dev)
        self.engine.set_kde_points(np.deg2rad(self.binned_locs) if self.haversine else self.binned_locs, self.binned_classes,
                                   self.counts, self.num_classes, self.haversine)

    def _scan_inputs(self, locs):
        """The batch on the device and its per-row (thr, two_h2) there; h (B,) on the host (NaN for a NaN row)."""
        if self.kde_nb is None:
            raise ValueError("hyper_params['kde_nb'] is missing")
        k = int(self.kde_nb)
        if k < 1 or k > self.num_bins:
            raise ValueError(f"kde_nb = {k} of {self.num_bins} bins (1 .. M, as BallTree.query)")
        q = np.asarray(locs.detach().cpu() if hasattr(locs, "detach") else locs, dtype=np.float64).reshape(-1, 2)
        if np.isinf(q).any():
            row = int(np.flatnonzero(np.isinf(q).any(axis=1))[0])
            raise ValueError(f"kde prior: query row {row} {tuple(q[row])} has an infinite coordinate")
        dev = self.engine.device
        qd = torch.from_numpy(np.ascontiguousarray(np.deg2rad(q) if self.haversine else q)).to(dev)
        red_k = self.engine.neighbor_select(qd, k)[0].cpu().numpy()
        with np.errstate(invalid="ignore"):
            d_k = 2 * np.arcsin(np.sqrt(red_k)) if self.haversine else np.sqrt(red_k)       # as kth_distance
        h = 0.5 * d_k
        if (h == 0).any():
            row = int(np.flatnonzero(h == 0)[0])
            raise ValueError(f"kde prior: query row {row}: {KDE_ZERO_BANDWIDTH}")
        # numpy scalars, the reference's expressions: r = 2 h + 1e-9, 2 h ** 2 (a scalar ** is pow, not a product)
        thr = np.array([radius_threshold(2 * x + 1e-9, self.haversine) for x in h], dtype=np.float64)
        two_h2 = np.array([2 * x ** 2 for x in h], dtype=np.float64)
        return qd, torch.from_numpy(thr).to(dev), torch.from_numpy(two_h2).to(dev), h

    def prior(self, locs) -> np.ndarray:
        """(B, num_classes) float64: ``kde_prior`` of every row."""
        qd, thr, two_h2, _ = self._scan_inputs(locs)
        return self.engine.kde_prior(qd, thr, two_h2).cpu().numpy()

    def label_ranks(self, locs, labels, preds=None) -> Tuple[np.ndarray, np.ndarray]:
        """(ranks, predicted classes) of ``preds * prior(locs)``; no row is dropped."""
        qd, thr, two_h2, _ = self._scan_inputs(locs)
        lab, img = self._inputs(labels, preds, qd.shape[0])
        return _ranks(self.engine.kde_rank(qd, thr, two_h2, labels=lab, img=img))

    def bandwidth(self, locs) -> np.ndarray:
        """The kernel bandwidth ``h = 0.5 d_k`` of every row (radians / degrees); NaN for a NaN location."""
        return self._scan_inputs(locs)[3]
