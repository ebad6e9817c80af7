"""The reference's checkerboard task (range/evaluation/checkerboarddataset.py): a Fibonacci lattice of
support points with cyclic class labels, samples drawn at random or on a second lattice, every sample
labelled with the class of its nearest support point by haversine distance.

The O(N) parts - the lattice, the random draw, ``random_classes`` - are numpy on the host, the reference's
expressions value for value.  The O(samples x support) part - ``assign_closest_label`` and the
nearest-neighbour statistic of ``calc_avg_distances``, a dense float64 matrix in the reference - is the
GPU scan ``HipEngine.nearest_support`` (csrc/checker_kernel.h): O(samples + support) memory, no CPU path.

Deviations: the three datasets of ``CheckerDataset`` hold (lonlat, label) pairs, which
``save_embeddings`` can iterate (the reference's hold three tensors and its save.py:25 unpacks two);
the nearest point is chosen on the haversine term ``a``, of which the distance is a growing function;
non-finite coordinates raise ValueError."""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import _native

EARTH_RADIUS = {"km": 6371, "m": 6371000, "rad": 1, "deg": 1}    # calculate_average_distance_between_closest_neighbors
_engines = {}


def _engine(device=None) -> _native.HipEngine:
    """One bare engine per GPU, created on first use."""
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError(f"the checkerboard task's nearest-support scan runs on the GPU only; there is no CPU path (device={dev})")
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU visible: the checkerboard task's nearest-support scan has no CPU path")
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    if index not in _engines:
        _engines[index] = _native.HipEngine(torch.device("cuda", index))
    return _engines[index]


def generate_fibonaccilattice(N: int, n_classes: int = 16) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """2 * (N // 2) points i = -N//2 .. N//2 - 1 -> (lons, lats) float64 degrees, labels i mod n_classes."""
    n = N // 2
    phi = (1 + math.sqrt(5)) / 2
    i = np.arange(-n, n)
    lats = np.arcsin((2 * i) / (2 * n + 1)) * 180 / np.pi
    lons = (i % phi) * (360 / phi)
    lons = np.where(lons < -180, lons + 360, lons)
    lons = np.where(lons > 180, lons - 360, lons)
    return lons, lats, i % n_classes


def random_samples(N: int, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """N directions of a seeded isotropic normal draw -> (lons, lats) float64 degrees (get_data, grid=False)."""
    x, y, z = np.random.RandomState(seed).normal(size=(3, N))
    hxy = np.hypot(x, y)
    return np.rad2deg(np.arctan2(y, x)), np.rad2deg(np.arctan2(z, hxy))


def _radians_pairs(lons, lats, what: str) -> np.ndarray:
    ll = np.stack([np.asarray(lons, dtype=np.float64), np.asarray(lats, dtype=np.float64)], axis=1)
    if ll.ndim != 2 or ll.shape[0] < 1:
        raise ValueError(f"{what}: need one-dimensional longitudes and latitudes of equal, non-zero length")
    if not np.isfinite(ll).all():
        raise ValueError(f"{what}: non-finite coordinates")
    return np.radians(ll)


def nearest_support(lons_q, lats_q, lons_s, lats_s, exclude_self: bool = False, want_dist: bool = True, device=None):
    """Degrees in -> (index of the nearest support point per query (int64), its distance in radians or None)."""
    s = _radians_pairs(lons_s, lats_s, "support points")
    q = None if exclude_self else _radians_pairs(lons_q, lats_q, "query points")
    eng = _engine(device)
    s = torch.from_numpy(s).to(eng.device)
    q = s if exclude_self else torch.from_numpy(q).to(eng.device)
    idx, dist = eng.nearest_support(q, s, exclude_self=exclude_self, want_dist=want_dist)
    idx = idx.cpu().numpy()
    if (idx < 0).any():
        raise RuntimeError("nearest_support: a query without a valid pair (NaN haversine term)")
    return idx, (dist.cpu().numpy() if want_dist else None)


def assign_closest_label(lons_grid, lats_grid, lons, lats, labels, device=None) -> np.ndarray:
    """The label of the (lons, lats) point nearest to every (lons_grid, lats_grid) point."""
    idx, _ = nearest_support(lons_grid, lats_grid, lons, lats, want_dist=False, device=device)
    return np.asarray(labels)[idx]


def calculate_average_distance_between_closest_neighbors(lons, lats, unit: str = "km", device=None):
    if unit not in EARTH_RADIUS:
        raise ValueError(f"unit {unit!r}: one of {sorted(EARTH_RADIUS)}")
    _, dist = nearest_support(None, None, lons, lats, exclude_self=True, device=device)
    nearest = EARTH_RADIUS[unit] * dist      # (the smallest of radius * c is radius * the smallest c: the product grows with c)
    mean_distance, std_distance = nearest.mean(), nearest.std()
    if unit == "deg":
        return np.rad2deg(mean_distance), np.rad2deg(std_distance)
    return mean_distance, std_distance


def calc_avg_distances(N: int, unit: str = "deg", device=None):
    """Mean and standard deviation of the distance from a lattice point to its nearest neighbour."""
    lons, lats, _ = generate_fibonaccilattice(N)
    return calculate_average_distance_between_closest_neighbors(lons, lats, unit=unit, device=device)


def get_data(N_samples: int, N_support: int, n_classes: int, seed: int = 0, grid: bool = False,
             random_classes: bool = False, device=None):
    """-> (lonlats (n,2) float64 degrees, zeros, labels int64), the reference's three tensors."""
    lons, lats, labels = generate_fibonaccilattice(N_support, n_classes=n_classes)
    if random_classes:
        labels = (np.random.RandomState(seed).rand(len(labels)) * n_classes).astype(int)
    if grid:
        lons_q, lats_q, _ = generate_fibonaccilattice(N_samples)
    else:
        lons_q, lats_q = random_samples(N_samples, seed)
    labels_q = assign_closest_label(lons_q, lats_q, lons, lats, labels, device=device)
    lonlats = torch.from_numpy(np.stack([lons_q, lats_q])).T
    labels_q = torch.from_numpy(labels_q)
    return lonlats, torch.zeros_like(labels_q), labels_q


class CheckerDataset:
    """``train_ds`` (seed 0), ``valid_ds`` (seed 1) and ``evalu_ds`` (a lattice of ``num_samples`` points):
    TensorDatasets of (lonlat, label); ``mean_dist`` / ``std_dist``: the support's nearest-neighbour
    distance in degrees."""

    def __init__(self, num_samples: int = 5000, batch_size: int = 1000, num_classes: int = 4, num_support: int = 200,
                 device: Optional[torch.device | str | int] = None):
        from torch.utils.data import TensorDataset
        self.num_samples = num_samples
        self.batch_size = batch_size
        self.num_support = num_support
        self.num_classes = num_classes
        self.mean_dist, self.std_dist = calc_avg_distances(num_support, unit="deg", device=device)

        def pairs(**kw):
            lonlats, _, labels = get_data(N_samples=num_samples, N_support=num_support, n_classes=num_classes,
                                          device=device, **kw)
            return TensorDataset(lonlats, labels)

        self.train_ds = pairs(seed=0)
        self.valid_ds = pairs(seed=1)
        self.evalu_ds = pairs(grid=True)
