"""Settings of the reference's training-free positional encoders 'Theory' and 's2vec_*'
(range/range.py:164-168, :176-188; positional_encoding/theory.py, sphere2vec/sphere2vec.py).

numpy only: importable without a GPU.  The kernel (range_amd/csrc/posenc_kernel.h) takes the
frequency table as an argument; this module is where the table and the per-name settings come from:
``Theory(frequency_num=32, min_radius=1)`` with the class defaults, and the ``inat2018`` /
``*-linear`` entries of sphere2vec/hparams.yaml as ``get_sphere2vec`` reads them.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

# range_posenc_features(kind), include/range_hip.h
KIND_THEORY, KIND_GRID, KIND_SPHEREC, KIND_SPHERECPLUS, KIND_SPHEREM, KIND_SPHEREMPLUS = range(6)
#: outputs per frequency of a kind (6 for Theory, 4 for grid, 2T for the sphere kinds)
PER_FREQ = {KIND_THEORY: 6, KIND_GRID: 4, KIND_SPHEREC: 6, KIND_SPHERECPLUS: 12, KIND_SPHEREM: 10,
            KIND_SPHEREMPLUS: 16}
MAX_FREQ = 64   # RANGE_POSENC_MAX_F


class PosencSpec(NamedTuple):
    kind: int
    frequency_num: int
    min_radius: float
    max_radius: float
    width: int


def _spec(kind, F, min_radius, max_radius):
    return PosencSpec(kind, F, min_radius, max_radius, PER_FREQ[kind] * F)


#: load_model name -> settings.  (s2vec: hparams.yaml gives frequency_num and min_radius; max_radius is
#: hparams' for grid and get_sphere2vec's default 0.01 for the sphere kinds, sphere2vec.py:250-276)
MODELS = {
    "Theory": _spec(KIND_THEORY, 32, 1, 10000),
    "s2vec_grid": _spec(KIND_GRID, 48, 1, 360),
    "s2vec_spherec": _spec(KIND_SPHEREC, 48, 1, 0.01),
    "s2vec_spherecplus": _spec(KIND_SPHERECPLUS, 16, 1, 0.01),
    "s2vec_spherem": _spec(KIND_SPHEREM, 48, 1, 0.01),
    "s2vec_spheremplus": _spec(KIND_SPHEREMPLUS, 32, 1, 0.01),
}


def is_posenc_name(name: str) -> bool:
    """The names the reference sends to these encoders: 'Theory' and anything holding 's2vec'
    (range.py:165, :177) - an unknown s2vec kind included (``spec`` then raises)."""
    return name == "Theory" or "s2vec" in name


def spec(name: str) -> PosencSpec:
    if name not in MODELS:
        raise NotImplementedError(f"{name} not implemented")
    return MODELS[name]


def cal_freq_list(frequency_num: int, max_radius, min_radius) -> np.ndarray:
    """``_cal_freq_list("geometric", ...)`` (positional_encoding/common.py:4-11) in its expression order."""
    log_timescale_increment = (math.log(float(max_radius) / float(min_radius)) / (frequency_num * 1.0 - 1))
    timescales = min_radius * np.exp(np.arange(frequency_num).astype(float) * log_timescale_increment)
    return 1.0 / timescales


def freq_list(name: str) -> np.ndarray:
    s = spec(name)
    return cal_freq_list(s.frequency_num, s.max_radius, s.min_radius)
