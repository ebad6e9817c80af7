"""The numpy restatement of the KDE geo prior (range_amd/csrc/kde_kernel.h, range_amd/geo_baselines.py: KdePrior)
and the error bounds of its three layers of comparison.  tests/test_kde_cpu.py pins the restatement to what the
reference's own ``create_kde_grid`` / ``kde_prior`` gave (tests/golden/kde_priors.npz); the GPU tests compare the
kernels with it.  numpy only.  Locations are (lon, lat) DEGREES at this level.

THE FORMULA.  With w_j = exp(-dist_j / (2 h^2)) the float64 weight of member j, S_c = sum of count_j w_j over the
members of class c and m the smallest non-zero S_c, the reference's (2 pi h)^-1 and kde_den cancel:
prior[c] = (S_c + m) / (sum_c S_c + C m).  ``kde_prior_exact`` evaluates it on the float64 weights with exact integer
sums and one rounding at the end.

LAYER 1, reference vs ``kde_prior_exact`` (eps = 2^-53, first order, every term non-negative so relative errors do
not amplify).  The reference forms Q_j = K w_j (1 rounding), count_j Q_j (1), a sequential sum of n_c <= n members
(n - 1): S_c carries (n + 1) eps.  The minimum carries as much; adding it, 1 more: the numerator (n + 2) eps.
kde_den is ONE float64 for all classes and cancels from kde / sum(kde) whatever its error.  The division by it: 1;
the sum of the C quotients, each within (n + 3) eps: (n + 3) + (C - 1); the last division: 1; the rounding of the
exact value: 1.  Together (2 n + C + 8) eps with n the members of the row; ``layer1_bound`` returns 1.01 times that
for the terms of second order.  (Observed: below 6e-16.)

LAYER 2, the kernel's integer sums vs ``fixed_sums`` (numpy's exp).  A member enters as count * rint(w 2^s).  Two
evaluations of w that differ by at most u units of 2^-52 (the spacing of doubles below 1; w <= 1) differ, after the
rint of each, by at most 1 + ceil(u 2^(s - 52)) units of 2^-s: per member count * that (``layer2_units``).
u = U_EXP for the euclidean metric, whose dist is red, bit for bit the host's.  U_EXP: the device's exp was measured
once on an MI355X against long-double numpy over 2 000 001 arguments of [-2 - 1e-6, 0] through this kernel (one bin
of count 1, so s = 52 and a row IS rint(w 2^52)): the largest |row - w_exact 2^52| was 0.906 units, rint's half
unit included; U_EXP_MEASURED is that, rounded up.  (The same run through the haversine chain, 10^6 members with
a <= 0.09: 1.69 units.)  numpy's exp is within U_NUMPY_EXP of the exact value on that range (asserted by
tests/test_kde_cpu.py).  U_EXP = 2 * U_EXP_MEASURED + U_NUMPY_EXP: twice the measured value, as the project does
elsewhere.  For haversine the member's dist goes through sin, cos, sqrt and asin on the device: ``hav_weight_units``
turns the chain's bound into units of w and adds U_EXP.

LAYER 3, KdePrior.prior vs the reference.  Every integer is within layer 2's per-member bound of w_j 2^s and
w_j >= e^-2 - 1e-6, so numerator and denominator of the prior are each within a relative eta of the exact ones:
``layer3_bound`` = 2.02 eta + layer 1, eta = (0.5 + u 2^(s - 52)) / (W_MIN 2^s) + (haversine: the bandwidth's
error, see there)."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import neighbor_refs as R
from range_amd import csp_eval
from range_amd import geo_baselines as gb

EPS = 2.0 ** -53
ULP = 2.0 ** -52
W_MIN = math.exp(-2.0) - 1e-6            # dist <= (2 h + 1e-9)^2: the argument of exp stays above -2 - 1e-6
ARG_MIN = -2.0 - 1e-6
U_EXP_MEASURED = 0.91                     # units of 2^-52, measured on the GPU (see above)
U_NUMPY_EXP = 1.0
U_EXP = 2 * U_EXP_MEASURED + U_NUMPY_EXP
# the random sweeps of tests/test_gpu_kde.py: (seed, M); tests/test_kde_cpu.py asserts that they leave out no query
SWEEP_SEEDS = ((201, 1), (202, 255), (203, 256), (204, 257), (205, 1000))
SWEEP_B = 25
SWEEP_NBS = (1, 2, 64)                    # and M


# ---- binning

def bin_grid(train_classes, train_locs, q):
    """The restated binning: quantise, then keep the first occurrence of every (class, key) with
    key = floor(quantised / q) per axis - evaluated on the quantised value -, counting the repeats."""
    quant = np.floor(np.asarray(train_locs) / q) * q
    slot, classes, locs, counts = {}, [], [], []
    for cls, loc in zip(np.asarray(train_classes).tolist(), quant):
        key = (cls, int(np.floor(loc[0] / q)), int(np.floor(loc[1] / q)))
        if key in slot:
            counts[slot[key]] += 1
        else:
            slot[key] = len(counts)
            classes.append(cls)
            locs.append(loc)
            counts.append(1)
    return np.array(classes), np.array(locs).reshape(-1, 2), np.array(counts)


# ---- per query: bandwidth, members, weights

def query_params(red_k, haversine: bool, radius_eps: float = 1e-9, h_factor: float = 0.5):
    """(h, thr, two_h2), (B,) each, from the k-th reduced distance, in numpy scalars and the reference's expressions;
    NaN rows stay NaN.  ``radius_eps`` / ``h_factor``: planted defects."""
    red_k = np.asarray(red_k, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        d_k = 2 * np.arcsin(np.sqrt(red_k)) if haversine else np.sqrt(red_k)
    h = h_factor * d_k
    thr = np.array([gb.radius_threshold(2 * x + radius_eps, haversine) for x in h], dtype=np.float64)
    two_h2 = np.array([2 * x ** 2 for x in h], dtype=np.float64)
    return h, thr, two_h2


def member_dist(qm, sm, red, haversine: bool, sklearn_order: bool = False):
    """(B, M) the squared distance a member is weighed by, metric-space rows."""
    if not haversine:
        return red
    with np.errstate(invalid="ignore"):
        if sklearn_order:
            return (2 * np.arcsin(np.sqrt(red))) ** 2
        d_lon = sm[:, 0][None, :] - qm[:, 0][:, None]
        d_lat = sm[:, 1][None, :] - qm[:, 1][:, None]
        cos_term = np.cos(sm[:, 1])[None, :] * np.cos(qm[:, 1])[:, None]
        a = np.sin(d_lat / 2.0) ** 2 + cos_term * np.sin(d_lon / 2.0) ** 2
        return (2 * 1 * np.arcsin(np.sqrt(a))) ** 2


class Rows:
    """Everything per (query, bin) of one batch: red, members, float64 weights; h, thr, two_h2 per query."""

    def __init__(self, q_deg, binned_locs_deg, haversine: bool, nb: int, radius_eps: float = 1e-9, h_factor: float = 0.5,
                 sklearn_order: bool = False):
        self.hav = haversine
        self.qm, self.sm = R.metric_locs(q_deg, haversine), R.metric_locs(binned_locs_deg, haversine)
        self.red = R.red_matrix(self.qm, self.sm, haversine)
        self.nan = np.isnan(self.qm).any(axis=1)
        self.red_k = R.select_kth(self.red, nb)[0]
        self.h, self.thr, self.two_h2 = query_params(self.red_k, haversine, radius_eps, h_factor)
        with np.errstate(invalid="ignore"):
            self.members = self.red <= self.thr[:, None]
            self.dist = member_dist(self.qm, self.sm, self.red, haversine, sklearn_order)
            self.arg = -self.dist / self.two_h2[:, None]
            self.w = np.exp(self.arg)

    def gaps(self):
        """(a) per row the smallest relative distance from thr of a pair NOT tied with the k-th; (b) the k-th pair's
        own margin (thr - red_k) / thr.  inf for a NaN row."""
        with np.errstate(invalid="ignore"):
            g = np.abs(self.red - self.thr[:, None]) / self.thr[:, None]
            g = np.where((self.red == self.red_k[:, None]) | np.isnan(g), np.inf, g)
            own = (self.thr - self.red_k) / self.thr
        return g.min(axis=1), np.where(np.isnan(own), np.inf, own)


def kde_prior_exact(rows: Rows, classes, counts, C: int, use_counts: bool = True, min_per_class: bool = True,
                    min_over_zero: bool = False) -> np.ndarray:
    """(B, C) float64: the formula on the float64 weights with exact sums (integers: w 2^60 is one for w >= 2^-8) and
    one rounding.  The keyword arguments plant defects."""
    B = rows.w.shape[0]
    out = np.empty((B, C))
    cls, cnt = np.asarray(classes).tolist(), np.asarray(counts).tolist()
    for i in range(B):
        js = np.flatnonzero(rows.members[i])
        if rows.nan[i] or len(js) == 0:
            out[i] = np.ones(C) / float(C)
            continue
        S = [0] * C
        for j in js.tolist():
            w = float(rows.w[i, j])
            assert w >= 2.0 ** -8
            S[cls[j]] += (cnt[j] if use_counts else 1) * int(w * 2.0 ** 60)
        m = min(S) if min_over_zero else min(v for v in S if v > 0)
        if min_per_class:
            den = sum(S) + C * m
            out[i] = [float(Fraction(v + m, den)) for v in S]
        else:                                  # the minimum added once, to the total only
            den = sum(S) + m
            out[i] = [float(Fraction(v, den)) for v in S]
    return out


def layer1_bound(n_members, C: int):
    return 1.01 * (2 * np.asarray(n_members, dtype=np.float64) + C + 8) * EPS


# ---- the kernel's integers

def scale_bits(total_count: int) -> int:
    """host_plan.h: kde_scale_bits."""
    return min(52, 62 - int(total_count).bit_length())


def fixed_sums(rows: Rows, classes, counts, C: int, s: int) -> np.ndarray:
    """(B, C) int64: the kernel's rows with numpy's exp."""
    out = np.zeros((rows.w.shape[0], C), dtype=np.int64)
    cls, cnt = np.asarray(classes).astype(np.int64), np.asarray(counts).astype(np.int64)
    for i in range(out.shape[0]):
        js = np.flatnonzero(rows.members[i])
        fixed = np.rint(rows.w[i, js] * 2.0 ** s).astype(np.int64)
        np.add.at(out[i], cls[js], cnt[js] * fixed)
    return out


def prior_from_sums(sums) -> np.ndarray:
    """The rank tail's prior, float64 operation by operation as the kernel does it."""
    sums = np.asarray(sums, dtype=np.int64)
    B, C = sums.shape
    total = sums.sum(axis=1)
    m = np.where(sums > 0, sums, np.iinfo(np.int64).max).min(axis=1)
    den = total.astype(np.float64) + np.float64(C) * m.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = (sums.astype(np.float64) + m.astype(np.float64)[:, None]) / den[:, None]
    p[total == 0] = 1.0 / np.float64(C)
    return p


def ranks_from_sums(sums, img, labels):
    return csp_eval.rank_counts(R.scores(prior_from_sums(sums), img), labels)


def member_units(u, s: int):
    """Per member of count 1: by how many units of 2^-s two evaluations whose w differ by u units of 2^-52 may differ."""
    return 1 + np.ceil(np.asarray(u, dtype=np.float64) * 2.0 ** (s - 52))


def asin_amplification(a):
    """d = 2 asin(sqrt(a)): the relative error of d per relative error of a."""
    r = np.sqrt(a)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = r / (2 * np.arcsin(r) * np.sqrt(1 - a))
    return np.where(a > 0, f, 0.5)


def hav_weight_units(rows: Rows):
    """(B, M) units of 2^-52 by which the device's and numpy's w of a haversine member may differ.  a = sA sA + cc
    (sB sB): sin / cos of device and numpy differ by at most 5 ulp (4, the OpenCL bound of the device library, + 1),
    four factors and three roundings, the sum keeps the larger relative error plus one: 24, 32 taken as for red
    (tests/test_gpu_neighbors.py).  sqrt: 1.5 ulp between the two, through asin twice the amplification; asin: 5;
    d d, the division and the negation: 2 more; w's relative error is |arg| <= 2 - ARG_MIN times the argument's; w <= 1."""
    a = np.sin(np.sqrt(rows.dist) / 2) ** 2
    amp = np.maximum(asin_amplification(a), 0.5)
    rel_d = 32 * amp + 1.5 * 2 * amp + 5
    rel_arg = 2 * rel_d + 2
    return U_EXP + np.abs(rows.arg) * rel_arg


def layer2_units(rows: Rows, classes, counts, C: int, s: int) -> np.ndarray:
    """(B, C) the bound on |kernel row - fixed_sums| in units of 2^-s."""
    out = np.zeros((rows.w.shape[0], C), dtype=np.float64)
    cls, cnt = np.asarray(classes).astype(np.int64), np.asarray(counts).astype(np.float64)
    u = hav_weight_units(rows) if rows.hav else np.full(rows.w.shape, U_EXP)
    for i in range(out.shape[0]):
        js = np.flatnonzero(rows.members[i])
        np.add.at(out[i], cls[js], cnt[js] * member_units(u[i, js], s))
    return out


def layer3_bound(rows: Rows, C: int, s: int) -> np.ndarray:
    """(B,) the bound on |KdePrior.prior - reference| / reference.  Every integer of a row is within
    0.5 + u 2^(s - 52) units of count w 2^s, w >= W_MIN: a relative eta on S_c, on m and on their sums, hence
    (1 + eta) / (1 - eta) - 1 <= 2.02 eta on the prior; plus layer 1.  Haversine: the device's red_k is within 32 ulp
    of numpy's (tests/test_gpu_neighbors.py: RED_REL_BOUND), h through d(a) within 32 amp + 4 ulp, and two_h2 =
    2 h^2 within twice that plus 2: the argument of every exp, at most 2 - ARG_MIN, moves by that relative amount."""
    n = rows.members.sum(axis=1)
    if rows.hav:
        u = np.where(rows.members, hav_weight_units(rows), 0.0).max(axis=1)
        with np.errstate(invalid="ignore"):
            amp = np.maximum(asin_amplification(np.where(rows.nan, 0.0, rows.red_k)), 0.5)
        u = u + (2.0 - ARG_MIN) * (2 * (32 * amp + 4) + 2)
    else:
        u = np.full(len(n), U_EXP)
    eta = (0.5 + u * 2.0 ** (s - 52)) / (W_MIN * 2.0 ** s)
    return 2.02 * eta + layer1_bound(n, C)


class NumpyKdePrior:
    """A stand-in for geo_baselines.KdePrior on the host: ``label_ranks`` from the restatement."""

    def __init__(self, train_locs, train_classes, num_classes, hyper_params):
        self.C, self.hp = num_classes, hyper_params
        self.classes, self.locs, self.counts = gb.create_kde_grid(train_classes, train_locs, hyper_params)
        self.calls = 0

    def prior(self, locs):
        rows = Rows(locs, self.locs, self.hp.get("kde_dist_type") == "haversine", int(self.hp["kde_nb"]))
        return kde_prior_exact(rows, self.classes, self.counts, self.C)

    def label_ranks(self, locs, labels, preds=None):
        self.calls += 1
        g, e, am = R.ranks(self.prior(np.asarray(locs, dtype=np.float64)), preds, labels)
        if (g == -2).any():
            raise ValueError("labels outside the classes of the prior")
        ok = g >= 0
        return np.where(ok, 1 + g.astype(np.int64) + e, 0), np.where(ok, am, -1).astype(np.int64)


def sweep_points(seed: int, M: int, C: int):
    """M bins (distinct random locations, classes, counts 1 .. 5) and SWEEP_B queries."""
    s = R.random_locs(M, seed)
    rng = np.random.default_rng(seed + 3)
    return s, rng.integers(0, C, M), rng.integers(1, 6, M), R.queries_near(s, SWEEP_B, seed + 50)
