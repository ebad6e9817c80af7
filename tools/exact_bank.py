"""Banks whose retrieval result is exactly representable in float32.

A correct kernel returns these answers bit for bit, in any summation order, so a dropped, doubled
or misplaced row, block, split part or query fails an equality check with certainty at any bank size
(tests/test_gpu_exact.py).  The construction:

* keys are signed one-hot vectors (+-e_j, 512 directions, every other entry +0.0).  A *semantic
  class* is the set of rows with one direction; a query's e-hat is a class direction, so every
  semantic similarity is exactly 1 (in class), 0 (orthogonal) or -1 (opposite);
* locations are the axis vectors +-x, +-y, +-z (a *geographic class* per axis), and so are the
  queries' xq: every geographic similarity is 1, 0 or -1 (up to float32 trig residues of ~1e-8
  when they come from lon/lat, which round away next to 1);
* with the constant shift m = tau*log2(e) of pass 1 an in-class row weighs exactly 1 and an
  out-of-class row 2^-tau*log2(e) or less; every queried class has a power-of-two size P <= 2^17,
  so l = P exactly, and with beta in {0, 1/4, 1/2, 3/4, 1} every in-class weight beta/P,
  (1-beta)/Q or their sum has a few significant bits;
* values are 1 or 2 (column 0 constant, columns 1-20 one bit of the row index, the rest a hash bit
  of (row, column)), so every partial sum of in-class terms needs fewer than 24 bits;
* ``assert_margin``: the whole out-of-class mass of an output element (and of l) stays below half
  an ulp of the smallest in-class term, so round-to-nearest absorbs it at every addition.

The answer is then beta * S_sem / P + (1 - beta) * S_geo / Q (S = the class's column sums), computed
here in float64 and checked to be a float32.

These operands pin the accounting and leave the arithmetic unchecked: a 256-long chain that adds one
non-zero product, values without mantissa bits and weights of 1 survive bf16 keys, a truncated V or a
wrong exp2.  A second family (``build_dense``, below: full-width keys with mantissa bits, 18-bit
values, graded power-of-two weights) keeps the method and widens the operands; it shares ``ExactBank``,
``queries``, ``expect``, ``expect_stats``, ``assert_margin`` and ``topk_expect`` with this one
(tests/test_gpu_exact_dense.py, tests/test_exact_dense_cpu.py).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

KEY_DIM, VAL_DIM = 256, 1024
LOG2E = 1.4426950408889634
TAU = 43.0                       # RANGE_MAX_TAU: the widest gap between in- and out-of-class weights
N_DIRS = 2 * KEY_DIM             # direction d: +e_d for d < 256, -e_(d-256) otherwise
AXES = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]], np.float32)
AXIS_LONLAT = np.array([[0, 0], [90, 0], [0, 90], [180, 0], [-90, 0], [0, -90]], np.float64)
N_GEO_QUERIED = 3                # geographic classes 0..2 are queried; rows on axes 3..5 are not
_HASH_A, _HASH_B, _HASH_P = 1_000_003, 7_919, 2_147_483_647


def k_shift(tau: float) -> np.float32:
    """The kernels' shift m = k = (float)(tau * log2 e) (scan_host.h: softmax_scales, k_sem / k_geo)."""
    return np.float32(float(np.float32(tau)) * LOG2E)


def pow2_partition(n: int, cap: int) -> List[int]:
    """n rows as power-of-two class sizes: equal classes of ``cap`` rows, then the binary digits
    of the remainder (largest first)."""
    assert n >= 1 and cap >= 1 and cap & (cap - 1) == 0
    sizes = [cap] * (n // cap)
    r = n % cap
    sizes += [1 << b for b in range(r.bit_length() - 1, -1, -1) if r >> b & 1]
    return sizes


def direction_vector(d: int) -> np.ndarray:
    v = np.zeros(KEY_DIM, np.float32)
    v[d % KEY_DIM] = -1.0 if d >= KEY_DIM else 1.0
    return v


def value_bits(rows, xp=np):
    """(len(rows), 1024) 0/1 matrix of the value signature (V = 1 + bits): column 0 zero, columns
    1-20 bit j-1 of the row index, the rest a hash bit of (row, column).  ``xp``: numpy or torch."""
    if xp is np:
        i = np.asarray(rows, np.int64)[:, None]
        j = np.arange(VAL_DIM, dtype=np.int64)[None, :]
    else:
        i = rows.to(xp.int64)[:, None]
        j = xp.arange(VAL_DIM, dtype=xp.int64, device=rows.device)[None, :]
    h = (i * _HASH_A + j * _HASH_B) % _HASH_P
    h = (h * h) % _HASH_P
    bits = (h >> 9) & 1
    low = (i >> xp.clip(j - 1, 0, 62) if xp is np else i >> (j - 1).clamp(0, 62)) & 1
    bits = xp.where((j >= 1) & (j <= 20), low, bits)
    return xp.where(j == 0, xp.zeros_like(bits), bits)


@dataclass
class ExactBank:
    n: int
    keys: np.ndarray          # (n,256) float32 signed one-hot
    values: np.ndarray        # (n,1024) float32 in {1, 2}
    xyz: np.ndarray           # (n,3) float32 axis vectors
    sem: np.ndarray           # (n,) semantic class of each row
    geo: np.ndarray           # (n,) axis of each row (0..5)
    sem_dir: np.ndarray       # (n_classes,) direction of each semantic class
    sem_size: np.ndarray      # (n_classes,) rows per class (powers of two)
    geo_size: np.ndarray      # (6,) rows per axis (0..2: powers of two or 0)
    sem_sum: np.ndarray       # (n_classes,1024) float64 column sums of the class's values (dense family:
                              # each row times its weight 2^(-k d/128) under the constant shift)
    geo_sum: np.ndarray       # (6,1024) float64
    # the dense family (``build_dense``); None / 0 on a one-hot bank
    grade: Optional[np.ndarray] = None    # (n,) sign flips d of each row: its in-class similarity is 1 - d/128
    k: int = 0                            # the integer k = tau * log2(e) the class sizes are made for
    sem_l: Optional[np.ndarray] = None    # (n_classes,) float64 l_sem of a class at k (a power of two)
    geo_l: Optional[np.ndarray] = None    # (6,) float64 l_geo of an axis at k (graded geographic classes), else None

    @property
    def n_classes(self) -> int:
        return int(self.sem_size.shape[0])

    @property
    def dense(self) -> bool:
        return self.grade is not None

    @property
    def l_sem(self) -> np.ndarray:
        """l_sem of each class under the constant shift (one-hot family: the class size)."""
        return self.sem_size if self.sem_l is None else self.sem_l

    @property
    def l_geo(self) -> np.ndarray:
        return self.geo_size if self.geo_l is None else self.geo_l

    def class_vectors(self, classes) -> np.ndarray:
        """(len(classes),256) float32 unit directions of semantic classes."""
        d = self.sem_dir[np.asarray(classes, np.int64)]
        if self.dense:
            return dense_directions(d)
        out = np.zeros((len(d), KEY_DIM), np.float32)
        out[np.arange(len(d)), d % KEY_DIM] = np.where(d >= KEY_DIM, -1.0, 1.0).astype(np.float32)
        return out

    def rows(self, lo: int, hi: int):
        """Arrays of rows [lo, hi) (a shard)."""
        return self.keys[lo:hi], self.values[lo:hi], self.xyz[lo:hi]


def _geo_sizes(n: int, cap: int) -> List[int]:
    """Rows on the three queried axes: powers of two, together at most n."""
    out, left = [], n
    for share in (2, 2, 1):
        s = min(cap, max(left // share, 1 if left else 0))
        out.append(1 << (s.bit_length() - 1) if s else 0)
        left -= out[-1]
    return out


def _plan(n: int, seed: int, sem_cap: int, geo_cap: int, sem_dirs: Optional[Sequence[int]],
          sem_sizes: Optional[Sequence[int]] = None):
    rng = np.random.default_rng(seed)
    sizes = np.array(pow2_partition(n, sem_cap) if sem_sizes is None else sem_sizes, np.int64)
    assert sizes.sum() == n
    dirs = (np.array(sem_dirs, np.int64) if sem_dirs is not None else
            rng.permutation(N_DIRS)[: len(sizes)].astype(np.int64))
    assert len(dirs) == len(sizes) and len(set(dirs.tolist())) == len(dirs)
    sem = np.empty(n, np.int64)
    sem[rng.permutation(n)] = np.repeat(np.arange(len(sizes)), sizes)
    gq = _geo_sizes(n, geo_cap)
    rest = n - sum(gq)
    gs = np.array(gq + [rest - 2 * (rest // 3), rest // 3, rest // 3], np.int64)
    geo = np.empty(n, np.int64)
    geo[rng.permutation(n)] = np.repeat(np.arange(6), gs)
    return sizes, dirs, sem, gs, geo


def build(n: int, seed: int = 0, sem_cap: int = 1 << 14, geo_cap: int = 1 << 14,
          sem_dirs: Optional[Sequence[int]] = None, sem_sizes: Optional[Sequence[int]] = None) -> ExactBank:
    """A seeded bank of ``n`` rows: semantic classes of ``pow2_partition(n, sem_cap)`` sizes (or
    ``sem_sizes``; directions ``sem_dirs`` or seeded) spread over the rows by a permutation (every
    16-row block mixes many classes), geographic classes of ``_geo_sizes`` on the three queried axes,
    the other rows on the other three axes."""
    sizes, dirs, sem, gs, geo = _plan(n, seed, sem_cap, geo_cap, sem_dirs, sem_sizes)
    keys = np.zeros((n, KEY_DIM), np.float32)
    d = dirs[sem]
    keys[np.arange(n), d % KEY_DIM] = np.where(d >= KEY_DIM, -1.0, 1.0).astype(np.float32)
    values = np.empty((n, VAL_DIM), np.float32)
    sem_sum = np.zeros((len(sizes), VAL_DIM))
    geo_sum = np.zeros((6, VAL_DIM))
    for lo in range(0, n, 8192):
        hi = min(n, lo + 8192)
        v = 1.0 + value_bits(np.arange(lo, hi))
        values[lo:hi] = v
        # (integer sums below 2^53: exact in float64)
        sem_sum += np.eye(len(sizes))[sem[lo:hi]].T @ v
        geo_sum += np.eye(6)[geo[lo:hi]].T @ v
    return ExactBank(n, keys, values, AXES[geo].copy(), sem, geo, dirs, sizes, gs, sem_sum, geo_sum)


def build_device(n: int, device, seed: int = 0, sem_cap: int = 1 << 14, geo_cap: int = 1 << 14):
    """``build`` for large n (10^6 rows) made on the device with torch: returns (ExactBank whose
    keys / values / xyz are None, keys, values, xyz as device tensors).  Same bank as ``build``."""
    import torch
    sizes, dirs, sem, gs, geo = _plan(n, seed, sem_cap, geo_cap, None)
    dev = torch.device(device)
    d = torch.from_numpy(dirs[sem]).to(dev)
    keys = torch.zeros((n, KEY_DIM), dtype=torch.float32, device=dev)
    keys[torch.arange(n, device=dev), d % KEY_DIM] = torch.where(d >= KEY_DIM, -1.0, 1.0)
    values = torch.empty((n, VAL_DIM), dtype=torch.float32, device=dev)
    semt, geot = torch.from_numpy(sem).to(dev), torch.from_numpy(geo).to(dev)
    sem_sum = torch.zeros((len(sizes), VAL_DIM), dtype=torch.float64, device=dev)
    geo_sum = torch.zeros((6, VAL_DIM), dtype=torch.float64, device=dev)
    for lo in range(0, n, 65536):
        hi = min(n, lo + 65536)
        v = 1.0 + value_bits(torch.arange(lo, hi, device=dev), torch).to(torch.float64)
        values[lo:hi] = v.float()
        sem_sum.index_add_(0, semt[lo:hi], v)
        geo_sum.index_add_(0, geot[lo:hi], v)
    xyz = torch.from_numpy(AXES).to(dev)[geot].contiguous()
    eb = ExactBank(n, None, None, None, sem, geo, dirs, sizes, gs,
                   sem_sum.cpu().numpy(), geo_sum.cpu().numpy())
    return eb, keys, values, xyz


@dataclass
class Queries:
    sem: np.ndarray    # (B,) semantic class asked for
    geo: np.ndarray    # (B,) axis asked for (0..2)
    e32: np.ndarray    # (B,256) float32
    xq: np.ndarray     # (B,4) float32 (x, y, z, 0)


def queries(bank: ExactBank, B: int, seed: int = 1, classes: Optional[Sequence[int]] = None,
            perturb: bool = False) -> Queries:
    """B queries: the first ones walk through every semantic class (and the non-empty queried
    axes), so that every row of the bank is asked for when B >= n_classes; the rest are drawn at
    random (seeded), so equal queries sit at many positions of the batch.  ``perturb`` (dense family):
    each query carries its own mantissa bits (``_signed_zero_sum`` on the query columns), which leave
    every in-class similarity what it is."""
    rng = np.random.default_rng(seed)
    cls = np.arange(bank.n_classes) if classes is None else np.asarray(classes, np.int64)
    axes = np.flatnonzero(bank.geo_size[:N_GEO_QUERIED] > 0)
    sem = np.concatenate([rng.permutation(cls), rng.choice(cls, size=max(0, B - len(cls)))])[:B]
    geo = np.concatenate([rng.permutation(axes), rng.choice(axes, size=max(0, B - len(axes)))])[:B]
    geo = geo[rng.permutation(B)]
    e32 = bank.class_vectors(sem)
    if perturb:
        assert bank.dense, "only the dense family's queries carry a perturbation"
        e32 = _perturbed(e32, _hadamard(bank.sem_dir[sem]), rng, Q_PERT_COLS)
    xq = np.zeros((B, 4), np.float32)
    xq[:, :3] = AXES[geo]
    return Queries(sem, geo, e32, xq)


def forward_queries(bank: ExactBank, c: int, B: int, seed: int) -> Queries:
    """B queries of a forward through a constant-bias encoder: every one the plain direction of class
    ``c`` (no perturbation: the encoder's float64 normalisation is then exact), at the non-empty queried
    axes in turn and then at random."""
    rng = np.random.default_rng(seed)
    axes = np.flatnonzero(bank.geo_size[:N_GEO_QUERIED] > 0)
    geo = np.concatenate([axes, rng.choice(axes, B)])[:B]
    xq = np.zeros((B, 4), np.float32)
    xq[:, :3] = AXES[geo]
    return Queries(np.full(B, c), geo, np.tile(bank.class_vectors([c])[0], (B, 1)), xq)


def lonlat_of(axes) -> np.ndarray:
    """(lon, lat) degrees of axis points (a forward's queries, an .npz bank's locations)."""
    return AXIS_LONLAT[np.asarray(axes)].copy()


def covered(bank: ExactBank, q: Queries) -> bool:
    """Every row of the bank belongs to a semantic class some query asks for."""
    return bool(np.isin(np.arange(bank.n_classes), q.sem).all())


def _class_stats(bank: ExactBank, k: float, sharp: bool):
    """(m, l) of every semantic class at k = tau * log2(e): the constant shift m = k, or - ``sharp`` -
    the running maximum m = k (1 - d_min / 128); l = the sum of 2^(k s - m) over the class.  float64,
    asserted to be float32 numbers (every exponent an integer)."""
    nc = bank.n_classes
    if not bank.dense:
        return np.full(nc, k), bank.sem_size.astype(np.float64)
    e = -k * bank.grade.astype(np.float64) / 128.0
    assert np.array_equal(e, np.round(e)), f"k = {k}: a grade's exponent is not an integer"
    top = np.full(nc, -np.inf)
    np.maximum.at(top, bank.sem, e)
    if not sharp:
        top = np.zeros(nc)
    l = np.zeros(nc)
    np.add.at(l, bank.sem, np.exp2(e - top[bank.sem]))
    m = k + top
    for a in (m, l):
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a), "statistics are not float32 numbers"
    return m, l


def expect_stats(bank: ExactBank, q: Queries, tau_sem: float = TAU, tau_geo: float = TAU,
                 sharp: bool = False) -> np.ndarray:
    """(B,4) float32 {m_sem, l_sem, m_geo, l_geo} of pass 1 (geo head off: m_geo, l_geo unchecked).
    ``sharp``: the running-maximum form (a temperature above 43): m is the largest logit in the bank.
    The geographic maximum is an in-class row's (similarity 1) either way."""
    st = np.zeros((len(q.sem), 4), np.float32)
    m, l = _class_stats(bank, float(k_shift(tau_sem)), sharp)
    st[:, 0] = m[q.sem]
    st[:, 1] = l[q.sem]
    st[:, 2] = k_shift(tau_geo)
    st[:, 3] = bank.l_geo[q.geo]
    if bank.geo_l is not None:
        assert float(k_shift(tau_geo)) == bank.k, "graded geographic classes: l_geo is known at the bank's k"
    return st


def expect(bank: ExactBank, q: Queries, beta: float, geo: bool = True) -> np.ndarray:
    """(B,1024) float32: beta * S_sem / l + (1 - beta) * S_geo / Q (S = the class's weighted column
    sums, l = l_sem; one-hot family: l = P; geo head off: S_sem / l, as the kernels force beta = 1
    then).  Asserts that the float64 value is a float32."""
    if not geo:
        beta = 1.0
    out = beta * bank.sem_sum[q.sem] / bank.l_sem[q.sem][:, None]
    if beta != 1.0:
        out = out + (1.0 - beta) * bank.geo_sum[q.geo] / bank.l_geo[q.geo][:, None]
    out32 = out.astype(np.float32)
    assert np.array_equal(out32.astype(np.float64), out), "expected retrieval is not a float32"
    return out32


def _half_ulp(x: float) -> float:
    return 2.0 ** (math.floor(math.log2(x)) - 24)


def assert_margin(n: int, P: int, Q: int, beta: float, tau_sem: float, tau_geo: float,
                  s_out: float = 0.0, g_out: float = 0.0, residue: float = 1e-6,
                  l_sem: Optional[float] = None, w_min: float = 1.0, v_bits: int = 0,
                  stats_only: bool = False, l_geo: Optional[float] = None, g_min: float = 1.0) -> None:
    """The out-of-class mass of one query (semantic class of P rows, geographic class of Q rows, n
    rows in all; out-of-class similarities at most ``s_out`` / ``g_out``, up to ``residue``) stays
    below half an ulp of the smallest in-class term of the output, and of l_sem / l_geo: round-to-
    nearest absorbs it at every addition, in any order.  Geo head off: tau_geo <= 0.

    Graded classes (dense family): ``l_sem`` is the class's l (a power of two; default: P rows of
    weight 1), ``w_min`` its smallest in-class weight 2^(-k d/128) - the smallest partial sum of l
    and, times beta / l, the smallest term of the output.  ``v_bits``: the values are 1 + j / 2^v_bits;
    every in-class term is then a multiple of (beta's grid) / l * w_min / 2^v_bits resp.
    (1 - beta's grid) / Q / 2^v_bits, which must be at least 2^-23 - an ulp of the outputs, which
    lie in [1, 2) - so that every partial sum is a float32.  ``stats_only``: the conditions on l_sem /
    l_geo alone (a temperature at which only the statistics are compared: l need not be a power of
    two, beta is not used).  ``l_geo`` / ``g_min``: the same for a graded geographic class of Q rows."""
    graded = l_sem is not None
    l1 = float(l_sem) if graded else float(P)
    if stats_only:
        beta = 0.5
    else:
        assert 2.0 ** -17 <= l1 <= 1 << 17 and math.log2(l1) == round(math.log2(l1)), (P, l1)
    assert P >= 1
    assert 0 < w_min <= 1 and math.log2(w_min) == round(math.log2(w_min)), w_min
    geo = tau_geo > 0
    if not geo:
        beta = 1.0
    assert beta in (0.0, 0.25, 0.5, 0.75, 1.0), beta
    step = 0.25 if beta in (0.25, 0.75) else 0.5 if beta == 0.5 else 1.0     # beta and 1 - beta are multiples of it
    # (a head of weight 0 does not enter the output at all: 0 * finite = 0)
    ca, cb, mass, grid = beta / l1, 0.0, 0.0, 1.0
    if ca > 0:
        w1 = 2.0 ** (float(k_shift(tau_sem)) * (s_out + residue - 1.0))   # heaviest out-of-class weight
        assert (n - P) * w1 < _half_ulp(w_min if graded else P), "l_sem: out-of-class mass not absorbed"
        mass += 2.0 * ca * (n - P) * w1                  # values are at most 2
        grid = min(grid, step / l1 * w_min)
    if geo and beta < 1.0:
        l2 = float(Q) if l_geo is None else float(l_geo)
        assert 1 <= Q and 1 <= l2 <= 1 << 17 and math.log2(l2) == round(math.log2(l2)), (Q, l2)
        assert 0 < g_min <= 1 and math.log2(g_min) == round(math.log2(g_min)), g_min
        w2 = 2.0 ** (float(k_shift(tau_geo)) * (g_out + residue - 1.0))
        assert (n - Q) * w2 < _half_ulp(Q if l_geo is None else g_min), "l_geo: out-of-class mass not absorbed"
        cb = (1.0 - beta) / l2 * g_min
        mass += 2.0 * (1.0 - beta) / l2 * (n - Q) * w2
        grid = min(grid, step / l2 * g_min)
    if stats_only:
        return
    assert grid * 2.0 ** -v_bits >= 2.0 ** -23, f"grid: in-class terms on 2^{math.log2(grid) - v_bits:.0f}, outputs in [1, 2)"
    smallest = min(c for c in (ca * w_min, cb) if c > 0)
    assert mass < _half_ulp(smallest), f"margin: out-of-class mass {mass:.3e} vs half ulp {_half_ulp(smallest):.3e}"


def similarities64(bank: ExactBank, e32: np.ndarray) -> np.ndarray:
    """(B,n) float64 semantic similarities, exact: every product and partial sum of the banks of
    this module fits a float64 many times over."""
    return e32.astype(np.float64) @ bank.keys.astype(np.float64).T


def assert_bank_margin(bank: ExactBank, q: Queries, beta: float, tau_sem: float = TAU,
                       tau_geo: float = TAU, stats_only: bool = False) -> None:
    """``assert_margin`` for every (semantic class, axis) pair the queries ask for.  Dense family:
    with the class's l and smallest weight at ``tau_sem``, the value grid, and the largest
    out-of-class similarity these queries meet in this bank (sign flips of another class reach
    2 d / 256; the perturbations add a little)."""
    pairs = set(zip(q.sem.tolist(), q.geo.tolist()))
    if not bank.dense:
        for c, a in pairs:
            assert_margin(bank.n, int(bank.sem_size[c]), int(bank.geo_size[a]), beta, tau_sem, tau_geo,
                          stats_only=stats_only)
        return
    k = float(k_shift(tau_sem))
    _, l = _class_stats(bank, k, False)
    s = similarities64(bank, q.e32)
    s[q.sem[:, None] == bank.sem[None, :]] = -1.0
    s_out = float(s.max()) if bank.n > 1 else -1.0
    gmax = np.zeros(bank.n_classes, np.int64)
    np.maximum.at(gmax, bank.sem, bank.grade)
    for c, a in pairs:
        assert_margin(bank.n, int(bank.sem_size[c]), int(bank.geo_size[a]), beta, tau_sem, tau_geo,
                      s_out=s_out, residue=0.0, l_sem=float(l[c]), w_min=2.0 ** (-k * gmax[c] / 128.0),
                      v_bits=DENSE_V_BITS, stats_only=stats_only,
                      **({} if bank.geo_l is None else dict(l_geo=float(bank.geo_l[a]), g_min=2.0 ** (-bank.k * GEO_GRADE))))


BETAS = (0.25, 0.5, 0.75, 1.0, 0.0)


def dense_betas(bank: ExactBank) -> tuple:
    """The blend weights of BETAS that a dense bank's value grid admits at its own k, for every semantic
    class and queried axis - ``assert_margin``'s grid condition: a term (beta's grid) / l * (smallest
    in-class weight) / 2^17 stays a multiple of 2^-23.  A head of weight 0 sets no condition."""
    assert bank.dense
    _, l = _class_stats(bank, float(bank.k), False)
    gmax = np.zeros(bank.n_classes, np.int64)
    np.maximum.at(gmax, bank.sem, bank.grade)
    sem = float((np.exp2(-bank.k * gmax / 128.0) / l).min())
    ax = np.flatnonzero(bank.geo_size[:N_GEO_QUERIED] > 0)
    geo = float((1.0 / bank.geo_size[ax]).min()) if bank.geo_l is None else float((2.0 ** (-bank.k * GEO_GRADE) / bank.geo_l[ax]).min())
    floor = 2.0 ** (DENSE_V_BITS - 23)
    out = []
    for beta in BETAS:
        step = 0.25 if beta in (0.25, 0.75) else 0.5 if beta == 0.5 else 1.0
        if (beta == 0.0 or step * sem >= floor) and (beta == 1.0 or step * geo >= floor):
            out.append(beta)
    return tuple(out)


def topk_expect(bank: ExactBank, q: Queries, k: int):
    """Exact top-k of each query (ties to the lower row).  One-hot family: its class's lowest rows
    (similarity 1), then - a class smaller than k - the lowest orthogonal rows (0).  Dense family: by
    the exact similarities (1, 1 - d/128 in eight-way and wider ties, then the other classes' rows).
    (B,k) values, indices."""
    B = len(q.sem)
    if bank.dense:
        s = similarities64(bank, q.e32)
        ti = np.argsort(-s, axis=1, kind="stable")[:, :k]
        assert ti.shape[1] == k, "bank too small for k"
        tv = np.take_along_axis(s, ti, axis=1)
        assert np.array_equal(tv.astype(np.float32).astype(np.float64), tv)
        return tv.astype(np.float32), ti.astype(np.int64)
    tv = np.zeros((B, k), np.float32)
    ti = np.zeros((B, k), np.int64)
    opp = (bank.sem_dir + KEY_DIM) % N_DIRS
    for c in np.unique(q.sem):
        own = np.flatnonzero(bank.sem == c)[:k]
        orth_cls = np.flatnonzero(bank.sem_dir != opp[c])
        orth = np.flatnonzero(np.isin(bank.sem, orth_cls) & (bank.sem != c))[: k - len(own)]
        idx = np.concatenate([own, orth])
        assert len(idx) == k, "bank too small for k"
        sel = q.sem == c
        ti[sel] = idx
        tv[sel] = np.concatenate([np.ones(len(own)), np.zeros(len(orth))]).astype(np.float32)
    return tv, ti


# -- the dense family: full-width keys, 18-bit values, graded weights -----------------------------
# The one-hot family above pins the accounting (which rows, blocks, parts and queries enter a result)
# with operands that no arithmetic defect can change.  This family keeps the bit-for-bit method and
# widens the operands:
# * class c has the direction +-h_c / 16, h_c a row (c >= 1) of the 256 x 256 Sylvester Hadamard
#   matrix: unit norm, two classes exactly orthogonal (or opposite), every one of the 256 products of
#   a similarity non-zero;
# * a row at *grade* d is its class direction with d seeded sign flips: similarity 1 - d/128.  tau is
#   the float32 for which the kernels' k = (float)(tau * log2 e) is a small integer (DENSE_TAU), so
#   with the shift m = k the row weighs 2^(-k d/128) - at k = 48, d = 8: 2^-3.  A class holds n_0 rows
#   at d = 0 and n_g at d = 8 with l = n_0 + n_g 2^(-k/16) a power of two (1 + 8/8 = 2 at k = 48; a third
#   grade d = 16, weight 2^-6, where assert_margin admits it: 4/8 + 32/64 = 1);
#   every other class sits at similarity <= 2 d / 256 + (perturbations) and rounds away;
# * values are 1 + j / 2^17, j a hash of (row, column): 18 significant bits;
# * keys carry a perturbation on the 2^-16 grid (|.| < 2^-9, eight entries per row on KEY_PERT_COLS),
#   whose signed sum over the class direction is 0: the entries have 13 significant bits - neither
#   bf16 (8) nor tf32 (11) holds them - and the similarity is unchanged.  Queries may carry one of their
#   own on Q_PERT_COLS; the sign flips live on FLIP_COLS.  The column sets are disjoint, so every
#   product is a multiple of 2^-20 and every partial sum of a similarity (|.| <= 1 + 2^-6) a float32.
# ``emulate`` is the any-order float32 pipeline these claims are checked with on the CPU
# (tests/test_exact_dense_cpu.py), ``DEFECTS`` the arithmetic faults it can carry.
DENSE_TAU = {32: 22.18071, 40: 27.725887, 48: 33.271065, 56: 38.816242, 64: 44.36142}
DENSE_V_BITS = 17
N_DENSE_DIRS = 2 * (KEY_DIM - 1)          # direction code u: +h_(1 + u) for u < 255, -h_(1 + u - 255) otherwise
GRADE = 8                                  # sign flips of a graded row
KEY_PERT_COLS, FLIP_COLS, Q_PERT_COLS = (0, 128), (128, 192), (192, 256)
PERT_UNIT, PERT_MAX, PERT_PAIRS = 2.0 ** -16, 127, 4
GEO_GRADE = 1.0 / 16                       # a graded location is (1 - 1/16) x its axis: dyadic, norm below 1


def dense_tau(k: int) -> float:
    """The float32 temperature whose k = (float)(tau * log2 e) is the integer ``k``."""
    tau = float(np.float32(DENSE_TAU[k]))
    assert k_shift(tau) == np.float32(k)
    return tau


def _hadamard(dirs) -> np.ndarray:
    """(len(dirs),256) float64 +-1: the signed Hadamard row of each direction code."""
    u = np.asarray(dirs, np.int64)
    c = 1 + u % (KEY_DIM - 1)
    x = c[:, None] & np.arange(KEY_DIM, dtype=np.int64)[None, :]
    par = np.zeros_like(x)
    for b in range(8):
        par ^= x >> b & 1
    return (1.0 - 2.0 * par) * np.where(u >= KEY_DIM - 1, -1.0, 1.0)[:, None]


def dense_directions(dirs) -> np.ndarray:
    return (_hadamard(dirs) / 16.0).astype(np.float32)


def _perturbed(vec: np.ndarray, h: np.ndarray, rng, cols) -> np.ndarray:
    """``vec`` + a perturbation of PERT_PAIRS column pairs inside ``cols`` per row: +u h_a at one column,
    -u h_b at the other (u odd, <= PERT_MAX units of 2^-16), so its signed sum over h is 0."""
    n = vec.shape[0]
    out = vec.astype(np.float64)
    width = cols[1] - cols[0]
    pick = cols[0] + np.argsort(rng.random((n, width)), axis=1)[:, : 2 * PERT_PAIRS]
    u = (2 * rng.integers(0, (PERT_MAX + 1) // 2, size=(n, PERT_PAIRS)) + 1) * PERT_UNIT
    r = np.arange(n)[:, None]
    out[r, pick[:, :PERT_PAIRS]] += u * h[r, pick[:, :PERT_PAIRS]]
    out[r, pick[:, PERT_PAIRS:]] -= u * h[r, pick[:, PERT_PAIRS:]]
    assert np.array_equal(((out - vec) * h).sum(1), np.zeros(n))
    o32 = out.astype(np.float32)
    assert np.array_equal(o32.astype(np.float64), out)
    return o32


def dense_values(rows) -> np.ndarray:
    """(len(rows),1024) float64 1 + j / 2^17, j a 17-bit hash of (row, column)."""
    i = np.asarray(rows, np.int64)[:, None]
    j = np.arange(VAL_DIM, dtype=np.int64)[None, :]
    h = (i * _HASH_A + j * _HASH_B + 12_345) % _HASH_P
    h = (h * h) % _HASH_P
    return 1.0 + ((h >> 7) & ((1 << DENSE_V_BITS) - 1)) / float(1 << DENSE_V_BITS)


def dense_classes(n: int, k: int = 48, no_top: int = 0) -> List[tuple]:
    """n rows as (rows at d = 0, rows at d = GRADE) classes: graded classes of 1 + 2^(k/16) rows
    (l = 2), the first ``no_top`` of them with 2^(k/16) graded rows and none at d = 0 (l = 1: the largest
    logit of such a class is a graded row's), then d = 0 classes of 8, 4, 2, 1 rows for the remainder."""
    assert k % 16 == 0
    g = 1 << (k * GRADE // 128)
    out = []
    while len(out) < no_top and n >= g:
        out.append((0, g))
        n -= g
    while n >= 1 + g and len(out) < N_DENSE_DIRS - 8:
        out.append((1, g))
        n -= 1 + g
    return out + [(s, 0) for s in pow2_partition(n, 8)] if n else out


def build_dense(n: int, k: int = 48, seed: int = 0, classes: Optional[Sequence[tuple]] = None,
                perturb: bool = True, top_last: bool = False, geo_cap: int = 8, geo_graded: bool = False) -> ExactBank:
    """A seeded dense bank of ``n`` rows for the temperature ``dense_tau(k)``: ``classes`` (default
    ``dense_classes(n, k)``; a class is (rows at d = 0, at d = 8[, at d = 16]) - the third grade weighs
    2^-6 at k = 48, which the value grid admits only with l = 1 and beta = 1) with seeded directions, spread over the rows by a permutation
    (``top_last``: the d = 0 rows after all graded rows, so that a running maximum arrives last);
    geographic classes of at most ``geo_cap`` rows on the queried axes (a value term (1 - beta) / Q / 2^17
    must stay on the 2^-23 grid).  ``perturb``: the keys' mantissa perturbation (without it fp16 and bf16
    hold the keys, and numpy's float32 row normalisation of an .npz bank is the identity).  ``geo_graded``:
    each queried axis holds one row at the axis and 2^(k/16) rows at 15/16 of it (similarity 15/16, weight
    2^(-k/16), l_geo = 2).  An .npz bank cannot carry either - its reader divides the keys by their float32
    norm and derives unit locations from lon / lat - a prepared bank file (range_amd.bankfile) carries both:
    its arrays are uploaded as written."""
    rng = np.random.default_rng(seed)
    cls = list(dense_classes(n, k) if classes is None else classes)
    sizes = np.array([sum(c) for c in cls], np.int64)
    assert sizes.sum() == n and len(cls) <= N_DENSE_DIRS and all(1 <= len(c) <= 3 for c in cls)
    dirs = rng.permutation(N_DENSE_DIRS)[: len(cls)].astype(np.int64)
    sem_sorted = np.repeat(np.arange(len(cls)), sizes)
    grade_sorted = np.concatenate([np.full(m, GRADE * j, np.int64) for c in cls for j, m in enumerate(c)])
    perm = rng.permutation(n)
    if top_last:
        perm = np.concatenate([perm[grade_sorted[perm] != 0], perm[grade_sorted[perm] == 0]])
    sem, grade = sem_sorted[perm], grade_sorted[perm]
    h = _hadamard(dirs[sem])
    flipped = h.copy()
    width = FLIP_COLS[1] - FLIP_COLS[0]
    pick = FLIP_COLS[0] + np.argsort(rng.random((n, width)), axis=1)[:, : 2 * GRADE]
    flip = np.arange(2 * GRADE)[None, :] < grade[:, None]                # the first d of a row's seeded columns
    flipped[np.nonzero(flip)[0], pick[flip]] *= -1.0
    keys = (flipped / 16.0).astype(np.float32)
    if perturb:
        keys = _perturbed(keys, h, rng, KEY_PERT_COLS)
    assert float(np.linalg.norm(keys.astype(np.float64), axis=1).max()) < 1.0005
    n_geo_graded = 1 << (k // 16)
    gq = [1 + n_geo_graded] * 3 if geo_graded else _geo_sizes(n, geo_cap)
    rest = n - sum(gq)
    assert rest >= 0
    gs = np.array(gq + [rest - 2 * (rest // 3), rest // 3, rest // 3], np.int64)
    geo = np.empty(n, np.int64)
    at = rng.permutation(n)
    geo[at] = np.repeat(np.arange(6), gs)
    xyz = AXES[geo].copy()
    gw = np.ones(n)
    if geo_graded:                                     # all but the first row of each queried axis
        graded = np.concatenate([at[gs[:a].sum() + 1: gs[: a + 1].sum()] for a in range(N_GEO_QUERIED)])
        xyz[graded] *= np.float32(1.0 - GEO_GRADE)
        gw[graded] = 2.0 ** (-k * GEO_GRADE)
    v = dense_values(np.arange(n))
    w = np.exp2(-float(k) * grade / 128.0)
    sem_sum = np.zeros((len(cls), VAL_DIM))
    geo_sum = np.zeros((6, VAL_DIM))
    np.add.at(sem_sum, sem, w[:, None] * v)          # (multiples of 2^-21 below 2^20: exact in float64)
    np.add.at(geo_sum, geo, gw[:, None] * v)
    bank = ExactBank(n, keys, v.astype(np.float32), xyz, sem, geo, dirs, sizes, gs, sem_sum, geo_sum,
                     grade=grade, k=k)
    if geo_graded:
        bank.geo_l = np.bincount(geo, weights=gw, minlength=6)
    bank.sem_l = _class_stats(bank, float(k), False)[1]
    assert all(math.log2(x) == round(math.log2(x)) for x in bank.sem_l), "a class's l is not a power of two"
    return bank


# -- the any-order float32 pipeline, and the arithmetic faults it can carry -------------------------
DEFECTS = ("v16", "v8", "k_bf16", "q_bf16", "tf32", "drop_col255", "mispair", "k_ulp", "exp2_trunc4",
           "l_missing_grade", "v_swap_cols", "grade_wrong_row")


def _keep_bits(x: np.ndarray, bits: int) -> np.ndarray:
    """float32 truncated to ``bits`` significant bits."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return (u & np.uint32((0xFFFFFFFF << (24 - bits)) & 0xFFFFFFFF)).view(np.float32)


def _round_bf16(x: np.ndarray) -> np.ndarray:
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def _fma32(a, b, c):
    """float32 a * b + c with one rounding (the product of two float32 is exact in float64)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _sum_in_parts(terms, shape, order: np.ndarray, parts: int) -> np.ndarray:
    """float32 sum of ``terms(i)`` (i in ``order``) dealt round-robin to ``parts`` accumulators, which
    are added up afterwards: every addition rounds to float32."""
    acc = np.zeros((parts,) + tuple(shape), np.float32)
    for pos, i in enumerate(order):
        acc[pos % parts] += terms(int(i))
    out = acc[0]
    for p in range(1, parts):
        out = out + acc[p]
    return out


def emulate(bank: ExactBank, q: Queries, beta: float, tau_sem: float, tau_geo: float, seed: int = 0,
            parts: int = 1, sharp: bool = False, defect: Optional[str] = None):
    """The retrieval as a correct float32 pipeline computes it - similarities (256-long chains),
    weights exp2(fma(s, k, -m)), l and w @ V, each accumulated in float32 in a seeded random order
    over ``parts`` partial sums - or, ``defect``, with one planted arithmetic fault (DEFECTS).
    Returns ((B,4) statistics, (B,1024) output), float32."""
    assert defect is None or defect in DEFECTS, defect
    rng = np.random.default_rng(seed)
    f32 = np.float32
    K, E, V = bank.keys.copy(), q.e32.copy(), bank.values.copy()
    B, n = E.shape[0], bank.n
    geo = tau_geo > 0
    if defect in ("v16", "v8"):
        V = _keep_bits(V, 16 if defect == "v16" else 8)
    if defect == "k_bf16":
        K = _round_bf16(K)
    if defect == "q_bf16":
        E = _round_bf16(E)
    if defect == "tf32":
        K, E = _keep_bits(K, 11), _keep_bits(E, 11)
    if defect == "drop_col255":
        K[:, 255] = 0.0
    if defect == "mispair":                                  # q[i] meets k[i ^ 1] inside the chunk of columns 0..3
        K[:, [0, 1, 2, 3]] = K[:, [1, 0, 3, 2]]
    if defect == "v_swap_cols":
        V[:, [5, 6]] = V[:, [6, 5]]
    s = _sum_in_parts(lambda c: E[:, c, None] * K[None, :, c], (B, n), rng.permutation(KEY_DIM), parts)
    k1 = k_shift(tau_sem)
    if defect == "k_ulp":
        k1 = np.nextafter(k1, f32(np.inf))
    m1 = (k1 * s).max(axis=1).astype(f32) if sharp else np.full(B, k1, f32)
    t1 = _fma32(s, k1, -m1[:, None])
    if defect == "exp2_trunc4":
        t1 = (np.trunc(t1 / f32(4)) * f32(4)).astype(f32)
    e1 = np.exp2(t1).astype(f32)
    order = rng.permutation(n)
    grade = np.zeros(n, np.int64) if bank.grade is None else bank.grade     # (a one-hot bank: every row at d = 0)
    in_l = e1 * (grade != GRADE)[None, :].astype(f32) if defect == "l_missing_grade" else e1
    l1 = _sum_in_parts(lambda i: in_l[:, i], (B,), order, parts)
    st = np.zeros((B, 4), f32)
    st[:, 0], st[:, 1] = m1, l1
    if not geo:
        beta = 1.0
    w = (f32(beta) / l1)[:, None] * e1
    if geo:
        k2 = k_shift(tau_geo)
        g = q.xq[:, None, 0] * bank.xyz[None, :, 0]
        g = _fma32(q.xq[:, None, 1], bank.xyz[None, :, 1], g)
        g = _fma32(q.xq[:, None, 2], bank.xyz[None, :, 2], g)
        m2 = (k2 * g).max(axis=1).astype(f32) if sharp else np.full(B, k2, f32)
        e2 = np.exp2(_fma32(g, k2, -m2[:, None])).astype(f32)
        l2 = _sum_in_parts(lambda i: e2[:, i], (B,), rng.permutation(n), parts)
        st[:, 2], st[:, 3] = m2, l2
        w = _fma32(((f32(1.0) - f32(beta)) / l2)[:, None], e2, w)
    if defect == "grade_wrong_row":                          # the weight of row i ^ 1 of its 16-row block
        w = w[:, np.minimum(np.arange(n) ^ 1, n - 1)]
    out = _sum_in_parts(lambda i: w[:, i, None] * V[None, i, :], (B, VAL_DIM), rng.permutation(n), parts)
    return st, out
