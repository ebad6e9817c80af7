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
    """The kernels' shift m = k = (float)(tau * log2 e) (range_hip.hip: k_sem / k_geo)."""
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
    sem_sum: np.ndarray       # (n_classes,1024) float64 column sums of the class's values
    geo_sum: np.ndarray       # (6,1024) float64

    @property
    def n_classes(self) -> int:
        return int(self.sem_size.shape[0])

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


def queries(bank: ExactBank, B: int, seed: int = 1, classes: Optional[Sequence[int]] = None) -> Queries:
    """B queries: the first ones walk through every semantic class (and the non-empty queried
    axes), so that every row of the bank is asked for when B >= n_classes; the rest are drawn at
    random (seeded), so equal queries sit at many positions of the batch."""
    rng = np.random.default_rng(seed)
    cls = np.arange(bank.n_classes) if classes is None else np.asarray(classes, np.int64)
    axes = np.flatnonzero(bank.geo_size[:N_GEO_QUERIED] > 0)
    sem = np.concatenate([rng.permutation(cls), rng.choice(cls, size=max(0, B - len(cls)))])[:B]
    geo = np.concatenate([rng.permutation(axes), rng.choice(axes, size=max(0, B - len(axes)))])[:B]
    geo = geo[rng.permutation(B)]
    e32 = np.zeros((B, KEY_DIM), np.float32)
    d = bank.sem_dir[sem]
    e32[np.arange(B), d % KEY_DIM] = np.where(d >= KEY_DIM, -1.0, 1.0).astype(np.float32)
    xq = np.zeros((B, 4), np.float32)
    xq[:, :3] = AXES[geo]
    return Queries(sem, geo, e32, xq)


def lonlat_of(axes) -> np.ndarray:
    """(lon, lat) degrees of axis points (a forward's queries, an .npz bank's locations)."""
    return AXIS_LONLAT[np.asarray(axes)].copy()


def covered(bank: ExactBank, q: Queries) -> bool:
    """Every row of the bank belongs to a semantic class some query asks for."""
    return bool(np.isin(np.arange(bank.n_classes), q.sem).all())


def expect_stats(bank: ExactBank, q: Queries, tau_sem: float = TAU, tau_geo: float = TAU) -> np.ndarray:
    """(B,4) float32 {m_sem, l_sem, m_geo, l_geo} of pass 1 (geo head off: m_geo, l_geo unchecked)."""
    st = np.zeros((len(q.sem), 4), np.float32)
    st[:, 0] = k_shift(tau_sem)
    st[:, 1] = bank.sem_size[q.sem]
    st[:, 2] = k_shift(tau_geo)
    st[:, 3] = bank.geo_size[q.geo]
    return st


def expect(bank: ExactBank, q: Queries, beta: float, geo: bool = True) -> np.ndarray:
    """(B,1024) float32: beta * S_sem / P + (1 - beta) * S_geo / Q (geo head off: S_sem / P, as the
    kernels force beta = 1 then).  Asserts that the float64 value is a float32."""
    if not geo:
        beta = 1.0
    out = beta * bank.sem_sum[q.sem] / bank.sem_size[q.sem][:, None]
    if beta != 1.0:
        out = out + (1.0 - beta) * bank.geo_sum[q.geo] / bank.geo_size[q.geo][:, None]
    out32 = out.astype(np.float32)
    assert np.array_equal(out32.astype(np.float64), out), "expected retrieval is not a float32"
    return out32


def _half_ulp(x: float) -> float:
    return 2.0 ** (math.floor(math.log2(x)) - 24)


def assert_margin(n: int, P: int, Q: int, beta: float, tau_sem: float, tau_geo: float,
                  s_out: float = 0.0, g_out: float = 0.0, residue: float = 1e-6) -> None:
    """The out-of-class mass of one query (semantic class of P rows, geographic class of Q rows, n
    rows in all; out-of-class similarities at most ``s_out`` / ``g_out``, up to ``residue``) stays
    below half an ulp of the smallest in-class term of the output, and of l_sem / l_geo: round-to-
    nearest absorbs it at every addition, in any order.  Geo head off: tau_geo <= 0."""
    assert 1 <= P <= 1 << 17 and P & (P - 1) == 0, P
    geo = tau_geo > 0
    if not geo:
        beta = 1.0
    assert beta in (0.0, 0.25, 0.5, 0.75, 1.0), beta
    # (a head of weight 0 does not enter the output at all: 0 * finite = 0)
    ca, cb, mass = beta / P, 0.0, 0.0
    if ca > 0:
        w1 = 2.0 ** (float(k_shift(tau_sem)) * (s_out + residue - 1.0))   # heaviest out-of-class weight
        assert (n - P) * w1 < _half_ulp(P), "l_sem: out-of-class mass not absorbed"
        mass += 2.0 * ca * (n - P) * w1                  # values are at most 2
    if geo and beta < 1.0:
        assert 1 <= Q <= 1 << 17 and Q & (Q - 1) == 0, Q
        w2 = 2.0 ** (float(k_shift(tau_geo)) * (g_out + residue - 1.0))
        assert (n - Q) * w2 < _half_ulp(Q), "l_geo: out-of-class mass not absorbed"
        cb = (1.0 - beta) / Q
        mass += 2.0 * cb * (n - Q) * w2
    smallest = min(c for c in (ca, cb) if c > 0)
    assert mass < _half_ulp(smallest), f"margin: out-of-class mass {mass:.3e} vs half ulp {_half_ulp(smallest):.3e}"


def assert_bank_margin(bank: ExactBank, q: Queries, beta: float, tau_sem: float = TAU,
                       tau_geo: float = TAU) -> None:
    """``assert_margin`` for every (semantic class, axis) pair the queries ask for."""
    for c, a in set(zip(q.sem.tolist(), q.geo.tolist())):
        assert_margin(bank.n, int(bank.sem_size[c]), int(bank.geo_size[a]), beta, tau_sem, tau_geo)


def topk_expect(bank: ExactBank, q: Queries, k: int):
    """Exact top-k of each query (ties to the lower row): its class's lowest rows (similarity 1),
    then - a class smaller than k - the lowest orthogonal rows (0).  (B,k) values, indices."""
    B = len(q.sem)
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
