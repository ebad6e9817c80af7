"""The SatCLIP location encoder (encoder_kernel.h; range_set_encoder, range_set_sh_table, range_encode[_raw]) over its
envelope beyond what the other tests run on a device: L = 41 .. 64 (a first layer of up to 4096 padded features, 33
slots in 9 rounds, orders m > 40), 1 to 7 hidden layers, every kernel width, 32-query workgroups at every width that
has them.  tests/test_enc_sweep_cpu.py first shows on the CPU that the cases are discriminating and which entries of
the five launch tables of encoder_host.h they reach; tests/test_gpu_enc_sweep.py runs them on the device.  A network
reaches a GPU test only through this module - its weights through ``weights``, its rows through ``queries``, its
reference through ``oracle``, its bound through ``bound`` - so the two files cannot drift apart.

The bound is the project's rule for this encoder (tests/test_gpu_parity.py, tests/test_gpu_round2.py): 2e-12 against
the float64 oracle, 4e-12 where the kernel width exceeds 512.  ``encode_ld`` restates the oracle in 80-bit long
double; the CPU test holds the oracle within a tenth of the bound of it for every case here."""
import functools
import math
import os
import re
import subprocess

import numpy as np

from oracle import range_oracle as O
from tools import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
N_CU = 256                       # the CU count the coverage statement is made for (MI355X)
KERNEL_WIDTHS = (64, 128, 192, 256, 320, 384, 448, 512, 768, 1024)

# name: (L, hidden, hidden_layers, mode, batches).  With 256 CUs the batches reach (tests/native/enc_sweep_plan.cpp):
#   B = 1, 17     one and two tiles: the one-launch tile kernel with 7 K parts (two-layer nets up to 512 wide), else
#                 the first-layer part kernels with S x KP workgroups a tile + the rest kernel
#   B = 300       19 tiles: S x KP mixes of 2..13 workgroups a tile
#   B = 600       38 tiles: the 33..128-tile form of the tile kernel (second-layer parts of 128 / 256 columns); for nets
#                 that are not two-layer the second layer over S2 > 1 column parts in a launch of its own
#   B = 1250      79 tiles: the same with 2 or 3 workgroups a tile
#   B = 3000      188 tiles: the main kernel in 16-query workgroups (no split fits the CUs)
SWEEP = {
    # the round-count steps 6 -> 7 -> 8 -> 9 (n_slots 21 | 24 25 | 28 29 | 32 33) and odd / even L
    "L41_H64_n1":     (41, 64, 1, "analytic", (1, 17, 300, 600, 3000)),
    "L47_H128_n2":    (47, 128, 2, "closed-form", (17, 300, 600, 1250, 3000)),
    "L48_H128_n3":    (48, 128, 3, "closed-form", (1, 300, 600, 1250)),
    "L55_H192_n2":    (55, 192, 2, "analytic", (17, 300, 3000)),
    "L56_H320_n4":    (56, 320, 4, "closed-form", (1, 300, 1250)),
    "L57_H256_n2":    (57, 256, 2, "closed-form", (17, 300, 600, 1250, 3000)),
    "L63_H768_n5":    (63, 768, 5, "analytic", (17, 300, 1250)),
    "L64_H64_n2":     (64, 64, 2, "closed-form", (1, 17, 300, 600, 1250, 3000)),
    "L64_H256_n7":    (64, 256, 7, "analytic", (17, 300, 600, 1250)),
    "L64_H512_n2":    (64, 512, 2, "analytic", (1, 17, 300, 600, 1250, 3000)),
    "L64_H1024_n2":   (64, 1024, 2, "closed-form", (17, 300, 1250)),
    "L64_H600_n2":    (64, 600, 2, "closed-form", (17, 300)),                 # runs zero-padded at 768
    "L63_H384_n3":    (63, 384, 3, "closed-form", (17, 300, 3000)),
    "L48_H448_n1":    (48, 448, 1, "analytic", (1, 300)),
    "L56_H512_n3":    (56, 512, 3, "analytic", (17, 600, 1250)),
    "L55_H1024_n4":   (55, 1024, 4, "analytic", (1, 600)),
    "L10_H64_n7":     (10, 64, 7, "analytic", (1, 17, 600, 3000)),            # depth only
}
# 32-query workgroups (n_wg32 > 0, the QT = 2 LDS layout) at every width that has them.  Widths with a split:
# B = 9000 = 256 x 32 + a split tail of 808; widths without: B = 5000 = 157 x 32, the last holding 8 queries, and
# B = 9000 = 256 x 32 + 51 x 16
WG32 = {
    "wg32_H64":      (10, 64, 2, "analytic", (9000,)),
    "wg32_H128":     (10, 128, 2, "closed-form", (9000,)),
    "wg32_H192":     (10, 192, 2, "analytic", (5000, 9000)),
    "wg32_H256":     (10, 256, 3, "closed-form", (9000,)),
    "wg32_H320":     (10, 320, 2, "analytic", (5000, 9000)),
    "wg32_H384":     (10, 384, 2, "closed-form", (5000, 9000)),
    "wg32_H448":     (10, 448, 1, "analytic", (5000, 9000)),
    "wg32_H512":     (10, 512, 2, "closed-form", (9000,)),
    "wg32_L64_H128": (64, 128, 2, "analytic", (9000,)),
    "wg32_L64_H320": (64, 320, 2, "closed-form", (5000,)),
}
# the reference's generated polynomials (range_amd.sh_table.generate_table(L)) beyond L = 40: 200 rows within
# |lat| <= 5, where they still equal the exact basis, and 300 rows pole to pole, where they mean nothing
TABLE = {
    "table_L48": (48, 64, 2, "analytic", (200, 300)),
    "table_L64": (64, 64, 2, "analytic", (200, 300)),
}
TABLE_NEAR_EQUATOR, TABLE_POLE_TO_POLE = 200, 300
CASES = {**SWEEP, **WG32, **TABLE}
# the L > 40 cases that run on three engines (default, RANGE_ENC_SPLIT=0, RANGE_ENC_FUSED=0), at B = 300 and 1250
ROUTES = tuple(n for n, c in SWEEP.items() if c[0] > 40)
ROUTE_BATCHES = (300, 1250)
# one engine takes these in turn; each result is that of a fresh engine
IN_TURN = ("L64_H1024_n2", "L10_H64_n7", "L64_H256_n7", "L41_H64_n1")
FORWARD_CASE, FORWARD_BANK_ROWS, FORWARD_BATCHES = "L64_H64_n2", 500, (33, 300)

# Entries of the launch tables no plan reaches: ENC_REST runs behind the first-layer part kernels only, and a hidden
# width splits into parts only where H / S is 64, 128, 256 or 512 for a power of two S (host_plan.h:
# choose_encoder_split and split_width_ok) - 384 = 6 x 64 and 768 = 12 x 64 have no such S, so these two widths always
# take encoder_kernel (ENC_MAIN).  The CPU test checks over the whole plan sweep that no batch reaches them.
UNREACHABLE = {("ENC_REST", 6), ("ENC_REST", 12)}

# max |oracle - the reference's closed-form encoder| over the fixture's 128 rows, after normalising, measured on the
# CPU on 2026-10-21 with `python -m pytest tests/test_enc_sweep_cpu.py -k fixtures -s` (which prints the value measured
# now): 1.10e-15 and 8.71e-15, recorded with a few ulp of 1 (1.1e-16 each) to spare for another BLAS's summation order
# in the oracle's Siren.  The fixtures are written by tests/golden/make_golden_enc_sweep.py.  The GPU test allows
# 4 x this + the kernel's bound.
E_GOLDEN = {
    "enc_closedform_L48_H128_n3": 1.5e-15,
    "enc_closedform_L64_H64_n2": 1.0e-14,
}
FIXTURE_SEED = {"enc_closedform_L48_H128_n3": 4801, "enc_closedform_L64_H64_n2": 6401}
FIXTURE_ROWS = 128


def seed_of(name):
    """The weight seed of a case: its shape and its place in its table."""
    L, hidden, layers, _, _ = CASES[name]
    return 1000000 * L + 1000 * hidden + 10 * layers + (name in WG32) + 2 * (name in TABLE)


@functools.lru_cache(maxsize=None)
def weights(name):
    L, hidden, layers, _, _ = CASES[name]
    return synth.make_encoder_weights(L, hidden, 256, layers, seed_of(name))


def weight_lists(w):
    n = len([k for k in w if k.startswith("layers.") and k.endswith(".weight")])
    return ([w[f"layers.{i}.weight"] for i in range(n)] + [w["last_layer.weight"]],
            [w[f"layers.{i}.bias"] for i in range(n)] + [w["last_layer.bias"]])


FIXED_ROWS = np.array([[12.5, 0.0], [-77.0, 0.001], [40.0, 90.0], [-40.0, -90.0], [-180.0, 3.0], [180.0, -3.0],
                       [-0.0, -0.0]], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def queries(B, seed=0):
    """(B, 2) float64 (lon, lat): the fixed rows first (lat = 0 and 0.001, where Y(l, l) is O(1); both poles;
    lon = +-180; -0.0), then seeded rows, three quarters within |lat| <= 45 and one quarter up to 89.999, interleaved.
    Read-only: copy before changing."""
    rng = np.random.default_rng(100003 * seed + B)
    lon = rng.uniform(-180.0, 180.0, size=B)
    lat = np.where(np.arange(B) % 4 == 3, rng.uniform(45.0, 89.999, size=B), rng.uniform(0.0, 45.0, size=B))
    lat *= rng.choice([-1.0, 1.0], size=B)
    q = np.stack([lon, lat], axis=1)
    n = min(B, len(FIXED_ROWS))
    q[:n] = FIXED_ROWS[:n]
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def equator_queries(B, seed=0):
    """(B, 2): |lat| <= 5, lat = 0 and 0.001 among them.  Read-only."""
    rng = np.random.default_rng(200003 * seed + B)
    q = np.stack([rng.uniform(-180.0, 180.0, size=B), rng.uniform(-5.0, 5.0, size=B)], axis=1)
    q[:2] = FIXED_ROWS[:2]
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def table(L):
    """range_amd.sh_table.generate_table(L) (4.5 s at L = 64): once."""
    from range_amd import sh_table
    return sh_table.generate_table(L)


@functools.lru_cache(maxsize=None)
def oracle(name, B, seed=0):
    """O.encode of the case on ``queries(B, seed)``: computed once, read-only."""
    L, _, _, mode, _ = CASES[name]
    e = O.encode(queries(B, seed), weights(name), L, mode)
    e.setflags(write=False)
    return e


def bound(name):
    return 4e-12 if kernel_hidden_width(CASES[name][1]) > 512 else 2e-12


def kernel_hidden_width(hidden):
    """host_plan.h: kernel_hidden_width."""
    assert 1 <= hidden <= 1024
    return (hidden + 63) // 64 * 64 if hidden <= 512 else (768 if hidden <= 768 else 1024)


# ---- the long-double restatement ------------------------------------------------------------------------------
LD = np.longdouble


def features_ld(lonlat, L, mode):
    """The real spherical harmonics by the three-term recurrence, feature index l*l + l + m, conventions of the two
    modes as in the reference (analytic: pi x orthonormal for m = 0, no Condon-Shortley sign; closed-form: orthonormal
    m = 0, the sign kept).  The angles are the float64 ones every implementation starts from; everything after them is
    long double."""
    lonlat = np.asarray(lonlat, dtype=np.float64)
    phi = ((lonlat[:, 0] + 180.0) * (math.pi / 180.0)).astype(LD)
    theta = ((lonlat[:, 1] + 90.0) * (math.pi / 180.0)).astype(LD)
    pi = LD(4) * np.arctan(LD(1))
    x, s = np.cos(theta), np.abs(np.sin(theta))
    Y = np.zeros((len(phi), L * L), dtype=LD)
    c = np.sqrt(LD(1) / (LD(4) * pi))
    for m in range(L):
        if m > 0:
            c = c * np.sqrt(LD(2 * m + 1) / LD(2 * m))
        if m == 0:
            scale, cm, sm = (pi if mode == "analytic" else LD(1)), LD(1), None
        else:
            scale = np.sqrt(LD(2)) * (LD(-1) if (mode == "closed-form" and m % 2) else LD(1))
            cm, sm = np.cos(LD(m) * phi), np.sin(LD(m) * phi)
        q2 = None
        q1 = c * s ** m
        for l in range(m, L):
            if l == m:
                q = q1
            elif l == m + 1:
                q = np.sqrt(LD(2 * m + 3)) * x * q1
            else:
                a = np.sqrt(LD(4 * l * l - 1) / LD(l * l - m * m))
                b = np.sqrt(LD((l - 1) ** 2 - m * m) / LD(4 * (l - 1) ** 2 - 1))
                q = a * (x * q1 - b * q2)
            if l > m:
                q2, q1 = q1, q
            if m == 0:
                Y[:, l * l + l] = scale * q
            else:
                Y[:, l * l + l + m] = scale * q * cm
                Y[:, l * l + l - m] = scale * q * sm
    return Y


def encode_ld(lonlat, w, L, mode):
    """Features -> Siren (w0 = 30 on the first layer, 1 after it, a linear last layer) -> L2 normalisation, in long
    double; returned as float64."""
    h = features_ld(lonlat, L, mode)
    Ws, bs = weight_lists(w)
    for i in range(len(Ws) - 1):
        h = np.sin(LD(30 if i == 0 else 1) * (h @ Ws[i].astype(LD).T + bs[i].astype(LD)))
    e = h @ Ws[-1].astype(LD).T + bs[-1].astype(LD)
    return (e / np.sqrt((e * e).sum(axis=1, keepdims=True))).astype(np.float64)


# ---- planted defects: what the oracle would compute from a subtly wrong kernel ---------------------------------
def _f(l, m):
    return l * l + l + m


def _drop_highest_order(Y, w, L, mode):
    Y[:, _f(L - 1, L - 1)] = 0.0
    Y[:, _f(L - 1, -(L - 1))] = 0.0


def _odd_order_sign(Y, w, L, mode):
    m = 41                                         # the first odd order no test below L = 42 computes
    for l in range(m, L):
        Y[:, _f(l, m)] *= -1.0
        Y[:, _f(l, -m)] *= -1.0


def _swap_in_last_slot(Y, w, L, mode):
    m = L // 2                                     # the last slot's first order; degrees L - 1 and L - 2
    a, b = _f(L - 1, m), _f(L - 2, m)
    Y[:, [a, b]] = Y[:, [b, a]]


def _sincos_exchanged(Y, w, L, mode):
    a, b = _f(L - 1, L - 1), _f(L - 1, -(L - 1))
    Y[:, [a, b]] = Y[:, [b, a]]


def _w0_on_second_layer(Y, w, L, mode):
    w["layers.1.weight"] = 30.0 * w["layers.1.weight"]
    w["layers.1.bias"] = 30.0 * w["layers.1.bias"]


def _last_hidden_bias_dropped(Y, w, L, mode):
    n = len(weight_lists(w)[0]) - 1
    w[f"layers.{n - 1}.bias"] = np.zeros_like(w[f"layers.{n - 1}.bias"])


def _hidden_2_and_3_exchanged(Y, w, L, mode):
    for k in ("weight", "bias"):
        w[f"layers.1.{k}"], w[f"layers.2.{k}"] = w[f"layers.2.{k}"], w[f"layers.1.{k}"]


# name: (the change, applied in place to a copy of the features and of the weight dict; which cases it applies to)
DEFECTS = {
    "drop_highest_order": (_drop_highest_order, lambda L, layers, mode: L >= 2),
    "odd_order_sign": (_odd_order_sign, lambda L, layers, mode: L >= 42 and mode == "closed-form"),
    "swap_in_last_slot": (_swap_in_last_slot, lambda L, layers, mode: L >= 4),
    "sincos_exchanged": (_sincos_exchanged, lambda L, layers, mode: L >= 2),
    "w0_on_second_layer": (_w0_on_second_layer, lambda L, layers, mode: layers >= 2),
    "last_hidden_bias_dropped": (_last_hidden_bias_dropped, lambda L, layers, mode: True),
    "hidden_2_and_3_exchanged": (_hidden_2_and_3_exchanged, lambda L, layers, mode: layers >= 3),
}


def applicable_defects(name):
    L, _, layers, mode, _ = CASES[name]
    return [d for d, (_, applies) in DEFECTS.items() if applies(L, layers, mode)]


def encode_with_defect(name, lonlat, defect, encode=None):
    """The oracle's e-hat of the case with ``defect`` planted before its Siren (``encode``: O.encode by default)."""
    L, _, _, mode, _ = CASES[name]
    Y = O.sh_features(lonlat, L, mode)
    w = dict(weights(name))
    DEFECTS[defect][0](Y, w, L, mode)
    return (encode or O.encode)(lonlat, w, L, mode, features=Y)


# ---- the launch plan of a case, from the native program --------------------------------------------------------
PLAN_SRC = os.path.join(REPO, "tests", "native", "enc_sweep_plan.cpp")


def build_plan_program(out_dir, flags=()):
    exe = os.path.join(str(out_dir), "enc_sweep_plan")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", *flags, PLAN_SRC, "-o", exe], check=True)
    return exe


def plans(exe, rows):
    """rows of (n_cu, L, hidden, layers, split, fused, B) -> a dict of fields per row (ints; ``tables``: a set of
    (table, nt))."""
    text = "".join(" ".join(str(int(v)) for v in r) + "\n" for r in rows)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.splitlines()
    assert len(lines) == len(rows), p.stdout
    out = []
    for line in lines:
        d = dict(f.split("=", 1) for f in line.split())
        tables = {(t.split(":")[0], int(t.split(":")[1])) for t in d.pop("tables").split(",") if t}
        d = {k: int(v) for k, v in d.items()}
        d["tables"] = tables
        out.append(d)
    return out


def launch_tables():
    """The entries of the five launch tables of encoder_host.h: {table: [nt, ...]}."""
    text = open(os.path.join(REPO, "range_amd", "csrc", "encoder_host.h")).read()
    out = {}
    for m in re.finditer(r"const EncVariant (ENC_\w+)\[\] = \{(.*?)\};", text, re.S):
        out[m.group(1)] = [int(n) for n in re.findall(r"\{\s*(\d+)\s*,\s*encoder_", m.group(2))]
    return out


def case_rows(name, n_cu=N_CU):
    """The plan queries of a case's GPU runs: every batch on the default engine; for a ROUTES case the two other
    engines at ROUTE_BATCHES too."""
    L, hidden, layers, _, batches = CASES[name]
    rows = [(n_cu, L, hidden, layers, 1, 1, B) for B in batches]
    if name in ROUTES:
        rows += [(n_cu, L, hidden, layers, s, f, B) for B in ROUTE_BATCHES for s, f in ((1, 1), (0, 1), (1, 0))]
    return rows
