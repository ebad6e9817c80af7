"""What the context-lifecycle tests share (test_lifecycle_cpu.py, test_gpu_lifecycle.py,
test_gpu_lifecycle_side.py): poisoned predecessor banks, the exact banks and queries that follow them, the
table of setters with the test that REPLACES what each one installed, and the parser behind that table.

A ``range_ctx`` lives long: its device buffers only grow and are never cleared, and a handful of validity
words decide whose contents may be read.  A defect there shows on the second use of a context only.  The
method: a context first holds a *poison* bank - unit keys on every one-hot direction the exact banks of
tools/exact_bank.py use, locations on all six axes, values no exact answer survives - and then an exact bank
that is smaller.  Every query of the successor has similarity exactly 1 with many poison rows that still sit
behind the successor's padded rows in the same allocation, so one stale row, bf16 / fp16 key tile, plane or
kept logit that reaches a result changes it by at least one in-class term, and ``torch.equal`` sees it.
"""
from __future__ import annotations

import functools
import os
import re
from typing import Dict, List

import numpy as np

from tools import exact_bank as X

BLK = 16                          # rows of a bank block: n_pad = the next multiple
TAU = X.TAU                       # every head of the exact banks at the widest constant-shift gap
TAU2 = 40.0                       # stats_kept's second temperature (m = k(40), l = the class size still)
TAU_SHARP = 48.0                  # above 43: the running-maximum pass 1
BETA = 0.5
KINDS = ("huge", "one", "nan")
PRED_N = 12500                    # the poisoned predecessor
SUCCESSORS = (4099, 17, 1)        # ... and what replaces it
GROWTH = (17, 12500, 50001)       # back up: the last crosses from the stream-K walk to bank splits
ROUTE_B = 257                     # queries of the engine walk: four tiles and one query
TOPK_B = (16, 33, 257)            # topk_stream: fused, streaming, the batch-scale fp16 route
FORWARD_B = (5, 33, 257)          # forward: one pass, two passes
FLT_MAX = np.float32(np.finfo(np.float32).max)


def n_pad(n: int) -> int:
    return (n + BLK - 1) // BLK * BLK


def poison_bank(n: int, kind: str):
    """(keys, values, xyz) of ``n`` rows: row i has the key +-e_j of direction i mod 512 (tools/exact_bank.py:
    direction_vector) and sits on axis i mod 6; values +-FLT_MAX in alternation (``huge``), 3.0 (``one``: a
    stale row shows as a small wrong number, not as an overflow) or NaN (``nan``: a stale row read under a
    weight of zero shows too)."""
    assert kind in KINDS, kind
    i = np.arange(n)
    d = i % X.N_DIRS
    keys = np.zeros((n, X.KEY_DIM), np.float32)
    keys[i, d % X.KEY_DIM] = np.where(d >= X.KEY_DIM, -1.0, 1.0).astype(np.float32)
    xyz = X.AXES[i % 6].copy()
    if kind == "huge":
        values = np.where((i[:, None] + np.arange(X.VAL_DIM)[None, :]) % 2 == 0, FLT_MAX, -FLT_MAX).astype(np.float32)
    elif kind == "one":
        values = np.full((n, X.VAL_DIM), 3.0, np.float32)
    else:
        values = np.full((n, X.VAL_DIM), np.nan, np.float32)
    return keys, values, xyz


@functools.lru_cache(maxsize=None)
def exact(n: int) -> X.ExactBank:
    """The exact bank of ``n`` rows of every lifecycle test (seed n: banks of different sizes differ in the
    directions of their classes too)."""
    return X.build(n, seed=n)


@functools.lru_cache(maxsize=None)
def route_queries(n: int, B: int = ROUTE_B) -> X.Queries:
    return X.queries(exact(n), B, seed=n + B)


def topk_k(n: int) -> int:
    return min(16, n)


FORWARD_CLASS = 0                 # the class of the constant-e-hat encoder on every exact bank: the first (largest)


def forward_queries(n: int, B: int) -> X.Queries:
    return X.forward_queries(exact(n), FORWARD_CLASS, B, seed=B)


# -- workspaces filled by a larger call (n = PRED_N): the large call asks for other classes than the small ones
WS_N = PRED_N
WS_BIG_B = 4097
WS_SMALL_B = (1, 17, 33, 65)
WS_MID_B = 257
WS_OVERLAP_B = (700, 130, 700)


def ws_classes(big: bool) -> np.ndarray:
    c = np.arange(exact(WS_N).n_classes)
    return c[c % 2 == (0 if big else 1)]


@functools.lru_cache(maxsize=None)
def ws_queries(B: int, big: bool) -> X.Queries:
    return X.queries(exact(WS_N), B, seed=B + (1000 if big else 0), classes=ws_classes(big))


def ws_forward_class(big: bool) -> int:
    """The constant-e-hat encoder's class in the large call's forward and in the small calls'."""
    return int(ws_classes(big)[0])


def ws_forward_queries(B: int, big: bool) -> X.Queries:
    return X.forward_queries(exact(WS_N), ws_forward_class(big), B, B)


def premises():
    """Every (what, bank, queries, beta, tau_sem, tau_geo, stats_only) the GPU files compare bit for bit on the
    one-hot banks: the host checks ``assert_bank_margin`` on each before a device is asked."""
    for n in sorted(set(SUCCESSORS + GROWTH)):
        b, q = exact(n), route_queries(n)
        yield f"routes n={n}", b, q, BETA, TAU, TAU, False
        yield f"stats_kept n={n}", b, q, BETA, TAU2, TAU2, True
        for B in FORWARD_B:
            yield f"forward n={n} B={B}", b, forward_queries(n, B), BETA, TAU, TAU, False
    b = exact(WS_N)
    for B in (WS_BIG_B,) + WS_SMALL_B + (WS_MID_B,):
        for big in (True, False):
            yield f"workspace B={B} big={big}", b, ws_queries(B, big), BETA, TAU, TAU, False
            yield f"workspace forward B={B} big={big}", b, ws_forward_queries(B, big), BETA, TAU, TAU, False
    for i, B in enumerate(WS_OVERLAP_B):
        yield f"overlap forward B={B} call {i}", b, ws_forward_queries(B, i != 1), BETA, TAU, TAU, False
    for B in sorted(set(WS_OVERLAP_B)) + [WS_BIG_B, 33]:
        q = forward_queries(WS_N, B)
        yield f"forward n={WS_N} B={B}", b, q, BETA, TAU, TAU, False
        # set_temperatures(48, 0): the semantic head sharp, the geographic one at its default 40; the defaults
        # (12, 40) with beta = 0 - the geographic head alone
        yield f"forward sharp n={WS_N} B={B}", b, q, BETA, TAU_SHARP, 40.0, False
        yield f"forward default n={WS_N} B={B}", b, q, 0.0, 12.0, 40.0, False


# -- model level (load_model on a prepared bank of MODEL_N rows)
MODEL_N = 4099
MODEL_B = (1, 16, 17, 32, 33, 256, 257, 512, 513, 4097)
MODEL_BETAS = (0.25, 0.75)


def model_premises():
    b = exact(MODEL_N)
    for B in MODEL_B:
        q = X.forward_queries(b, FORWARD_CLASS, B, B)
        for beta in (BETA,) + MODEL_BETAS:
            yield f"model B={B} beta={beta}", b, q, beta, TAU, TAU, False
        yield f"model sharp B={B}", b, q, BETA, TAU_SHARP, TAU, False
        yield f"model RANGE B={B}", b, q, 1.0, TAU, 0.0, False


# -- set_temperatures on the dense banks (tests/exact_dense_cases.py): k = 48 (constant shift), k = 64 (sharp), 48 again
DENSE_TEMPS = (("n108", X.dense_tau(48), 0.25), ("s108", X.dense_tau(64), 0.5), ("n108", X.dense_tau(48), 0.25))
DENSE_TEMPS_B = (17, 65)


def dense_forward_class(name: str) -> int:
    """The constant-e-hat encoder's class on a dense bank: the first graded class (the largest)."""
    import exact_dense_cases as D
    return int(np.argmax(D.bank(name).sem_size))


# -- the setters and the test that replaces what each installed ---------------------------------------------
HEADERS = ("range_hip.h", "range_neighbors.h", "range_probe.h", "range_map.h", "range_cluster.h")

#: entry point -> (test module, test function) that calls it on a context which already holds an earlier
#: installation of the same kind and checks what comes out afterwards
SETTER_CASES: Dict[str, tuple] = {
    "range_set_encoder": ("test_gpu_lifecycle", "test_encoder_replaced"),
    "range_set_sh_table": ("test_gpu_lifecycle", "test_encoder_replaced"),
    "range_set_bank": ("test_gpu_lifecycle", "test_bank_shrinks"),
    "range_set_keys": ("test_gpu_lifecycle", "test_set_keys_and_set_bank_alternate"),
    "range_set_pv_mode": ("test_gpu_lifecycle", "test_pv_mode_flips"),
    "range_set_temperatures": ("test_gpu_lifecycle", "test_temperatures_flip"),
    "range_set_csp": ("test_gpu_lifecycle_side", "test_csp_network_replaced_behind_a_head"),
    "range_set_csp_head": ("test_gpu_lifecycle_side", "test_csp_network_replaced_behind_a_head"),
    "range_set_neighbors": ("test_gpu_lifecycle_side", "test_neighbor_sets_shrink_and_change_kind"),
    "range_set_kde_points": ("test_gpu_lifecycle_side", "test_neighbor_sets_shrink_and_change_kind"),
    "range_map_reserve": ("test_gpu_lifecycle_side", "test_probe_context_reserved_large_then_used_small"),
    "range_cluster_reserve": ("test_gpu_lifecycle_side", "test_probe_context_reserved_large_then_used_small"),
}


def setter_entry_points() -> Dict[str, List[str]]:
    """Per public header the functions named ``range_set_*`` or ``range_*_reserve`` it declares (the headers
    parsed as text, comments removed - the approach of stream_order.stream_entry_points)."""
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    found = {}
    for header in HEADERS:
        with open(os.path.join(inc, header)) as f:
            text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
        text = re.sub(r"//[^\n]*", " ", text)
        found[header] = [m.group(1) for m in re.finditer(r"\b(range_\w+)\s*\(([^()]*)\)\s*;", text)
                         if re.match(r"range_set_\w+$|range_\w+_reserve$", m.group(1))]
    return found


# -- a planted defect on the host: one stale row admitted -----------------------------------------------------
def with_stale_rows(bank: X.ExactBank, kind: str, rows) -> X.ExactBank:
    """``bank`` followed by the given rows of its poisoned predecessor - what a kernel computes that reads
    them: the emulator's input (X.emulate reads n, keys, values, xyz, grade)."""
    import dataclasses
    keys, values, xyz = poison_bank(PRED_N, kind)
    rows = np.asarray(rows, np.int64)
    return dataclasses.replace(bank, n=bank.n + len(rows), keys=np.concatenate([bank.keys, keys[rows]]),
                               values=np.concatenate([bank.values, values[rows]]),
                               xyz=np.concatenate([bank.xyz, xyz[rows]]))
