#!/usr/bin/env python3
"""The checkerboard task's nearest-support scan (range_nearest_support) at 10 000 x 200 (a task's train set),
10 000 x 10 000 and 10^6 x 10^4 (an evaluation lattice) queries x supports (GPU only).  Per shape, after a warm-up
of at least 0.3 s of the same launch (which also ramps the clock), the median / min / max of HIP-event times of
single calls (scan + merge where the plan splits the support), and from the median:
  pairs/s          Q * S over the time;
  share of the float64 vector issue rate: pairs/s * F64_PER_PAIR over 39.3e12 float64 lane-instructions/s (256 CUs
                   x 4 SIMDs x 16 lanes per clock at 2.4 GHz: the 78.6 TFLOP/s FP64 vector rate counts an FMA twice).
                   F64_PER_PAIR = 96 float64 instructions (of 124 vector instructions) were counted in the
                   compiler's listing of the pair loop (hipcc -S, gfx950) on its common path - both half-differences
                   below the large-argument threshold of the library's sin; its reduction and both polynomials are
                   in that count.  A bound by instruction issue, not a FLOP count.
For the first two shapes the numpy restatement of the reference's matrix (float64, in blocks of 2 000 queries to
bound its memory) is timed on the host, once, and the GPU's indices are compared with it.
Usage: python tools/checker_bench.py [repeats] [--json] [--no-host]"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from range_amd import _native, checker

args = [v for v in sys.argv[1:] if v.isdigit()]
REPEATS = int(args[0]) if args else 20
F64_PER_PAIR, VALU_PER_PAIR = 96, 124
F64_LANE_RATE = 256 * 4 * 16 * 2.4e9
dev = torch.device("cuda:0")
eng = _native.HipEngine(dev)


def lattice_rad(n):
    lons, lats, _ = checker.generate_fibonaccilattice(n)
    return np.radians(np.stack([lons, lats], axis=1))


def samples_rad(n, seed):
    return np.radians(np.stack(checker.random_samples(n, seed), axis=1))


def host_argmin(q, s, block=2000):
    """The reference's matrix and arg-min in numpy, float64, `block` queries at a time."""
    out = np.empty(len(q), dtype=np.int64)
    c2 = np.cos(s[:, 1])
    for a in range(0, len(q), block):
        lon1, lat1 = q[a:a + block, 0], q[a:a + block, 1]
        dlon, dlat = s[:, 0][:, None] - lon1, s[:, 1][:, None] - lat1
        h = np.sin(dlat / 2) ** 2 + np.cos(lat1) * c2[:, None] * np.sin(dlon / 2) ** 2
        c = 2 * np.arctan2(np.sqrt(h), np.sqrt(1 - h))
        out[a:a + block] = c.argmin(0)
    return out


def timed(fn, repeats, warm_seconds=0.3):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warm_seconds:
        fn()
        torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


rows = []
for Q, S, grid, reps in ((10_000, 200, False, REPEATS), (10_000, 10_000, False, REPEATS), (1_000_000, 10_000, True, max(3, REPEATS // 4))):
    q_host = lattice_rad(Q) if grid else samples_rad(Q, 0)
    s_host = lattice_rad(S)
    q, s = torch.from_numpy(q_host).to(dev), torch.from_numpy(s_host).to(dev)
    idx, dist = eng.nearest_support(q, s)
    med, lo, hi = timed(lambda: eng.nearest_support(q, s), reps)
    pairs = Q * S
    row = {"queries": Q, "supports": S, "pairs": pairs, "median_us": round(med, 1), "min_max_us": [round(lo, 1), round(hi, 1)],
           "repeats": reps, "pairs_per_s": float(f"{pairs / (med * 1e-6):.4g}"),
           "share_of_f64_vector_issue": round(pairs / (med * 1e-6) * F64_PER_PAIR / F64_LANE_RATE, 4),
           "f64_instructions_per_pair": F64_PER_PAIR, "vector_instructions_per_pair": VALU_PER_PAIR}
    if Q * S <= 10 ** 8 and "--no-host" not in sys.argv:
        t0 = time.perf_counter()
        ref = host_argmin(q_host, s_host)
        row["host_numpy_s"] = round(time.perf_counter() - t0, 3)
        row["host_over_gpu"] = round(row["host_numpy_s"] / (med * 1e-6), 1)
        row["indices_equal_host"] = bool(np.array_equal(idx.cpu().numpy(), ref))
    rows.append(row)
    if "--json" not in sys.argv:
        print(row, flush=True)
if "--json" in sys.argv:
    print(json.dumps({"checker_bench": rows}))
