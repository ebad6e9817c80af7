#!/usr/bin/env python3
"""The positional-encoder kernel (range_posenc_features) for the six kinds at 10^6 locations (GPU only):
HIP-event time per launch, GB/s written and the ratio to a plain device fill of the same bytes on the
same GPU, and the time of the numpy restatement (tests/posenc_refs.py) on 16 host threads for 10^5
locations.  A sample of every result is checked against the restatement.
Usage: python tools/posenc_bench.py [locations [repeats]] [--json]"""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

import posenc_refs as R
from range_amd import _native, posenc
from tools import synth

args = [v for v in sys.argv[1:] if v.isdigit()]
B = int(args[0]) if args else 1_000_000
REPEATS = int(args[1]) if len(args) > 1 else 20
HOST_B, HOST_THREADS = 100_000, 16
dev = torch.device("cuda:0")


def timed_us(fn, repeats=REPEATS, warmup=3):
    """Mean time of ``fn()`` in microseconds: ``repeats`` calls back to back between one pair of events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeats):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / repeats


def host_seconds(kind, q, f):
    """The numpy restatement over ``HOST_THREADS`` threads (numpy's sin / cos release the GIL), rows in chunks."""
    chunks = np.array_split(np.arange(q.shape[0]), HOST_THREADS * 4)
    with ThreadPoolExecutor(HOST_THREADS) as pool:
        t0 = time.perf_counter()
        list(pool.map(lambda idx: R.encode(kind, q[idx], f), chunks))
        return time.perf_counter() - t0


eng = _native.HipEngine(dev)
q = synth.make_queries(B, seed=7, lat_max=90.0)
x = torch.from_numpy(q).to(dev)
rows = []
for name, spec in posenc.MODELS.items():
    kind, f = R.KIND_OF_MODEL[name], posenc.freq_list(name)
    out = torch.empty((B, spec.width), dtype=torch.float64, device=dev)
    nbytes = out.numel() * 8
    row = {"model": name, "locations": B, "width": spec.width, "bytes": nbytes}
    fill_us = timed_us(lambda: out.fill_(0.5))
    row["fill_us"], row["fill_GBps"] = round(fill_us, 1), round(nbytes / fill_us / 1e3, 1)
    us = timed_us(lambda: eng.posenc_features(x, spec.kind, f, out=out))
    row.update({"us": round(us, 1), "GBps": round(nbytes / us / 1e3, 1), "of_fill": round(fill_us / us, 3)})
    sample = torch.linspace(0, B - 1, 256, dtype=torch.float64).long()
    R.assert_close(kind, out[sample.to(dev)].cpu().numpy(), R.encode(kind, q[sample.numpy()], f))
    del out
    row["numpy_16_threads_1e5_s"] = round(host_seconds(kind, q[:HOST_B], f), 3)
    rows.append(row)
    if "--json" not in sys.argv:
        print(row, flush=True)
if "--json" in sys.argv:
    print(json.dumps({"posenc_bench": rows}))
