#!/usr/bin/env python3
"""Stage times of the cluster map (range_amd/cluster_map.py) at D = 256 synthetic float64 features of a smooth field
on a lon/lat grid (about H x 2H cells) that are already in HBM, for n = 4 000, 16 200 and 64 800 rows (a 1-degree grid; GPU only).
Every stage is timed with a host clock around work that ends in a device synchronise:

  normalise     E = x / |x| and the squared norms: one read and one write of n D 8 bytes;
  gemm_finish   S = E E^T (lower tiles, float64 matrix cores) and D = max(0, 1 - S) mirrored in place;
  first_scan    the first linkage round up to its pair count: the nearest neighbour of all n rows, one read of the
                n x n matrix -> GB/s;
  rounds        all the other rounds: scans of the stale rows, the three merge launches, one synchronisation each;
  cut           the stable sort and the union-find on the host, the copy of the merge record included.

Beside them (unless --no-host), where it finishes within minutes (n <= 16 200): scikit-learn's
AgglomerativeClustering(n_clusters=30, metric="cosine", linkage="complete").fit on the same normalised rows on the
host, and whether its partition is the device's.
Usage: python tools/cluster_map_bench.py [n ...] [--json] [--no-host]"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from range_amd import _cluster_native

SIZES = [int(v) for v in sys.argv[1:] if v.isdigit()] or [4000, 16200, 64800]
D = 256
K = 30
HOST_MAX = 16200
dev = torch.device("cuda:0")
eng = _cluster_native.ClusterEngine(dev)


def features(n, d, seed=1):
    """sin(P W + b) of the unit vectors P of an H x W grid (H the divisor of n nearest sqrt(n / 2)), lon end point
    excluded."""
    h0 = int(round((n / 2) ** 0.5))
    h = next(h for k in range(h0) for h in (h0 - k, h0 + k) if n % h == 0)      # the divisor of n nearest sqrt(n / 2)
    w = n // h
    g = torch.Generator(device=dev).manual_seed(seed)
    lon = torch.deg2rad(torch.arange(w, device=dev, dtype=torch.float64) * (360.0 / w) - 180.0)
    lat = torch.deg2rad(torch.linspace(89.5, -89.5, h, device=dev, dtype=torch.float64))
    lat, lon = torch.meshgrid(lat, lon, indexing="ij")
    lat, lon = lat.reshape(-1), lon.reshape(-1)
    P = torch.stack([torch.cos(lat) * torch.cos(lon), torch.cos(lat) * torch.sin(lon), torch.sin(lat)], dim=1)
    W = 2.0 * torch.randn((3, d), generator=g, device=dev, dtype=torch.float64)
    b = 6.283185307179586 * torch.rand(d, generator=g, device=dev, dtype=torch.float64)
    return torch.sin(P @ W + b)


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


rows = []
for n in SIZES:
    X = features(n, D)
    eng.reserve(n, D)
    eng.normalize(X[:64])                                    # (loads the kernels)
    row = {"rows": n, "features": D, "n_clusters": K, "matrix_GB": round(n * n * 8 / 1e9, 2)}
    (E, _), row["normalise_ms"] = clocked(lambda: eng.normalize(X))
    Dm = eng.empty((n, n))
    eng.distances(E[:256], out=Dm[:256, :256])
    eng.linkage(Dm[:256, :256])
    _, row["gemm_finish_ms"] = clocked(lambda: eng.distances(E, out=Dm))
    row["gemm_tflops"] = round(n * n * D / (row["gemm_finish_ms"] * 1e-3) / 1e12, 2)   # (the triangle: half of 2 n^2 D)
    (merges, heights, rounds), total = clocked(lambda: eng.linkage(Dm))
    first, rest = eng.stage_times()
    row["first_scan_ms"], row["rounds_ms"], row["linkage_ms"], row["rounds"] = round(first, 3), round(rest, 3), total, rounds
    row["first_scan_GBps"] = round(n * n * 8 / (first * 1e-3) / 1e9, 1)
    t0 = time.perf_counter()
    labels, Z = _cluster_native.cut(merges.cpu().numpy(), heights.cpu().numpy(), K)
    row["cut_ms"] = (time.perf_counter() - t0) * 1e3
    for key in ("normalise_ms", "gemm_finish_ms", "linkage_ms", "cut_ms"):
        row[key] = round(row[key], 3)
    del Dm
    if "--no-host" not in sys.argv and n <= HOST_MAX:
        from sklearn.cluster import AgglomerativeClustering
        Eh = E.cpu().numpy()
        t0 = time.perf_counter()
        want = AgglomerativeClustering(n_clusters=K, metric="cosine", linkage="complete").fit(Eh).labels_
        row["sklearn_host_s"] = round(time.perf_counter() - t0, 2)
        seen = {}
        want = np.array([seen.setdefault(int(v), len(seen)) for v in want])
        row["sklearn_same_partition"] = bool(np.array_equal(want, labels))
        row["sklearn_host_threads"] = int(os.environ.get("OMP_NUM_THREADS", 0)) or None
    del E, X
    torch.cuda.empty_cache()
    rows.append(row)
    print(json.dumps({"cluster_map_bench": row}) if "--json" in sys.argv else row, flush=True)
