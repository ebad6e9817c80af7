#!/usr/bin/env python3
"""Stage times of the embedding map (range_amd/embedding_map.py) at N = 10^6 rows of D = 1280 synthetic float64
features that are already in HBM, three components (GPU only).  Every stage is warmed once and then timed with a
host clock around work that ends in a device synchronise (median of `repeats`):

  stats_centre_gram  column statistics, centring into the second copy, G = Zc^T Zc on the float64 matrix cores
                     (2 N D^2 / 2 FLOP for the lower triangle's tiles), the d x d copy to the host included;
  eigh_host          the three largest eigenpairs of the standardised Gram matrix (LAPACK, host);
  project            Y = K' (X - mean)^T: one read of N D 8 bytes -> GB/s and the share of 6.29 TB/s (the measured
                     HBM copy rate of MI355X_MICROARCH.md);
  ica_iteration      one iteration as ``ica_colors`` runs it, split into `kernel` (HIP events around the step and its
                     fold) and `round_trip` (the rest: the launch, the copy of 12 doubles, the synchronisation and the
                     3 x 3 update in numpy);
  sources_std        both source passes and the two-pass deviation;
  equalize           min/max, three histograms and three interpolation passes;
  total              one ``ica_colors`` call on the same matrix, with its iteration count.

Beside them (unless --no-host): scikit-learn's FastICA(n_components=3, random_state=2001, whiten='unit-variance',
max_iter=1000).fit(Xs).transform(Xs) on the host at N = 10^5, D = 1280, with the threads the process is given.
Usage: python tools/embedding_map_bench.py [N] [D] [repeats] [--json] [--no-host]"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from range_amd import _map_native
from range_amd.embedding_map import ica_colors, sym_decorrelation, whitening

nums = [int(v) for v in sys.argv[1:] if v.isdigit()]
N = nums[0] if len(nums) > 0 else 1_000_000
D = nums[1] if len(nums) > 1 else 1280
REPEATS = nums[2] if len(nums) > 2 else 5
C = 3
HBM_COPY_RATE = 6.29e12
dev = torch.device("cuda:0")
eng = _map_native.MapEngine(dev)


def features(n, d, seed=1):
    """Four independent non-Gaussian sources mixed into d columns plus noise, generated on the device in float64."""
    g = torch.Generator(device=dev).manual_seed(seed)
    s = torch.rand((n, 4), generator=g, device=dev, dtype=torch.float64) ** 3 - 0.25
    X = torch.randn((n, d), generator=g, device=dev, dtype=torch.float64).mul_(0.05)
    X.addmm_(s, torch.randn((4, d), generator=g, device=dev, dtype=torch.float64))
    return X


def timed(fn, repeats=REPEATS):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times))


X = features(N, D)
torch.cuda.synchronize()
row = {"rows": N, "features": D, "components": C, "repeats": REPEATS}
state = {}


def stats_centre_gram():
    mean = eng.colstats(X)[2] / N
    Zc = eng.scale_rows(X, shift=mean)
    state["G"] = eng.gemm(Zc, Zc, trans_a=True, lower_only=True).cpu().numpy()
    state["mean"] = mean


t = timed(stats_centre_gram, max(2, REPEATS // 2))
row["stats_centre_gram_ms"] = round(t * 1e3, 2)
row["gram_tflops_of_whole_stage"] = round(N * D * D / t / 1e12, 2)       # (the triangle: half of 2 N D^2)
row["eigh_host_ms"] = round(timed(lambda: state.update(zip(("std", "K", "Kp"), whitening(state["G"], N, C)))) * 1e3, 2)
Kp = torch.from_numpy(np.ascontiguousarray(state["Kp"])).to(dev)
t = timed(lambda: state.update(Y=eng.project(X, Kp, state["mean"])))
row["project_ms"] = round(t * 1e3, 3)
row["project_GBps"] = round(N * D * 8 / t / 1e9, 1)
row["project_share_of_hbm_copy_rate"] = round(N * D * 8 / t / HBM_COPY_RATE, 3)
Y = state["Y"]
eng.reserve(N, C)
W = sym_decorrelation(np.random.RandomState(2001).normal(size=(C, C)))


def iteration():
    Ab = eng.ica_step(Y, W).cpu().numpy()
    A, b = Ab[:C * C].reshape(C, C), Ab[C * C:]
    return sym_decorrelation(A / float(N) - (b / float(N))[:, None] * W)


whole = timed(iteration, 50)
ev = []
for _ in range(50):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    eng.ica_step(Y, W)
    b.record()
    b.synchronize()
    ev.append(a.elapsed_time(b) * 1e3)
row["ica_iteration_us"] = round(whole * 1e6, 1)
row["ica_iteration_kernel_us"] = round(float(np.median(ev)), 1)
row["ica_iteration_round_trip_us"] = round(whole * 1e6 - float(np.median(ev)), 1)


def sources_std():
    S0 = eng.sources(Y, W / np.sqrt(N))
    Sc = eng.scale_rows(S0, shift=eng.colstats(S0)[2] / N)
    s_std = np.sqrt(np.diagonal(eng.gemm(Sc, Sc, trans_a=True, lower_only=True).cpu().numpy()) / N)
    state["S"] = eng.sources(Y, W / s_std[:, None] / np.sqrt(N))


row["sources_std_ms"] = round(timed(sources_std) * 1e3, 3)
S = state["S"]


def equalize():
    mn, mx, _ = eng.colstats(S)
    mn, mx = mn.cpu().numpy(), mx.cpu().numpy()
    out = eng.empty((N, C))
    for k in range(C):
        eng.equalize(S[:, k], torch.from_numpy(np.linspace(mn[k], mx[k], 257)).to(dev), out=out[:, k])


row["equalize_ms"] = round(timed(equalize) * 1e3, 3)
del Y, S, state
info = {}
row["total_ms"] = round(timed(lambda: info.update(ica_colors(X, return_info=True)[1]), 2) * 1e3, 1)
row["total_n_iter"] = int(info["n_iter"])
if "--no-host" not in sys.argv:
    from sklearn.decomposition import FastICA
    n_host = min(N, 100_000)
    Xh = X[:n_host].cpu().numpy()
    Xh = (Xh - Xh.mean(0)) / Xh.std(0)
    t0 = time.perf_counter()
    ica = FastICA(n_components=C, random_state=2001, whiten="unit-variance", max_iter=1000)
    ica.fit(Xh).transform(Xh)
    row["sklearn_host_rows"] = n_host
    row["sklearn_host_s"] = round(time.perf_counter() - t0, 2)
    row["sklearn_host_n_iter"] = int(ica.n_iter_)
    row["sklearn_host_threads"] = int(os.environ.get("OMP_NUM_THREADS", 0)) or None
print(json.dumps({"embedding_map_bench": row}) if "--json" in sys.argv else row, flush=True)
