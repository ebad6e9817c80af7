#!/usr/bin/env python3
"""The KDE geo prior (range_amd/geo_baselines.py: KdePrior, csrc/kde_kernel.h) at the synthetic iNat-2018-like shape of
tools/neighbor_prior_bench.py: 436 000 training points on 40 blobs, 24 000 queries, 8142 classes, float32 image
predictions, euclidean degrees, with the reference's two kinds of KDE settings:
  inat_2018   kde_quant 5.0,   kde_nb 700   (few bins, every bin heavy)
  birdsnap    kde_quant 0.001, kde_nb 500   (M about N: every training point its own bin)

Per stage (GPU stages: after a warm-up call, the median of HIP-event times of single calls; host stages: wall time):
  binning        create_kde_grid on the host
  install        range_set_kde_points (upload, packing kernel, synchronisation)
  selection      the kde_nb-th bin's distance (neighbor_select_kernel: a scan per digit pass and one for the last tie)
  host_params    red_k to the host, h / thr / two_h2 in numpy scalars, back to the device
  scan_rank      kde_vote_kernel (+ fold) with the three rank integers
Beside the birdsnap setting the nn_dist scan (range_neighbor_rank, radius predicate, the inat_2018 dist_thresh) of the
SAME run at the same (B, N, C), and the ratio of the two scans.  Next to each setting the reference's loop body on
this machine's host (two BallTree queries, the weights, the per-class sums, the normalisation, an argsort over the
classes) on ``--host-queries`` of the queries, scaled to all of them.  Prints one JSON line.
Usage: python tools/kde_prior_bench.py [repeats] [--train N] [--queries B] [--classes C] [--host-queries n] [--no-host]"""
import json
import math
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from range_amd import _neighbors_native as nn
from range_amd import geo_baselines as gb
from prior_bench_common import blobs, timed, wall


def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 5
N, B, C = opt("--train", 436_000), opt("--queries", 24_000), opt("--classes", 8142)
HOST_Q = opt("--host-queries", 48)
SETTINGS = {"inat_2018": gb.get_cross_val_hyper_params("inat_2018"), "birdsnap": gb.get_cross_val_hyper_params("birdsnap", "ebird_meta")}
DEV = torch.device("cuda:0")


train, train_cls, centres = blobs(N, 1, C)
query, _, _ = blobs(B, 2, C, centres)
labels_h = np.random.default_rng(3).integers(0, C, B)
labels = torch.from_numpy(labels_h.astype(np.int32)).to(DEV)
img = torch.rand((B, C), dtype=torch.float32, device=DEV)
out = {"train": N, "queries": B, "classes": C, "repeats": REPEATS}

# the nn_dist scan of this run, for the ratio
hp_nn = dict(SETTINGS["inat_2018"])
nbr = gb.NeighborPrior(train, train_cls, C, hp_nn, device=DEV)
qn = nbr._q(query)
thr_nn = gb.radius_threshold(hp_nn["dist_thresh"], False)
nn_dist = timed(lambda: nbr.engine.neighbor_rank(qn, None, nn.RADIUS, labels, img, thr=thr_nn), REPEATS)
out["nn_dist_rank_s"] = round(nn_dist, 5)
out["nn_dist_plan"] = nn.plan(B, N, C)
nbr.engine.close()

for name, hp in SETTINGS.items():
    hp = dict(hp)
    (bcls, blocs, counts), t_bin = wall(lambda: gb.create_kde_grid(train_cls, train, hp))
    M = len(counts)
    hp["kde_nb"] = min(hp["kde_nb"], M)
    prior = gb.KdePrior(train, train_cls, C, hp, device=DEV)
    eng = prior.engine
    _, t_install = wall(lambda: eng.set_kde_points(blocs, bcls, counts, C, False))
    qd = torch.from_numpy(np.ascontiguousarray(query)).to(DEV)
    t_select = timed(lambda: eng.neighbor_select(qd, hp["kde_nb"]), max(1, REPEATS // 2))
    (qd, thr, two_h2, h), t_params = wall(lambda: prior._scan_inputs(query))
    t_params -= t_select
    t_scan = timed(lambda: eng.kde_rank(qd, thr, two_h2, labels, img), REPEATS)
    _, sums = eng.kde_prior(qd[:256], thr[:256], two_h2[:256], want_sums=True)
    plan = nn.kde_plan(B, M, C, int(counts.sum()))
    res = {"hyper_params": {k: hp[k] for k in ("kde_quant", "kde_nb", "kde_dist_type")}, "bins": M, "plan": plan,
           "mean_member_classes_first_256": float((sums > 0).sum(1).double().mean()),
           "stages": [dict(stage="binning", seconds=round(t_bin, 4)), dict(stage="install", seconds=round(t_install, 4)),
                      dict(stage="selection", seconds=round(t_select, 5), scans=nn.plan(B, M, C, hp["kde_nb"])["passes"] + 1),
                      dict(stage="host_params", seconds=round(max(t_params, 0.0), 4)),
                      dict(stage="scan_rank", seconds=round(t_scan, 5), pairs_per_s=float(f"{B * M / t_scan:.4g}"))]}
    if name == "birdsnap":
        res["scan_rank_over_nn_dist_rank"] = round(t_scan / nn_dist, 2)
    if "--no-host" not in sys.argv:
        from sklearn.neighbors import BallTree
        (tree, t_tree) = wall(lambda: BallTree(blocs[:, ::-1], metric="euclidean"))
        img_h = img[:HOST_Q].cpu().numpy()
        t0 = time.perf_counter()
        for i in range(HOST_Q):                 # the reference's loop body per sample
            at = query[i, ::-1][None]
            bw = 0.5 * np.max(tree.query(at, k=hp["kde_nb"])[0])
            inds = tree.query_radius(at, r=2 * bw + 1e-9)[0]
            d2 = ((blocs[inds, ::-1] - query[i, ::-1]) ** 2).sum(1)
            dens = (2 * math.pi * bw) ** -1.0 * np.exp(-d2 / (2 * bw ** 2))
            den = np.dot(counts[inds], dens)
            num = np.zeros(C)
            per_class = np.bincount(bcls[inds], counts[inds] * dens)
            num[:len(per_class)] = per_class
            num = num + np.min(num[np.nonzero(num)])
            p = num / den
            p = p / p.sum()
            np.argsort(img_h[i] * p)
        dt = time.perf_counter() - t0
        gpu = t_select + max(t_params, 0.0) + t_scan
        res["host_balltree_loop"] = {"queries": HOST_Q, "tree_build_s": round(t_tree, 3), "seconds": round(dt, 4),
                                     "scaled_to_all_queries_s": round(dt * B / HOST_Q, 2),
                                     "gpu_per_batch_s": round(gpu, 5), "scaled_over_gpu": round(dt * B / HOST_Q / gpu, 1)}
    out[name] = res
    eng.close()
print(json.dumps({"kde_prior_bench": out}))
