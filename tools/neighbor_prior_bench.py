#!/usr/bin/env python3
"""The neighbour and grid geo priors (range_amd/geo_baselines.py, csrc/neighbor_kernel.h) at a synthetic
iNat-2018-like shape: 436 000 training points clustered on land-like blobs, 24 000 queries, 8142 classes, the
reference's ``inat_2018`` hyper-parameters (euclidean degrees, dist_thresh 2.0, 1500 neighbours, a 180 x 60 grid,
pseudo_count 2) - and the same points with the haversine metric, whose pair term is the checkerboard scan's (GPU only).

Per stage, after a warm-up call, the median of HIP-event times of single calls with float32 image predictions, and
pairs/s = queries x training points over the time (the selection scans the set once per digit pass and once more for
the last tie: its pairs/s counts one scan's pairs over the whole time, its ``scans`` says how many it makes):
  install        range_set_neighbors (host time: upload, packing kernel, synchronisation)
  nn_dist_rank   vote scan + ranks, radius predicate
  knn_select     the k-th neighbour selection alone
  nn_knn_rank    selection + vote scan + ranks
  grid_rank      vote scan + ranks, cell predicate (one integer compare a pair)
Next to it scikit-learn's BallTree on the same machine's host: the reference's loop (one query_radius / query per
sample, a dense prior and an argsort over the classes) on ``--host-queries`` of the queries, and its time scaled to
all of them.  Prints one JSON line.
Usage: python tools/neighbor_prior_bench.py [repeats] [--train N] [--queries B] [--classes C] [--host-queries n] [--no-host]"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from range_amd import _neighbors_native as nn
from range_amd import geo_baselines as gb
from prior_bench_common import blobs, timed


def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 5
N, B, C = opt("--train", 436_000), opt("--queries", 24_000), opt("--classes", 8142)
HOST_Q = opt("--host-queries", 48)
HP = gb.get_cross_val_hyper_params("inat_2018")
HP["num_neighbors"] = min(HP["num_neighbors"], N)
DEV = torch.device("cuda:0")


def stage(name, seconds, scans=1, **more):
    return dict(stage=name, seconds=round(seconds, 5), scans=scans, pairs_per_s=float(f"{B * N / seconds:.4g}"), **more)


train, train_cls, centres = blobs(N, 1, C)
query, _, _ = blobs(B, 2, C, centres)
labels = torch.from_numpy(np.random.default_rng(3).integers(0, C, B).astype(np.int32)).to(DEV)
img = torch.rand((B, C), dtype=torch.float32, device=DEV)
out = {"train": N, "queries": B, "classes": C, "pairs": B * N, "hyper_params": HP, "repeats": REPEATS, "plan": nn.plan(B, N, C, HP["num_neighbors"])}
for metric in ("euclidean", "haversine"):
    hav = metric == "haversine"
    # the haversine run keeps the radius in degrees of arc: 2 degrees as radians
    hp = dict(HP, dist_type=metric, dist_thresh=float(np.deg2rad(HP["dist_thresh"])) if hav else HP["dist_thresh"])
    t0 = time.perf_counter()
    prior = gb.NeighborPrior(train, train_cls, C, hp, device=DEV)
    install = time.perf_counter() - t0
    eng, k = prior.engine, hp["num_neighbors"]
    q = prior._q(query)
    thr = gb.radius_threshold(hp["dist_thresh"], hav)
    rows = [dict(stage="install", seconds=round(install, 4))]
    rows.append(stage("nn_dist_rank", timed(lambda: eng.neighbor_rank(q, None, nn.RADIUS, labels, img, thr=thr), REPEATS)))
    rows.append(stage("knn_select", timed(lambda: eng.neighbor_select(q, k), max(1, REPEATS // 2)), scans=nn.plan(B, N, C, k)["passes"] + 1))
    rows.append(stage("nn_knn_rank", timed(lambda: eng.neighbor_rank(q, None, nn.KNN, labels, img, k=k), max(1, REPEATS // 2)),
                      scans=nn.plan(B, N, C, k)["passes"] + 2))
    _, counts = eng.neighbor_prior(q[:256], None, nn.RADIUS, thr=thr, want_counts=True)
    out[metric] = {"stages": rows, "mean_radius_members_first_256": float(counts.sum(1).double().mean())}
    if not hav:
        grid = gb.GridPrior(train, train_cls, C, hp, device=DEV)
        qc = grid._qcell(query)
        rows.append(stage("grid_rank", timed(lambda: grid.engine.neighbor_rank(None, qc, nn.CELL, labels, img, pc=grid._pc, cpc=grid._cpc), REPEATS)))
    if "--no-host" not in sys.argv:
        from sklearn.neighbors import BallTree
        t0 = time.perf_counter()
        tree = BallTree(np.deg2rad(train)[:, ::-1], metric="haversine") if hav else BallTree(train[:, ::-1], metric="euclidean")
        build = time.perf_counter() - t0
        qn = np.deg2rad(query[:HOST_Q]) if hav else query[:HOST_Q]
        img_h = img[:HOST_Q].cpu().numpy()
        host = {"queries": HOST_Q, "tree_build_s": round(build, 3)}
        for ptype in ("distance", "knn"):
            t0 = time.perf_counter()
            for i in range(HOST_Q):             # the reference's loop body: neighbours, dense prior, argsort over the classes
                loc = qn[i, ::-1][None]
                inds = tree.query_radius(loc, r=hp["dist_thresh"])[0] if ptype == "distance" else tree.query(loc, k=k)[1][0]
                p = np.ones(C)
                cls_id, cls_cnt = np.unique(train_cls[inds], return_counts=True)
                p[cls_id] += cls_cnt
                p /= p.sum()
                np.argsort(img_h[i] * p)
            dt = time.perf_counter() - t0
            gpu = next(r for r in rows if r["stage"] == ("nn_dist_rank" if ptype == "distance" else "nn_knn_rank"))["seconds"]
            host[ptype] = {"seconds": round(dt, 4), "scaled_to_all_queries_s": round(dt * B / HOST_Q, 2),
                           "scaled_over_gpu": round(dt * B / HOST_Q / gpu, 1)}
        out[metric]["host_balltree_loop"] = host
    prior.engine.close()
print(json.dumps({"neighbor_prior_bench": out}))
