#!/usr/bin/env python3
"""One checkerboard task end to end on the GPU, the reference's workflow from a bare checkout:
get_dataset('checker_<num_support>') -> load_model(name) -> save_embeddings -> evaluate_npz.  Prints the
validation accuracy (train: the seed-0 draw of 10 000 samples; validation: the 10 000-point lattice), the
support's nearest-neighbour distance, and the wall time of each stage (host clock; every stage ends synchronised).
Models that need files take them as load_model does (--pretrained-path, --db-path).
Usage: python tools/checker_task.py [--num-support 200] [--model s2vec_grid] [--batch-size 2048] [--device cuda:0]
                                   [--embeddings-dir DIR] [--json]"""
import argparse
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch

from range_amd import evaluate_npz, get_dataset, load_model, save_embeddings

ap = argparse.ArgumentParser()
ap.add_argument("--num-support", type=int, default=200)
ap.add_argument("--model", default="s2vec_grid")
ap.add_argument("--pretrained-path", default="unused")
ap.add_argument("--db-path", default=None)
ap.add_argument("--batch-size", type=int, default=2048)
ap.add_argument("--device", default="cuda:0")
ap.add_argument("--embeddings-dir", default=None)
ap.add_argument("--json", action="store_true")
a = ap.parse_args()

args = argparse.Namespace(task_name=f"checker_{a.num_support}", batch_size=a.batch_size, num_workers=0, device=a.device,
                          location_model_name=a.model, embeddings_dir=a.embeddings_dir or tempfile.mkdtemp(prefix="checker_task_"))
stages = {}


def stage(name, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    stages[name] = round(time.perf_counter() - t0, 4)
    return out


train, val, num_classes = stage("get_dataset_s", lambda: get_dataset(args))
kw = {"db_path": a.db_path} if a.db_path else {}
model = stage("load_model_s", lambda: load_model(a.model, pretrained_path=a.pretrained_path, device=a.device, **kw))
stage("save_embeddings_s", lambda: save_embeddings(args, train, val, model))
accuracy = stage("evaluate_npz_s", lambda: evaluate_npz(args))
row = {"task": args.task_name, "model": a.model, "num_classes": num_classes, "train": len(train.dataset),
       "val": len(val.dataset), "accuracy": float(accuracy), **stages, "embeddings_dir": args.embeddings_dir}
print(json.dumps({"checker_task": row}) if a.json else row)
