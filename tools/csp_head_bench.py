#!/usr/bin/env python3
"""The CSP class head (range_csp_head / range_csp_predict) at the iNat-2018 shape - the design network of
tools/csp_bench.py, num_filts 256, behind it class_emb of 8142 classes (GPU only).  Three workloads:
  probs      10 000 locations x 8142 classes, PROBS                     (the geo prior of a test set)
  one_class  2 000 000 locations x 1 class, PROBS with one class id      (a 1002 x 2004 range map)
  sum        100 000 locations, SUM over the 8142 classes                (dense_prediction_sum)
Per workload, medians of HIP-event times after a warm-up that also ramps the clock:
  predict    range_csp_predict: encoder and head, what the model calls;
  head       range_csp_head alone on embeddings already in memory;
  encode     range_csp_encode alone;
  torch      yardstick 1, what a user does without the head kernel: range_csp_encode, then
             torch.sigmoid(emb @ W.T) (one_class: emb @ W[c]; sum: .sum(1)) in float32 on the same GPU;
  floor      yardstick 2: the larger of the result's bytes at the HBM rate (8.0 TB/s spec) and the head's
             2 B num_filts M FLOP at the float32 MFMA peak (157.3 TFLOP/s) - which of the two is named.
The kernel's result is checked against torch's (float32 agreement) before anything is timed.
Usage: python tools/csp_head_bench.py [repeats] [--json]"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from range_amd import _native, csp, posenc
from tools import synth

args = [v for v in sys.argv[1:] if v.isdigit()]
REPEATS = int(args[0]) if args else 20
PEAK_F32_MFMA, PEAK_HBM = 157.3e12, 8.0e12
dev = torch.device("cuda:0")
C, K, ONE = 8142, 256, 4071
SETTINGS = dict(spa_enc_type="gridcell", F=32, hidden=512, layers=1, act="gelu", use_layn=True, skip=True, num_filts=K,
                min_radius=0.1, max_radius=360.0, seed=201, num_classes=C, class_scale=0.25)
PROBS, SUM = _native.CSP_HEAD_PROBS, _native.CSP_HEAD_SUM


def median_us(fn, repeats=REPEATS, warmup=5):
    for _ in range(warmup):
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
    return round(float(np.median(times)), 1), [round(float(np.min(times)), 1), round(float(np.max(times)), 1)]


sd = synth.make_csp_checkpoint(**SETTINGS)["state_dict"]
t = lambda i, k: sd[f"loc_enc.spa_enc.ffn.layers.{i}.{k}"].numpy()   # noqa: E731
eng = _native.HipEngine(dev)
eng.set_csp(posenc.KIND_GRID, csp.cal_freq_list("geometric", 32, 360.0, 0.1), [512, K],
            [t(0, "linear.weight"), t(1, "linear.weight")], [t(0, "linear.bias"), t(1, "linear.bias")],
            [t(0, "layernorm.weight"), None], [t(0, "layernorm.bias"), None], csp.ACTIVATIONS["gelu"], True, True)
W = sd["loc_enc.class_emb.weight"]
eng.set_csp_head(W.numpy())
Wd = W.to(dev)
Wt, w_one = Wd.t().contiguous(), Wd[ONE].contiguous()
one_id = torch.tensor([ONE], dtype=torch.int32, device=dev)

WORKLOADS = {
    "probs": (10_000, C, PROBS, None, lambda e: torch.sigmoid(e @ Wt)),
    "one_class": (2_000_000, 1, PROBS, one_id, lambda e: torch.sigmoid(e @ w_one).unsqueeze(1)),
    "sum": (100_000, C, SUM, None, lambda e: torch.sigmoid(e @ Wt).sum(1)),
}
rows = []
for name, (B, M, mode, ids, torch_head) in WORKLOADS.items():
    x = torch.from_numpy(synth.make_queries(B, seed=7, lat_max=90.0)).to(dev)
    emb = eng.csp_encode(x)
    got, want = eng.csp_predict(x, ids, mode), torch_head(emb)
    diff = float((got - want).abs().max())
    assert got.shape == want.shape and diff < (1e-2 if mode == SUM else 1e-5), (name, diff)
    assert torch.equal(got, eng.csp_head(emb, ids, mode))
    del got, want
    out_bytes = 4 * B * (1 if mode == SUM else M)
    flop = 2.0 * B * K * M
    t_bytes, t_flop = out_bytes / PEAK_HBM * 1e6, flop / PEAK_F32_MFMA * 1e6
    predict, predict_mm = median_us(lambda: eng.csp_predict(x, ids, mode))
    head, head_mm = median_us(lambda: eng.csp_head(emb, ids, mode))
    encode, _ = median_us(lambda: eng.csp_encode(x))
    torch_us, torch_mm = median_us(lambda: torch_head(eng.csp_encode(x)))
    torch_head_us, _ = median_us(lambda: torch_head(emb))
    floor = max(t_bytes, t_flop)
    row = {"workload": name, "locations": B, "classes": M, "predict_us": predict, "predict_min_max_us": predict_mm,
           "head_us": head, "head_min_max_us": head_mm, "encode_us": encode,
           "torch_encode_plus_head_us": torch_us, "torch_min_max_us": torch_mm, "torch_head_only_us": torch_head_us,
           "torch_over_predict": round(torch_us / predict, 2), "torch_head_over_head": round(torch_head_us / head, 2),
           "floor_us": round(floor, 1), "floor_is": "output bytes at 8.0 TB/s" if t_bytes >= t_flop else "FLOP at 157.3 TFLOP/s",
           "head_over_floor": round(head / floor, 2), "head_TFLOPs": round(flop / head / 1e6, 2),
           "head_out_TBs": round(out_bytes / head / 1e6, 3), "max_abs_kernel_minus_torch": diff}
    rows.append(row)
    if "--json" not in sys.argv:
        print(row, flush=True)
    del x, emb
    torch.cuda.empty_cache()
if "--json" in sys.argv:
    print(json.dumps({"csp_head_bench": rows}))
