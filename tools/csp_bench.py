#!/usr/bin/env python3
"""The fused CSP kernel (range_csp_encode) at the design shape - gridcell, F = 32, one hidden layer of 512, gelu,
skip + LayerNorm, 256 outputs - for 10 000 and 100 000 locations (GPU only).  Per size, medians of HIP-event times
of single launches after a warm-up that also ramps the clock:
  fused      the launch alone;
  composed   the same network from range_posenc_features (float64 'grid' features) + torch.nn.functional in
             float32 on the same GPU (cast, linear, gelu, layer_norm, linear, gelu);
  features   the fused kernel on a network of ONE output column behind the same features: its float64 sincos
             phase with next to no matrix work - an estimate of that phase's share of the fused time;
and the fused kernel's share of the float32 MFMA rate: 2 B sum(in * out) FLOP against 157.3 TFLOP/s.
The fused result is checked against the composition (float32 agreement) before anything is timed.
Usage: python tools/csp_bench.py [repeats] [--json]"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
import torch.nn.functional as F

from range_amd import _native, csp, posenc
from tools import synth

args = [v for v in sys.argv[1:] if v.isdigit()]
REPEATS = int(args[0]) if args else 50
PEAK_F32_MFMA = 157.3e12
dev = torch.device("cuda:0")
SETTINGS = dict(spa_enc_type="gridcell", F=32, hidden=512, layers=1, act="gelu", use_layn=True, skip=True, num_filts=256,
                min_radius=0.1, max_radius=360.0, seed=201)


def median_us(fn, repeats=REPEATS, warmup=10):
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
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def network(sd, n):
    t = lambda i, k: sd[f"loc_enc.spa_enc.ffn.layers.{i}.{k}"].numpy()   # noqa: E731
    return ([t(i, "linear.weight") for i in range(n)], [t(i, "linear.bias") for i in range(n)],
            [t(i, "layernorm.weight") if i + 1 < n else None for i in range(n)],
            [t(i, "layernorm.bias") if i + 1 < n else None for i in range(n)])


sd = synth.make_csp_checkpoint(**SETTINGS)["state_dict"]
ws, bs, gs, bes = network(sd, 2)
freq = csp.cal_freq_list("geometric", 32, 360.0, 0.1)
eng = _native.HipEngine(dev)
eng.set_csp(posenc.KIND_GRID, freq, [512, 256], ws, bs, gs, bes, csp.ACTIVATIONS["gelu"], True, True)
feat_eng = _native.HipEngine(dev)       # the same features, one output column
feat_eng.set_csp(posenc.KIND_GRID, freq, [1], [ws[0][:1]], [bs[0][:1]], [None], [None], csp.ACTIVATIONS["gelu"], False, False)
pos_eng = _native.HipEngine(dev)
tw, tb = [torch.from_numpy(a).to(dev) for a in ws], [torch.from_numpy(a).to(dev) for a in bs]
tg, tbe = torch.from_numpy(gs[0]).to(dev), torch.from_numpy(bes[0]).to(dev)


def composed(x):
    f = pos_eng.posenc_features(x, posenc.KIND_GRID, freq).float()
    h = F.layer_norm(F.gelu(F.linear(f, tw[0], tb[0])), (512,), tg, tbe)       # (128 != 512: no skip in this layer)
    return F.gelu(F.linear(h, tw[1], tb[1]))


flop_per_row = 2 * (128 * 512 + 512 * 256)
rows = []
for B in (10_000, 100_000):
    x = torch.from_numpy(synth.make_queries(B, seed=7, lat_max=90.0)).to(dev)
    out = torch.empty((B, 256), dtype=torch.float32, device=dev)
    one = torch.empty((B, 1), dtype=torch.float32, device=dev)
    diff = float((eng.csp_encode(x, out=out) - composed(x)).abs().max())
    assert diff < 1e-4, diff
    fused, fmin, fmax = median_us(lambda: eng.csp_encode(x, out=out))
    comp, cmin, cmax = median_us(lambda: composed(x))
    feat, _, _ = median_us(lambda: feat_eng.csp_encode(x, out=one))
    row = {"locations": B, "fused_us": round(fused, 1), "fused_min_max_us": [round(fmin, 1), round(fmax, 1)],
           "composed_us": round(comp, 1), "composed_min_max_us": [round(cmin, 1), round(cmax, 1)],
           "composed_over_fused": round(comp / fused, 2), "features_only_us": round(feat, 1),
           "features_share_of_fused": round(feat / fused, 3),
           "fused_TFLOPs": round(B * flop_per_row / fused / 1e6, 2),
           "share_of_f32_mfma_peak": round(B * flop_per_row / (fused * 1e-6) / PEAK_F32_MFMA, 4),
           "max_abs_fused_minus_composed": diff}
    rows.append(row)
    if "--json" not in sys.argv:
        print(row, flush=True)
if "--json" in sys.argv:
    print(json.dumps({"csp_bench": rows}))
