#!/usr/bin/env python3
"""The CSP evaluation kernel (range_csp_rank) at the iNat-2018 shape - num_filts 256, class_emb of 8142 classes,
float32 image predictions (GPU only).  Three batches: 24 426 rows (iNat-2018 val), 10 000 and 64.
Per batch, medians of HIP-event times after a warm-up that also ramps the clock:
  rank         range_csp_rank on embeddings and image predictions already in GPU memory: three int32 a row;
  composition  what a user does without it, on the same GPU: range_csp_head PROBS (the (B, 8142) float32 matrix),
               then torch ``s = p.double() * img``, the two comparisons with the label's score (greater, tied after
               the label) and an argmax;
  head         range_csp_head PROBS alone (the composition's first step);
  floor        the larger of the image predictions' bytes at the HBM rate (8.0 TB/s spec) and the head's
               2 B num_filts C FLOP at the float32 MFMA peak (157.3 TFLOP/s) - which of the two is named.
The kernel's three outputs are checked against the composition's (equal, bit for bit) before anything is timed.
Usage: python tools/csp_rank_bench.py [repeats] [--json]"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from range_amd import _native
from range_amd import posenc

args = [v for v in sys.argv[1:] if v.isdigit()]
REPEATS = int(args[0]) if args else 20
PEAK_F32_MFMA, PEAK_HBM = 157.3e12, 8.0e12
dev = torch.device("cuda:0")
C, K = 8142, 256
PROBS = _native.CSP_HEAD_PROBS


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


rng = np.random.default_rng(31)
eng = _native.HipEngine(dev)
# the head only needs the network's num_filts: the smallest network of that width
eng.set_csp(posenc.KIND_GRID, np.ones(1), [K], [np.zeros((K, 4), dtype=np.float32)], [np.zeros(K, dtype=np.float32)],
            [None], [None], 1, False, False)
eng.set_csp_head((rng.standard_normal((C, K)) * (2.0 / np.sqrt(K))).astype(np.float32))


def composition(emb, img, labels):
    p = eng.csp_head(emb, None, PROBS)
    s = p.double() * img
    st = s.gather(1, labels.long().unsqueeze(1))
    cols = torch.arange(C, device=dev).unsqueeze(0)
    greater = (s > st).sum(1)
    tied = ((s == st) & (cols > labels.unsqueeze(1))).sum(1)
    return greater, tied, s.argmax(1)


rows = []
for B in (24_426, 10_000, 64):
    emb = torch.from_numpy(rng.uniform(-1.0, 1.0, size=(B, K)).astype(np.float32)).to(dev)
    img = torch.softmax(torch.from_numpy(rng.standard_normal((B, C)).astype(np.float32) * 2.0).to(dev), dim=1)
    img[torch.rand((B, C), device=dev) < 0.1] = 0.0
    labels = torch.from_numpy(rng.integers(0, C, size=B).astype(np.int32)).to(dev)
    got, want = eng.csp_rank(emb, labels, img), composition(emb, img, labels)
    for g, w in zip(got, want):
        assert torch.equal(g.long(), w.long()), B
    del got, want
    rank, rank_mm = median_us(lambda: eng.csp_rank(emb, labels, img))
    comp, comp_mm = median_us(lambda: composition(emb, img, labels))
    head, _ = median_us(lambda: eng.csp_head(emb, None, PROBS))
    t_bytes, t_flop = 4.0 * B * C / PEAK_HBM * 1e6, 2.0 * B * K * C / PEAK_F32_MFMA * 1e6
    floor = max(t_bytes, t_flop)
    row = {"rows": B, "classes": C, "rank_us": rank, "rank_min_max_us": rank_mm, "composition_us": comp,
           "composition_min_max_us": comp_mm, "head_probs_us": head, "composition_over_rank": round(comp / rank, 2),
           "rank_over_head_probs": round(rank / head, 2), "floor_us": round(floor, 1),
           "floor_is": "image bytes at 8.0 TB/s" if t_bytes >= t_flop else "FLOP at 157.3 TFLOP/s",
           "rank_over_floor": round(rank / floor, 2), "rank_TFLOPs": round(2.0 * B * K * C / rank / 1e6, 2)}
    rows.append(row)
    if "--json" not in sys.argv:
        print(row, flush=True)
    del emb, img, labels
    torch.cuda.empty_cache()
if "--json" in sys.argv:
    print(json.dumps({"csp_rank_bench": rows}))
