#!/usr/bin/env python3
"""Step and epoch times of the class-head fit (range_amd/head_fit.py, csrc/headfit_kernels.h) at the iNat-2018
shape: N = 436 000 training rows, C = 8142 classes, F = 256 features, B = Bg = 1024 (GPU only).  Synthetic float32
features already in HBM; the background rows of a step are a random slice of them (the encoder's time is not the
fit's).  Recorded, with no pass mark:

  step_us               one range_headfit_step (gather, logit gradient, fold, update with Adam, loss scalars), HIP
                        events around `repeats` steps back to back, per step;
  step_tflops           the 17.1 GFLOP a step performs - TWO products of 2048 x 8142 x 256, the logits and dW; with the
                        encoder frozen there is no gradient with respect to X - over that time (a full backward pass
                        would be a third product, 25.6 GFLOP: recorded as floor_gflop_three_products);
  grad_us / loss_us     range_headfit_grad and range_headfit_loss the same way;
  epoch_s, epoch_steps  one epoch of fit_head_on_features with the balanced sampler (host clock, sampler included);
  head_kernel_us        reference point: the class head's own kernel (range_csp_head, PROBS) on one 2048 x 8142 x 256
                        product - half of a step's products;
  torch_host_step_s     reference point: the same step restated in torch (float32 autograd + torch.optim.Adam) on the
                        host with the threads the process is given.

Usage: python tools/head_fit_bench.py [--out profiles/head_fit_bench.json] [--repeats 20] [--no-host] [--no-epoch]"""
import argparse
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from range_amd import _headfit_native as hn
from range_amd import _native, head_fit, load_model
from tools import synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "head_fit_bench.json"))
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--no-epoch", action="store_true")
args = ap.parse_args()

N, C, F, B = 436_000, 8142, 256, 1024
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(1)
feats = torch.randn((N, F), generator=g, device=dev, dtype=torch.float32) * 0.5
labels_host = np.random.default_rng(2).integers(0, C, N)
labels = torch.from_numpy(labels_host.astype(np.int32)).to(dev)
w0 = (np.random.default_rng(3).standard_normal((C, F)) * 0.05).astype(np.float32)
rows = torch.from_numpy(np.random.default_rng(4).integers(0, N, B).astype(np.int32)).to(dev)
lab = labels[rows.long()].contiguous()
bg = feats[5000:5000 + B].contiguous()
row = {"N": N, "C": C, "F": F, "B": B, "Bg": B, "repeats": args.repeats, "plan": hn.plan(C, F, 2 * B)}


def per_call_us(fn, repeats):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeats):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / repeats


fit = hn.HeadFit(dev)
fit.begin(C, F, w0)
row["step_us"] = round(per_call_us(lambda: fit.step(feats, rows, lab, bg, 1e-3), args.repeats), 1)
row["step_gflop"] = round(2 * 2.0 * 2 * B * C * F / 1e9, 2)
row["floor_gflop_three_products"] = round(3 * 2.0 * 2 * B * C * F / 1e9, 2)
row["step_tflops"] = round(row["step_gflop"] * 1e3 / row["step_us"], 2)
row["grad_us"] = round(per_call_us(lambda: fit.grad(feats, rows, lab, bg), args.repeats), 1)
row["loss_us"] = round(per_call_us(lambda: fit.loss(feats, rows, lab, bg), args.repeats), 1)
fit.engine.close()

if not args.no_epoch:
    def bg_fn(n, spec, rng):
        i = int(rng.integers(0, N - n))
        return feats[i:i + n]
    t0 = time.perf_counter()
    res = head_fit.fit_head_on_features(feats, labels_host, bg_fn, C, epochs=1, batch_size=B, init=w0)
    torch.cuda.synchronize()
    row["epoch_s"] = round(time.perf_counter() - t0, 3)
    row["epoch_steps"] = res.steps
    row["epoch_train_loss"] = round(res.train_losses[0], 5)

# reference point 1: the head kernel's own time for one (2048 x 8142 x 256) product
with tempfile.TemporaryDirectory() as tmp:
    ck = synth.write_csp_checkpoint(os.path.join(tmp, "csp.pth.tar"), num_filts=F, num_classes=C, class_scale=0.05)
    model = load_model("CSP", pretrained_path=ck, device="cuda:0", class_head=True)
    x = feats[:2 * B].contiguous()
    eng = model.loc_model._engine[0]
    row["head_kernel_us"] = round(per_call_us(lambda: eng.csp_head(x, None, _native.CSP_HEAD_PROBS), args.repeats), 1)
    row["head_kernel_tflops"] = round(2.0 * 2 * B * C * F / row["head_kernel_us"] / 1e6, 2)

# reference point 2: the restatement's step in torch on the host
if not args.no_host:
    X, Xbg = feats[rows.long()].cpu(), bg.cpu()
    y = lab.long().cpu()
    W = torch.nn.Parameter(torch.from_numpy(w0.copy()))
    opt = torch.optim.Adam([W], lr=1e-3)
    inds = torch.arange(B)

    def host_step():
        opt.zero_grad()
        p, pr = torch.sigmoid(X @ W.t()), torch.sigmoid(Xbg @ W.t())
        lp = -torch.log(1.0 - p + 1e-5)
        lp[inds, y] = C * -torch.log(p[inds, y] + 1e-5)
        loss = lp.mean() + (-torch.log(1.0 - pr + 1e-5)).mean()
        loss.backward()
        opt.step()
    host_step()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        host_step()
        ts.append(time.perf_counter() - t0)
    row["torch_host_step_s"] = round(float(np.median(ts)), 3)
    row["torch_host_threads"] = torch.get_num_threads()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump({"head_fit_bench": row}, f, indent=1)
    f.write("\n")
print(json.dumps({"head_fit_bench": row}), flush=True)
