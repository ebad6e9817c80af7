#!/usr/bin/env python3
"""Step and epoch times of the CSP encoder fit (range_amd/csp_fit.py, csrc/cspfit_kernels.h) at the design shape:
'gridcell', F = 32, one hidden layer of 512 (a live skip needs 4 F = 128: this one is dead), 256 filters, gelu,
LayerNorm, C = 8142 classes, B = Bg = 1024, N = 436 000 training locations (GPU only).  Recorded, with no pass mark:

  step_us / grad_us / loss_us   one range_cspfit_step / _grad / _loss: HIP events around `repeats` calls back to back,
                                per call; the median and the spread (min, max) over `rounds` such measurements taken
                                after a warm-up round (clocks up);
  three_hidden                  the same with three hidden layers of 512 (two live skips);
  step_gflop                    the head's 17.1 GFLOP plus dE = G W_c (a third product of that size: 8.5 GFLOP) and the
                                layers' 3 x 2 R (in0 x 512 + 512 x 256) FLOP;
  epoch_s, epoch_steps          one epoch of fit_location_model with the balanced sampler (host clock, sampler and
                                the negatives' draw included);
  headfit_step_us               reference point: the frozen-encoder head step (range_headfit_step) on the same machine in
                                the same process, at the same C, F = 256 and rows;
  torch_host_step_s             reference point: the same step restated in torch (float32 autograd + torch.optim.Adam)
                                on the host with the threads the process is given.

Usage: python tools/csp_fit_bench.py [--out profiles/csp_fit_bench.json] [--repeats 20] [--rounds 5] [--no-host] [--no-epoch]"""
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

from range_amd import _cspfit_native as cn
from range_amd import _headfit_native as hn
from range_amd import csp, csp_fit, load_model
from tools import synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "csp_fit_bench.json"))
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--no-epoch", action="store_true")
args = ap.parse_args()

N, C, NF, B, HID, F = 436_000, 8142, 256, 1024, 512, 32
dev = torch.device("cuda:0")
rng = np.random.default_rng(1)
locs_host = np.stack([rng.uniform(-180, 180, N), rng.uniform(-90, 90, N)], axis=1)
labels_host = rng.integers(0, C, N)
locs = torch.from_numpy(locs_host).to(dev)
rows = torch.from_numpy(rng.integers(0, N, B).astype(np.int32)).to(dev)
lab = torch.from_numpy(labels_host.astype(np.int32)).to(dev)[rows.long()].contiguous()
bg = torch.from_numpy(np.stack([rng.uniform(-180, 180, B), rng.uniform(-90, 90, B)], axis=1)).to(dev)
out = {"N": N, "C": C, "num_filts": NF, "hidden": HID, "F": F, "B": B, "Bg": B, "repeats": args.repeats, "rounds": args.rounds}


def timed(fn):
    """Median and spread, over `rounds`, of the time per call of `repeats` calls back to back; one warm-up round."""
    vals = []
    for r in range(args.rounds + 1):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.repeats):
            fn()
        b.record()
        b.synchronize()
        if r:
            vals.append(a.elapsed_time(b) * 1e3 / args.repeats)
    return {"median": round(float(np.median(vals)), 1), "min": round(min(vals), 1), "max": round(max(vals), 1)}


def network(tmp, layers):
    ck = synth.write_csp_checkpoint(os.path.join(tmp, f"csp{layers}.pth.tar"), spa_enc_type="gridcell", F=F, hidden=HID, layers=layers,
                                    act="gelu", use_layn=True, skip=True, num_filts=NF, num_classes=C, class_scale=0.05, dropout=0.0)
    return ck, csp.read_csp_checkpoint(ck, class_head=True)


with tempfile.TemporaryDirectory() as tmp:
    for layers, key in ((1, "design"), (3, "three_hidden")):
        ck, p = network(tmp, layers)
        fit = cn.CspFit(dev)
        fit.begin(p, C, p.class_emb)
        row = {"plan": cn.plan(p.kind, F, p.widths, True, True, C, 2 * B), "params": fit.param_count}
        row["step_us"] = timed(lambda: fit.step(locs, rows, lab, bg, 1e-3))
        row["grad_us"] = timed(lambda: fit.grad(locs, rows, lab, bg))
        row["loss_us"] = timed(lambda: fit.loss(locs, rows, lab, bg))
        R = 2 * B
        layer_flop = sum(2.0 * R * w.shape[0] * w.shape[1] for w in p.weights) * 3
        row["step_gflop"] = round((3 * 2.0 * R * C * NF + layer_flop) / 1e9, 2)
        row["step_tflops"] = round(row["step_gflop"] * 1e3 / row["step_us"]["median"], 2)
        fit.engine.close()
        out[key] = row
        if layers == 1 and not args.no_epoch:
            model = load_model("CSP", pretrained_path=ck, device="cuda:0", class_head=True)
            t0 = time.perf_counter()
            res = csp_fit.fit_location_model(model, locs_host, labels_host, C, epochs=1, batch_size=B, dropout=0.0)
            torch.cuda.synchronize()
            out["epoch_s"] = round(time.perf_counter() - t0, 3)
            out["epoch_steps"] = res.steps
            out["epoch_train_loss"] = round(res.train_losses[0], 5)
        if layers == 1:
            host_p = p

# reference point 1: the head-only step on frozen embeddings, same rows and classes
feats = torch.randn((4 * B, NF), device=dev, dtype=torch.float32) * 0.5
hf = hn.HeadFit(dev)
hf.begin(C, NF, host_p.class_emb)
hrows = torch.arange(B, dtype=torch.int32, device=dev)
out["headfit_step_us"] = timed(lambda: hf.step(feats, hrows, lab, feats[2 * B:3 * B], 1e-3))
hf.engine.close()

# reference point 2: the restated step in torch on the host
if not args.no_host:
    from range_amd import _native
    eng = _native.HipEngine(dev)
    ll = torch.cat([locs[rows.long()], bg]).contiguous()
    X0 = eng.posenc_features(ll, host_p.kind, host_p.freq_list).float().cpu()       # float64 features rounded once
    eng.close()
    y = lab.long().cpu()
    par = lambda a: torch.nn.Parameter(torch.from_numpy(np.array(a)))              # noqa: E731
    Ws, bs = [par(w) for w in host_p.weights], [par(b) for b in host_p.biases]
    g0, be0, Wc = par(host_p.ln_gamma[0]), par(host_p.ln_beta[0]), par(host_p.class_emb)
    opt = torch.optim.Adam(Ws + bs + [g0, be0, Wc], lr=1e-3)
    inds = torch.arange(B)

    def host_step():
        opt.zero_grad()
        h = torch.nn.functional.gelu(X0 @ Ws[0].t() + bs[0])
        h = torch.nn.functional.layer_norm(h, (HID,), g0, be0, 1e-5)
        e = torch.nn.functional.gelu(h @ Ws[1].t() + bs[1])
        pr = torch.sigmoid(e @ Wc.t())
        lp = -torch.log(1.0 - pr[:B] + 1e-5)
        lp[inds, y] = C * -torch.log(pr[:B][inds, y] + 1e-5)
        loss = lp.mean() + (-torch.log(1.0 - pr[B:] + 1e-5)).mean()
        loss.backward()
        opt.step()
    host_step()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        host_step()
        ts.append(time.perf_counter() - t0)
    out["torch_host_step_s"] = round(float(np.median(ts)), 3)
    out["torch_host_threads"] = torch.get_num_threads()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump({"csp_fit_bench": out}, f, indent=1)
    f.write("\n")
print(json.dumps({"csp_fit_bench": out}), flush=True)
