#!/usr/bin/env python3
"""Temperature sweeps from one scan, timed on the bench workload (10 000 queries x range_db_large,
synthetic): (a) ``stats_kept`` - the softmax statistics at 1 / 4 / 8 temperature pairs from the kept
logits, with and without a geographic head - against ``scan_stats(keep_logits=True)`` of the same shape,
and the bytes of kept logits per second it reads; (b) a 3 x 3 x 5 grid through
``sweep(coords, betas, temps=, geo_temps=)`` against the same grid as nine ``sweep(coords, betas)`` calls
with ``args.temp`` / ``args.geo_temp`` set per call.  DESIGN.md section 5's protocol: >= 40 ms of warm-up
(the clock ramp), medians of >= 20, both sides of a comparison in the same process and alternating.
Usage: temp_sweep.py [queries] [repeats]."""
import os, sys, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from range_amd import _native, load_model
from tools import synth

B = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000
REPS = max(20, int(sys.argv[2])) if len(sys.argv) > 2 else 20
DEV = "cuda:0"
tmp = os.environ.get("TMPDIR", "/tmp")
ck = synth.write_checkpoint(os.path.join(tmp, "tsweep.ckpt"), L=40, hidden=512, seed=1234)
N = synth.BANK_ROWS["range_db_large"]
locs, vals, keys = synth.make_bank(N, 2024)
db = os.path.join(tmp, "tsweep_db.npz")
np.savez(db, locs=locs, image_embeddings=vals, satclip_embeddings=keys)
m = load_model("RANGE+", pretrained_path=ck, device=DEV, db_path=db, beta=0.5)
eng = m.engine
x = torch.from_numpy(synth.make_queries(B, seed=7)).to(DEV)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def medians(fns, reps):
    """Median ms of every callable of ``fns`` (name -> fn), called in turns ``reps`` times."""
    pairs = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            pairs[k].append(timed(fn))
    torch.cuda.synchronize()
    return {k: float(np.median([a.elapsed_time(b) for a, b in v])) for k, v in pairs.items()}


# ---- (a) the kernel --------------------------------------------------------------------------------
e64, e32, xq = eng.encode(x)
scan = lambda: eng.scan_stats(e32, xq, 12.0, 40.0, keep_logits=True)     # noqa: E731
for _ in range(12):               # > 40 ms of continuous work
    scan()
assert eng.kept_queries() == B
geo_pairs = [(12.0 + 4 * i, 40.0 + 5 * i) for i in range(8)]             # (one of them above 43: 40 .. 75)
sem_pairs = [(12.0 + 4 * i, 0.0) for i in range(8)]
fns = {"scan_stats_keep": scan}
for n in (1, 4, 8):
    fns[f"stats_kept_{n}_geo"] = lambda n=n: eng.stats_kept(0, xq, geo_pairs[:n])
    fns[f"stats_kept_{n}_nogeo"] = lambda n=n: eng.stats_kept(0, xq, sem_pairs[:n])
fns["stats_kept_8_sharp_geo"] = lambda: eng.stats_kept(0, xq, [(50.0 + 10 * i, 100.0 + 10 * i) for i in range(8)])
ms = medians(fns, REPS)
# the kernel alone (event pairs around the launch, without the merges behind it)
eng.profile_enable(True)
for _ in range(REPS):
    eng.stats_kept(0, xq, geo_pairs[:1])
k_ms, k_n = eng.profile_read(_native.PROF_KEPT_STATS)
eng.profile_enable(False)
n_blocks, n_qtiles = (N + 15) // 16, (B + 63) // 64
kept_bytes = n_qtiles * n_blocks * 4096
res_a = {"queries": B, "bank_rows": N, "repeats": REPS, "kept_logit_bytes": kept_bytes, "median_ms": ms,
         "kernel_only_1_geo_mean_ms": k_ms / max(k_n, 1),
         "TB_per_s": {k: kept_bytes / (v * 1e-3) / 1e12 for k, v in ms.items() if k.startswith("stats_kept")},
         "one_pair_over_scan": ms["stats_kept_1_geo"] / ms["scan_stats_keep"]}
print(json.dumps({"kernel": res_a}))
sys.stdout.flush()

# ---- (b) the whole sweep ---------------------------------------------------------------------------
temps, geo_temps, betas = (12.0, 25.0, 100.0), (20.0, 40.0, 200.0), (0.0, 0.25, 0.5, 0.75, 1.0)


def new_sweep():
    return m.sweep(x, betas, return_device=True, temps=temps, geo_temps=geo_temps)


def nine_sweeps():
    out = []
    for ts in temps:
        for tg in geo_temps:
            m.args.temp, m.args.geo_temp = ts, tg
            out.append(m.sweep(x, betas, return_device=True))
    m.args.temp, m.args.geo_temp = 12.0, 40.0
    return out


got, want = new_sweep(), nine_sweeps()
same, worst = [], 0.0
for i, ts in enumerate(temps):
    for j, tg in enumerate(geo_temps):
        w = want[i * len(geo_temps) + j]
        same.append(bool(torch.equal(got[i, j], w)) if (ts > 43.0) == (tg > 43.0) else None)
        worst = max(worst, float((got[i, j] - w).abs().max()))
del got, want
ms_b = medians({"temperature_sweep": new_sweep, "nine_beta_sweeps": nine_sweeps}, REPS)
print(json.dumps({"sweep": {"grid": [len(temps), len(geo_temps), len(betas)], "queries": B, "median_ms": ms_b,
                            "ratio": ms_b["nine_beta_sweeps"] / ms_b["temperature_sweep"],
                            "bitwise_equal_same_side_of_43": same, "max_abs_difference": worst}}))
