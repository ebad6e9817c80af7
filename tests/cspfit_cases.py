"""The cases of tests/golden/cspfit.npz (make_golden_cspfit.py writes it, test_cspfit_cpu.py / test_gpu_cspfit.py read
it): networks of a few thousand parameters with dropout 0 - one per activation, LayerNorm on and off, a live skip
(hidden = 4 F for 'gridcell', 6 F for 'theory') and a dead one, no hidden layer, three hidden layers.  Each entry:
(load_model name, keyword arguments of tools/synth.py: make_csp_checkpoint, hyper-parameters of the six steps)."""
import json

import numpy as np

B, BG, C, N, STEPS = 48, 48, 70, 200, 6
CLASS_SCALE = 0.3
_H = dict(lr=1e-3, weight_decay=0.01, rand_sample_weight=1.0)

CASES = {
    "gelu_ln_skip": ("CSP", dict(spa_enc_type="gridcell", F=4, hidden=16, layers=1, act="gelu", use_layn=True, skip=True,
                                 num_filts=12, min_radius=0.1, max_radius=360.0, seed=901), _H),
    "sigmoid_dead": ("CSP", dict(spa_enc_type="gridcell", F=4, hidden=20, layers=1, act="sigmoid", use_layn=False, skip=True,
                                 num_filts=12, min_radius=0.1, max_radius=360.0, seed=902),
                     dict(lr=2e-3, weight_decay=0.01, rand_sample_weight=0.5)),
    "relu_theory": ("CSP_INat", dict(spa_enc_type="theory", F=3, hidden=18, layers=2, act="relu", use_layn=True, skip=True,
                                     num_filts=10, min_radius=0.1, max_radius=360.0, seed=903), _H),
    "leaky_nohidden": ("CSP", dict(spa_enc_type="gridcell", F=5, hidden=8, layers=0, act="leakyrelu", use_layn=True, skip=True,
                                   num_filts=14, min_radius=0.1, max_radius=360.0, seed=904), _H),
    "tanh_three": ("CSP", dict(spa_enc_type="gridcell", F=4, hidden=16, layers=3, act="tanh", use_layn=True, skip=True,
                               num_filts=12, min_radius=0.1, max_radius=360.0, seed=905), _H),
    "gelu_noln_skip": ("CSP", dict(spa_enc_type="gridcell", F=4, hidden=16, layers=2, act="gelu", use_layn=False, skip=True,
                                   num_filts=12, min_radius=0.1, max_radius=360.0, seed=906), _H),
}


def case_params(golden, case: str):
    """The case's network as ``range_amd.csp.CspParams`` with its class head (regenerated from the numpy seed)."""
    import os
    import tempfile

    from range_amd.csp import read_csp_checkpoint
    from tools import synth
    s = json.loads(str(golden[case + "_settings"]))
    with tempfile.TemporaryDirectory() as tmp:
        path = synth.write_csp_checkpoint(os.path.join(tmp, "c.pth.tar"), device="cpu", **s)
        return read_csp_checkpoint(path, class_head=True)


def step_batch(golden, case: str, i: int):
    """(batch locations (B, 2) float64, labels (B,), background (Bg, 2) float64, row ids (B,)) of step i."""
    rows = golden[f"{case}_s{i}_rows"]
    locs = golden[f"{case}_train_locs"].astype(np.float64)
    return locs[rows], golden[f"{case}_classes"][rows], golden[f"{case}_s{i}_bg"].astype(np.float64), rows


# ---- the model-level compared run: fit_location_model against the float64 restatement of the SAME loop ---------------
# Two epochs of three given batches of 64 rows (and 64 negatives) from init='xavier', with weight decay, a background
# weight, dropout 0.25 and an lr that halves per epoch - so the epoch-to-lr mapping, the label gathering, the batches'
# plumbing and the dropout seed and step counter all show in the parameters.  The network has one hidden layer and no
# LayerNorm (the carried worst-case bound of tests/cspfit_refs.py grows about tenfold per layer and through a LayerNorm)
# and the lr is 5e-6: an Adam step is about lr * sign(g) at first, so an entry whose gradient is smaller than its bound is
# uncertain by a few lr, and that uncertainty re-enters the next forward in proportion to lr - at lr = 1e-3 it swamps the
# gradients' bounds within two steps and the comparison decides nothing, at 5e-6 the bound stays below lr / 2 for more
# than 90 % of every tensor's entries (median below lr / 4) over the six steps, against a movement of 4.5 lr - and of 6 lr
# with a wrong schedule.  Held-out predictions are compared where the restatement's top-2 gap exceeds the scores' bound.
CMP = dict(classes=12, points=600, held=200, epochs=2, steps=3, bs=64, lr=5e-6, lr_decay=0.5, weight_decay=0.01, weight=0.75,
           dropout=0.25, seed=3)
CMP_NET = dict(spa_enc_type="gridcell", F=8, hidden=32, layers=1, act="gelu", use_layn=False, skip=True, num_filts=32,
               min_radius=1.0, max_radius=360.0, dropout=0.0, seed=77)
CMP_EXCUSED_CAP = 0.05


def compare_checkpoint(tmp: str) -> str:
    import os

    from tools import synth
    return synth.write_csp_checkpoint(os.path.join(str(tmp), "cmp.pth.tar"), device="cpu", num_classes=CMP["classes"], **CMP_NET)


def compare_task():
    """(locations (points, 2) float64 holding float32 values, classes): twelve 30-degree bands of longitude; the last
    `held` rows are held out.  Per epoch the (row ids, negatives) pairs of ``batches=``."""
    from range_amd import head_fit
    rng = np.random.default_rng(21)
    n = CMP["points"]
    locs = np.stack([rng.uniform(-180, 180, n), rng.uniform(-80, 80, n)], axis=1).astype(np.float32).astype(np.float64)
    classes = np.minimum(((locs[:, 0] + 180.0) / 30.0).astype(np.int64), CMP["classes"] - 1)
    n_train = n - CMP["held"]
    batches = []
    for _ in range(CMP["epochs"]):
        order = rng.permutation(n_train)
        batches.append([(order[i * CMP["bs"]:(i + 1) * CMP["bs"]],
                         head_fit.rand_locations(rng.random((CMP["bs"], 3), dtype=np.float32), "sphere")) for i in range(CMP["steps"])])
    return locs, classes, batches


def compare_restatement(p0):
    """The loop of fit_location_model restated in float64 from ``xavier_params(p0, classes, seed)``: dict(traj, losses
    (per epoch, with the bound of the epoch's mean), top (held,) the predicted classes, decided (held,) bool - the rows
    whose prediction no float32 run inside the carried bound can change)."""
    import csp_refs
    import cspfit_refs as R
    import headfit_refs as H
    from range_amd import csp_fit
    locs, classes, batches = compare_task()
    start = csp_fit.xavier_params(p0, CMP["classes"], CMP["seed"])
    traj = R.Trajectory(start, start.class_emb, lr=CMP["lr"], weight_decay=CMP["weight_decay"])
    step, losses = 0, []
    for e in range(CMP["epochs"]):
        ls, bs = [], []
        for rows, bg in batches[e]:
            X0 = csp_refs.features(p0.spa_enc_type, np.concatenate([locs[rows], bg.astype(np.float64)]), p0.freq_list)
            drop = R.drop_factors(CMP["seed"], step, p0.widths, X0.shape[0], CMP["dropout"])
            r = traj.step(X0, classes[rows], len(rows), CMP["weight"], drop, lr=CMP["lr"] * CMP["lr_decay"] ** e)
            ls.append(r["loss"])
            bs.append(r["e_loss"])
            step += 1
        losses.append((float(np.mean(ls)), float(np.max(bs)) + 4 * R.U * float(np.mean(ls))))
    n_train = CMP["points"] - CMP["held"]
    net, Wc = traj.current()
    Xh = csp_refs.features(p0.spa_enc_type, locs[n_train:], p0.freq_list)
    E, e_E, _ = R.forward(net, Xh, e_par=traj.e_par())
    e_Wc = traj.adam["class_emb"].e_w
    z = E @ Wc.T
    dz = H.logit_bound(E, Wc) + e_E @ np.abs(Wc).T + np.abs(E) @ e_Wc.T
    score, d_score = H.sigmoid(z), dz / 4.0 + 4 * R.U                  # (the sigmoid's slope is at most 1/4)
    idx = np.arange(CMP["held"])
    top = score.argmax(axis=1)
    margin = (score[idx, top][:, None] - score) - (d_score[idx, top][:, None] + d_score)
    margin[idx, top] = np.inf
    return dict(traj=traj, start=start, losses=losses, top=top, decided=(margin > 0).all(axis=1), held_locs=locs[n_train:],
                held_classes=classes[n_train:])
