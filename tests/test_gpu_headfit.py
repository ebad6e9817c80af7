"""The class-head fit on the GPU (`-m gpu`): include/range_headfit.h through range_amd/_headfit_native.py and
range_amd/head_fit.py against the float64 restatement of tests/headfit_refs.py under ITS derived bounds (module
docstring there; tests/test_headfit_cpu.py holds the reference's own float32 results to the same bounds).

Gradient and loss over the shapes that cover the tile height, the 32-class tile, the 8-wide k group, odd row counts of
the x2 MFMA, the narrow tile above F = 512 and the columns of a pass - with labels on columns 0 and C - 1, repeated
row ids, row ids given and not, three or more panels with a ragged last one; a saturated case; bits across grids,
panel widths, streams and runs; Adam alone; the reference's six-step trajectories fed the fixture's batches; the
context's lifecycle and refusals; and a planted task at model level."""
import logging
import os

import numpy as np
import pytest
import torch

import headfit_refs as H
from range_amd import _headfit_native as hn
from range_amd import _native, head_fit
from tools import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
#: (B, Bg, C, F)
SHAPES = [(1, 0, 1, 1), (1, 1, 2, 3), (31, 33, 33, 7), (32, 32, 32, 8), (33, 31, 65, 9), (64, 64, 70, 40),
          (65, 63, 129, 257), (48, 48, 257, 520), (5, 0, 8142, 16)]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "headfit.npz"))


@pytest.fixture(scope="module")
def fit():
    return hn.HeadFit(DEV)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(DEV)


def problem(B, Bg, C, F, seed=0, logit_scale=1.0):
    """Features, repeated row ids, labels with columns 0 and C - 1, background rows, weights: logits ~ N(0, scale)."""
    rng = np.random.default_rng(1000 * seed + B + 7 * C + F)
    N = B + 5
    feats = (rng.standard_normal((N, F)) * 0.7).astype(np.float32)
    rows = rng.integers(0, N, B)
    if B > 2:
        rows[2] = rows[1]
    labels = rng.integers(0, C, B)
    labels[0], labels[-1] = 0, C - 1
    bg = (rng.standard_normal((Bg, F)) * 0.7).astype(np.float32)
    W = (rng.standard_normal((C, F)) * logit_scale / (0.7 * np.sqrt(F))).astype(np.float32)
    return dict(feats=feats, rows=rows, labels=labels, bg=bg, W=W, B=B, Bg=Bg, C=C, F=F)


def on_gpu(p):
    return dict(feats=dev(p["feats"], np.float32), rows=dev(p["rows"], np.int32), labels=dev(p["labels"], np.int32),
                bg=dev(p["bg"], np.float32) if p["Bg"] else None)


def check_against_restatement(p, dW, loss3, weight, what):
    ref = H.loss_and_grad(p["feats"][p["rows"]], p["labels"], p["bg"], p["W"], weight)
    gb, lb = H.grad_bound(ref, p["W"]), H.loss_bound(ref, p["W"], p["B"], weight)
    l3 = loss3.double().cpu().numpy()
    errs = [abs(l3[0] - ref["loss"]), abs(l3[1] - ref["loss_pos"]), abs(l3[2] - ref["label_mean"])]
    if dW is not None:
        g = dW.double().cpu().numpy()
        assert np.isfinite(g).all()
        err = np.abs(g - ref["dW"])
        print(f"{what}: grad err max {err.max():.3e}, err / bound max {(err / gb).max():.3f}; loss errs "
              f"{errs[0]:.3e} {errs[1]:.3e} {errs[2]:.3e} (bound {lb:.3e})")
        assert (err <= gb).all(), f"{what}: gradient outside the derived bound, worst ratio {(err / gb).max():.3f}"
    assert np.isfinite(l3).all() and max(errs) <= lb, f"{what}: loss errors {errs} beyond {lb}"
    return ref


def panels_for(C):
    """A panel width that gives three or more panels with a ragged last one (None: C has fewer than three tiles)."""
    tiles = (C + 31) // 32
    if tiles < 3:
        return None
    per = max(1, (tiles - 1) // 2)
    return 32 * per


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_Bg%d_C%d_F%d" % s)
def test_gradient_and_loss(fit, shape):
    B, Bg, C, F = shape
    p = problem(B, Bg, C, F)
    d = on_gpu(p)
    weight = 0.75
    fit.begin(C, F, p["W"])
    assert (fit.num_classes, fit.width, fit.steps) == (C, F, 0)
    assert np.array_equal(fit.weights().cpu().numpy(), p["W"])
    dW, l3 = fit.grad(d["feats"], d["rows"], d["labels"], d["bg"], weight, validate=True)
    check_against_restatement(p, dW, l3, weight, "grad")
    check_against_restatement(p, None, fit.loss(d["feats"], d["rows"], d["labels"], d["bg"], weight), weight, "loss")
    # without row ids on the gathered rows: the same bits
    dW2, l32 = fit.grad(d["feats"][d["rows"].long()].contiguous(), None, d["labels"], d["bg"], weight)
    assert torch.equal(dW, dW2) and torch.equal(l3, l32)
    # three or more panels with a ragged last one, and a capped grid: the same bits
    pc = panels_for(C)
    if pc:
        plan = hn.plan(C, F, B + Bg, 0, pc)
        assert plan["n_panels"] >= 3 and C % plan["panel_cols"] != 0
        dW3, l33 = fit.grad(d["feats"], d["rows"], d["labels"], d["bg"], weight, panel_cols=pc, max_grid=2)
        assert torch.equal(dW, dW3) and torch.equal(l3, l33)
        assert torch.equal(fit.loss(d["feats"], d["rows"], d["labels"], d["bg"], weight, panel_cols=pc),
                           fit.loss(d["feats"], d["rows"], d["labels"], d["bg"], weight))
    assert fit.steps == 0 and np.array_equal(fit.weights().cpu().numpy(), p["W"])      # nothing was updated


def test_labels_outside_match_no_column_and_row_ids_are_clamped(fit):
    p = problem(33, 31, 65, 9, seed=2)
    d = on_gpu(p)
    fit.begin(65, 9, p["W"])
    lab = p["labels"].copy()
    lab[3], lab[4] = -1, 65
    rows = p["rows"].copy()
    rows[5], rows[6] = -7, 10 ** 6
    dW, l3 = fit.grad(d["feats"], dev(rows, np.int32), dev(lab, np.int32), d["bg"], 1.0)
    q = dict(p, labels=lab, rows=np.clip(rows, 0, len(p["feats"]) - 1))
    check_against_restatement(q, dW, l3, 1.0, "outside labels, clamped rows")
    with pytest.raises(ValueError, match="label outside"):
        fit.grad(d["feats"], d["rows"], dev(lab, np.int32), d["bg"], 1.0, validate=True)
    with pytest.raises(ValueError, match="row id outside"):
        fit.grad(d["feats"], dev(rows, np.int32), d["labels"], d["bg"], 1.0, validate=True)


def test_nan_feature_row_gives_nan_as_in_torch(fit):
    p = problem(33, 31, 65, 9, seed=3)
    p["feats"][p["rows"][0]] = np.nan
    d = on_gpu(p)
    fit.begin(65, 9, p["W"])
    dW, l3 = fit.grad(d["feats"], d["rows"], d["labels"], d["bg"], 1.0)
    assert bool(torch.isnan(dW).all()) and bool(torch.isnan(l3[0]))


def test_saturated_logits(fit):
    """Logits up to +-30: finite, and inside the interval the restatement spans when its logits move by the derived
    logit bound (headfit_refs.g_bound: max |h(z +- dz) - h(z)|, plus the float32 evaluation of 1 - p)."""
    p = problem(64, 64, 70, 40, seed=4, logit_scale=9.0)
    z = H.loss_and_grad(p["feats"][p["rows"]], p["labels"], p["bg"], p["W"])["z"]
    p["W"] = (p["W"] * (30.0 / np.abs(z).max())).astype(np.float32)
    z = H.loss_and_grad(p["feats"][p["rows"]], p["labels"], p["bg"], p["W"])["z"]
    assert 29.0 < np.abs(z).max() <= 30.5 and z.max() > 20 and z.min() < -20
    d = on_gpu(p)
    fit.begin(70, 40, p["W"])
    dW, l3 = fit.grad(d["feats"], d["rows"], d["labels"], d["bg"], 1.0)
    check_against_restatement(p, dW, l3, 1.0, "saturated")


def test_bits_across_grids_panels_streams_and_runs(fit):
    p = problem(65, 63, 129, 257, seed=5)
    d = on_gpu(p)
    args = (d["feats"], d["rows"], d["labels"], d["bg"])
    adam = dict(lr=1e-2, weight=0.5, weight_decay=0.01)

    def run(max_grid=0, panel_cols=0):
        fit.begin(129, 257, p["W"])
        dW, l3 = fit.grad(*args, 0.5, max_grid=max_grid, panel_cols=panel_cols)
        ls = [fit.step(*args, max_grid=max_grid, panel_cols=panel_cols, **adam) for _ in range(2)]
        return dW, l3, ls[0], ls[1], fit.weights()
    want = run()
    assert not torch.equal(want[2], want[3])                     # (the second step started from other weights)
    for kw in (dict(max_grid=1), dict(max_grid=2), dict(panel_cols=32), dict(panel_cols=64, max_grid=3), dict()):
        got = run(**kw)
        for a, b in zip(want, got):
            assert torch.equal(a, b), kw
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        got = run()
    s.synchronize()
    for a, b in zip(want, got):
        assert torch.equal(a, b), "another stream"


@pytest.mark.parametrize("wd", (0.0, 0.01))
def test_adam_alone(fit, wd):
    """Steps 1-3 on the kernel's own gradient bits (range_headfit_grad: what the step feeds to Adam), against float64
    Adam under the bound of its handful of float32 operations (headfit_refs.AdamRef with e_g = 0)."""
    p = problem(33, 31, 65, 9, seed=6)
    d = on_gpu(p)
    args = (d["feats"], d["rows"], d["labels"], d["bg"])
    fit.begin(65, 9, p["W"])
    ad = H.AdamRef(p["W"], lr=3e-3, weight_decay=wd)
    for t in range(1, 4):
        g, _ = fit.grad(*args, 1.0)
        fit.step(*args, lr=3e-3, weight_decay=wd, want_loss=False)
        assert fit.steps == t
        ad.step(g.double().cpu().numpy())
        W = fit.weights().double().cpu().numpy()
        err = np.abs(W - ad.w)
        print(f"wd {wd} step {t}: |W - float64 Adam| max {err.max():.3e}, err / bound max {(err / ad.e_w).max():.3f}, "
              f"moved {np.abs(W - p['W']).max():.3e}")
        assert (err <= ad.e_w).all()
        assert np.abs(W - p["W"]).max() > 0.5 * 3e-3 * t          # ... and it did move, by about lr a step
    assert ad.e_w.max() < 0.01 * 3 * 3e-3


@pytest.mark.parametrize("case", ("base", "wd", "rsw"))
def test_reference_trajectory(fit, golden, case):
    """Six steps fed the fixture's batches (the stub's recorded embeddings): class_emb within the bound accumulated over
    the steps around the float64 trajectory - the reference's float32 one is inside it too (asserted here again)."""
    lr, wd, weight = (float(v) for v in golden[f"{case}_hyper"])
    w0 = golden[f"{case}_w0"]
    fit.begin(70, 40, w0)
    ad = H.AdamRef(w0, lr=lr, weight_decay=wd)
    for i in range(6):
        pre = f"{case}_s{i}_"
        emb, labels = golden[pre + "emb"], golden[pre + "labels"]
        ref = H.loss_and_grad(emb[:48], labels, emb[48:], ad.w, weight)
        lb = H.loss_bound(ref, ad.w, 48, weight, ad.e_w)
        l3 = fit.step(dev(emb[:48], np.float32), None, dev(labels, np.int32), dev(emb[48:], np.float32), lr, weight=weight,
                      weight_decay=wd)
        ad.step(ref["dW"], H.grad_bound(ref, ad.w, ad.e_w))
        W = fit.weights().double().cpu().numpy()
        err, err_ref = np.abs(W - ad.w), np.abs(golden[pre + "w"] - ad.w)
        print(f"{case} step {i}: |W - f64| max {err.max():.3e}, |W - reference| max {np.abs(W - golden[pre + 'w']).max():.3e}, "
              f"bound median {np.median(ad.e_w):.3e}; loss {float(l3[0]):.6f} vs reference {float(golden[pre + 'loss']):.6f}")
        assert (err <= ad.e_w).all() and (err_ref <= ad.e_w).all()
        assert abs(float(l3[0]) - ref["loss"]) <= lb and abs(float(golden[pre + "loss"]) - ref["loss"]) <= lb
    assert fit.steps == 6 and np.median(ad.e_w) < 0.05 * 6 * lr


def test_lifecycle_and_refusals():
    a, b = hn.HeadFit(DEV), hn.HeadFit(DEV)
    with pytest.raises(_native.RangeNativeError, match="no class-head fit begun"):
        a.weights()
    big, small = problem(64, 64, 70, 40, seed=7), problem(31, 33, 33, 24, seed=8)
    db, ds = on_gpu(big), on_gpu(small)
    a.begin(70, 40, big["W"])
    a.step(db["feats"], db["rows"], db["labels"], db["bg"], 1e-2)
    outs = []
    for f in (a, b):
        f.begin(33, 24, small["W"])
        assert f.steps == 0
        dW, l3 = f.grad(ds["feats"], ds["rows"], ds["labels"], ds["bg"], 1.0)
        l3s = f.step(ds["feats"], ds["rows"], ds["labels"], ds["bg"], 1e-2)
        outs.append((dW, l3, l3s, f.weights()))
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    # begin without weights: zeros
    b.begin(5, 3)
    assert not b.weights().any()
    # outside the envelope, natively and in the binding
    lib, h = b.lib, b._h
    for C, F in ((0, 8), (32769, 8), (8, 0), (8, 1025)):
        assert lib.range_headfit_begin(h, C, F, None) != 0
    assert b.num_classes == 5                                       # a refused begin leaves the fit alone
    x = torch.zeros((8200, 3), dtype=torch.float32, device=DEV)
    lab = torch.zeros(8200, dtype=torch.int32, device=DEV)
    out = torch.zeros(3, dtype=torch.float32, device=DEV)
    for B, Bg in ((8193, 0), (4097, 4096), (0, 4)):
        assert lib.range_headfit_loss(h, x.data_ptr(), 8200, None, lab.data_ptr(), B, x.data_ptr() if Bg else None, Bg, 1.0,
                                      out.data_ptr(), None) != 0
    assert lib.range_headfit_loss(h, x.data_ptr(), 8200, None, lab.data_ptr(), 4, None, 3, 1.0, out.data_ptr(), None) != 0
    assert lib.range_headfit_step(h, x.data_ptr(), 8200, None, lab.data_ptr(), 4, None, 0, 1.0, 1e-3, 1.5, 0.999, 1e-8, 0.0,
                                  None, None) != 0              # beta1 outside [0, 1)
    with pytest.raises(ValueError):
        b.loss(x, None, lab, None)                                  # B beyond the envelope
    with pytest.raises(ValueError):
        b.loss(x[:4].double(), None, lab[:4], None)
    assert b.steps == 0
    b.loss(x[:4], None, lab[:4], None)                              # ... and the context still works
    a.engine.close()
    b.engine.close()


# ------------------------------------------------------------------------------------------------ model level
N_CLASSES, N_POINTS, N_HELD = 12, 2000, 400


def planted_task():
    """12 classes, each owning a 30-degree band of longitude; 2000 points, the last 400 held out."""
    rng = np.random.default_rng(11)
    locs = np.stack([rng.uniform(-180, 180, N_POINTS), rng.uniform(-80, 80, N_POINTS)], axis=1)
    classes = np.minimum(((locs[:, 0] + 180.0) / 30.0).astype(np.int64), N_CLASSES - 1)
    return locs, classes


def test_fit_class_head_on_a_planted_task(tmp_path):
    from range_amd import csp_eval, load_model
    from range_amd.grid_predictor import GridPredictor
    ck = synth.write_csp_checkpoint(str(tmp_path / "csp.pth.tar"), spa_enc_type="gridcell", F=8, hidden=64, layers=1,
                                    num_filts=32, num_classes=N_CLASSES, min_radius=1.0, max_radius=360.0)
    model = load_model("CSP", pretrained_path=ck, device=DEV)
    unfitted = load_model("CSP", pretrained_path=ck, device=DEV, class_head=True)
    lm = model.loc_model
    assert lm.num_classes == 0
    locs, classes = planted_task()
    n_train = N_POINTS - N_HELD
    rng = np.random.default_rng(12)
    # three epochs of two batches of 128 rows, from zeros, at the reference's lr: the arg-max of a head does not depend
    # on its scale, and the first-order bound carried through Adam (headfit_refs.AdamRef) stays below the scores' gaps
    # over six small steps on short chains (its worst case grows with the rows of a step - the chain's (R + 1) u
    # against a gradient that cancels - and geometrically with the steps: over many large steps it decides nothing)
    epochs, bs, lr = 3, 128, 1e-3
    batches = []
    for _ in range(epochs):
        order = rng.permutation(n_train)
        batches.append([(order[i:i + bs], head_fit.rand_locations(rng.random((len(order[i:i + bs]), 3), dtype=np.float32), "sphere"))
                        for i in range(0, 2 * bs, bs)])
    w0 = np.zeros((N_CLASSES, 32), dtype=np.float32)
    log = logging.getLogger("headfit_test")
    res = head_fit.fit_class_head(model, locs[:n_train], classes[:n_train], N_CLASSES, epochs=epochs, batch_size=bs, lr=lr,
                                  lr_decay=0.98, init=w0, batches=batches, val=(locs[n_train:], classes[n_train:]), logger=log)
    assert res.weights.shape == (N_CLASSES, 32) and res.weights.dtype == np.float32 and res.steps == epochs * len(batches[0])
    assert len(res.train_losses) == epochs and len(res.val_losses) == epochs
    # (the label's probability itself FALLS over the first steps from zeros - eleven negatives and the background push
    # every logit down along the mean embedding harder than the one label term pulls up - so test()'s loss is compared
    # with the restatement below, not asked to fall)
    assert res.train_losses[-1] < res.train_losses[0] and np.isfinite(res.val_losses).all()
    # the float64 restatement of the same loop on the same (GPU-encoded) embeddings, with its carried bound
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)      # noqa: E731
    feats = lm.encode(to_dev(locs)).double().cpu().numpy()
    ad = H.AdamRef(w0, lr=lr)
    for e in range(epochs):
        for rows, bg in batches[e]:
            xbg = lm.encode(to_dev(bg)).double().cpu().numpy()
            ref = H.loss_and_grad(feats[rows], classes[rows], xbg, ad.w, 1.0)
            ad.step(ref["dW"], H.grad_bound(ref, ad.w, ad.e_w), lr=lr * 0.98 ** e)
    err = np.abs(res.weights - ad.w)
    print(f"model level: |W - f64| max {err.max():.3e}, bound median {np.median(ad.e_w):.3e} max {ad.e_w.max():.3e}")
    assert (err <= ad.e_w).all()
    # predicted classes of the held-out rows: the restatement's wherever its top-2 gap exceeds the bound on a score
    held = feats[n_train:]
    z = held @ ad.w.T
    dz = H.logit_bound(held, ad.w) + np.abs(held) @ ad.e_w.T
    score = H.sigmoid(z)
    d_score = dz / 4.0 + 4 * H.U                                      # (the sigmoid's slope is at most 1/4)
    top = score.argmax(axis=1)
    s_top, d_top = score[np.arange(N_HELD), top], d_score[np.arange(N_HELD), top]
    margin = (s_top[:, None] - score) - (d_top[:, None] + d_score)     # > 0: class j cannot overtake the top class
    margin[np.arange(N_HELD), top] = np.inf
    decided = (margin > 0).all(axis=1)
    print(f"model level: {int((~decided).sum())} of {N_HELD} held-out rows excused")
    assert (~decided).sum() <= 0.02 * N_HELD
    # test() of the last epoch: the mean label term on the held-out rows, within the argument's error d_score / p plus
    # logf and the fixed-order float32 mean (a chain of at most 5 + 1 + 2 + 8 additions): 20 u |L|
    p_lab = score[np.arange(N_HELD), classes[n_train:]]
    want = float(np.mean(-np.log(p_lab + H.EPS)))
    tol = float((d_score.max(axis=1) / p_lab).max() + 20 * H.U * want)
    print(f"model level: test() loss {res.val_losses[-1]:.7f}, restated {want:.7f}, tolerance {tol:.2e}")
    assert abs(res.val_losses[-1] - want) <= tol
    model.loc_model.set_class_head(res.weights)
    assert lm.num_classes == N_CLASSES and "loc_enc.class_emb.weight" in lm.state_dict()
    probs = lm(torch.from_numpy(locs[n_train:]), return_feats=False)
    assert probs.shape == (N_HELD, N_CLASSES)
    pred = probs.argmax(dim=1).cpu().numpy()
    assert np.array_equal(pred[decided], score.argmax(axis=1)[decided])
    # compute_acc_batch on the fitted model beats the unfitted head
    split = np.ones(N_HELD)
    kw = dict(val_feats=locs[n_train:], prior_type="geo_net", return_acc=True)
    _, acc = csp_eval.compute_acc_batch(None, classes[n_train:], split, prior=lm, **kw)
    _, acc0 = csp_eval.compute_acc_batch(None, classes[n_train:], split, prior=unfitted.loc_model, **kw)
    print(f"model level: top-1 {acc[1.0][1]} % fitted, {acc0[1.0][1]} % unfitted")
    assert acc[1.0][1] > acc0[1.0][1] + 10.0
    grid = GridPredictor(np.ones((18, 36)), lm).dense_prediction(3, mask_op=False)
    assert grid.shape == (18, 36) and np.isfinite(grid).all() and grid.max() > grid.min()
    with pytest.raises(ValueError):
        lm.set_class_head(res.weights.astype(np.float64))
    with pytest.raises(ValueError):
        lm.set_class_head(res.weights[:, :5])
