"""The CSP encoder fit on the GPU (`-m gpu`): include/range_cspfit.h through range_amd/_cspfit_native.py and
range_amd/csp_fit.py against the float64 restatement of tests/cspfit_refs.py under ITS derived bounds (module docstring
there; tests/test_cspfit_cpu.py holds the reference's own float32 results to the same bounds).

Every fixture case; the smallest shapes where a tile can go wrong (rows 1 / 31 / 32 / 33 / 65 with Bg = 0 and with B = 1,
widths 1 / 31 / 33 / 96 / 513, F = 1, an in0 that is no multiple of 8, C of 1 / 33 / 70 in panels of 32, row ids given,
repeated and absent, a label outside 0 .. C - 1); bits across grid caps, streams and panel widths; the head against the class-head fit on the same embeddings, bit for
bit; a step against Adam
restated on the gradient launch's bits; the training forward against range_csp_encode; dropout; the six-step
trajectories, re-anchored at the GPU's own parameters step by step; saturated pre-activations, saturated logits and a NaN
location; refusals; a planted task at model level; and fit_location_model against the restatement of its whole loop."""
import dataclasses
import os

import numpy as np
import pytest
import torch

import csp_refs
import cspfit_cases as K
import cspfit_refs as R
from range_amd import _cspfit_native as cn
from range_amd import _headfit_native as hn
from range_amd import _native, csp, csp_fit, head_fit
from tools import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "cspfit.npz"))


@pytest.fixture(scope="module")
def fit():
    return cn.CspFit(DEV)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(DEV)


def make_net(tmp, spa, F, hidden, layers, nf, act, layn, C, seed, skip=True, scale=0.3):
    kw = dict(spa_enc_type=spa, F=F, hidden=hidden, layers=layers, num_filts=nf, act=act, use_layn=layn, skip=skip, num_classes=C,
              class_scale=scale, seed=seed, min_radius=1.0, max_radius=360.0, dropout=0.0,
              freq_init="nerf" if F == 1 else "geometric")
    return csp.read_csp_checkpoint(synth.write_csp_checkpoint(os.path.join(str(tmp), f"n{seed}.pth.tar"), device="cpu", **kw), class_head=True)


def batch(B, Bg, C, seed, N=None):
    """Locations in float32 widened (as the reference feeds them), repeated row ids, labels on columns 0 and C - 1."""
    rng = np.random.default_rng(seed)
    N = N or B + 5
    locs = np.stack([rng.uniform(-180, 180, N), rng.uniform(-90, 90, N)], axis=1).astype(np.float32).astype(np.float64)
    rows = rng.integers(0, N, B)
    if B > 2:
        rows[2] = rows[1]
    labels = rng.integers(0, C, B)
    labels[0], labels[-1] = 0, C - 1
    bg = np.stack([rng.uniform(-180, 180, Bg), rng.uniform(-90, 90, Bg)], axis=1).astype(np.float32).astype(np.float64)
    return dict(locs=locs, rows=rows, labels=labels, bg=bg, B=B, Bg=Bg)


def on_gpu(b):
    return (dev(b["locs"], np.float64), dev(b["rows"], np.int32), dev(b["labels"], np.int32), dev(b["bg"], np.float64) if b["Bg"] else None)


def features(p, b):
    with np.errstate(invalid="ignore"):
        return csp_refs.features(p.spa_enc_type, np.concatenate([b["locs"][b["rows"]], b["bg"]]), p.freq_list)


def check(p, C, b, flat, loss3, weight, what, drop=None, Wc=None):
    Wc = p.class_emb if Wc is None else Wc
    ref = R.loss_and_grads(p, Wc, features(p, b), b["labels"], b["B"], weight, drop)
    l3 = loss3.double().cpu().numpy()
    errs = [abs(l3[0] - ref["loss"]), abs(l3[1] - ref["loss_pos"]), abs(l3[2] - ref["label_mean"])]
    print(f"{what}: loss errs {errs[0]:.3e} {errs[1]:.3e} {errs[2]:.3e} (bound {ref['e_loss']:.3e})")
    assert np.isfinite(l3).all() and max(errs) <= ref["e_loss"], f"{what}: loss errors {errs} beyond {ref['e_loss']}"
    if flat is not None:
        got = cn.split_unpacked(flat.double().cpu().numpy(), p, C)
        assert set(got) == set(ref["grads"])
        for name, g in ref["grads"].items():
            err, bound = np.abs(got[name] - g), ref["bounds"][name]
            print(f"{what} {name}: err max {err.max():.3e}, |g| max {np.abs(g).max():.3e}, err / bound max {(err / bound).max():.4f}")
            assert np.isfinite(got[name]).all() and (err <= bound).all(), f"{what} {name}: outside the derived bound"
    return ref


@pytest.mark.parametrize("case", tuple(K.CASES))
def test_fixture_cases_gradient_and_loss(fit, golden, case):
    p = K.case_params(golden, case)
    locs, labels, bg, rows = K.step_batch(golden, case, 0)
    b = dict(locs=golden[f"{case}_train_locs"].astype(np.float64), rows=rows, labels=labels, bg=bg, B=K.B, Bg=K.BG)
    weight = float(golden[case + "_hyper"][2])
    fit.begin(p, K.C, p.class_emb)
    assert (fit.num_classes, fit.width, fit.steps) == (K.C, p.num_filts, 0)
    flat0 = R.flatten(R.get_params(R.net_of(p), p.class_emb), R.net_of(p))
    assert np.array_equal(fit.flat_params().cpu().numpy(), flat0.astype(np.float32))
    d = on_gpu(b)
    flat, l3 = fit.grad(*d, weight, validate=True)
    check(p, K.C, b, flat, l3, weight, case)
    check(p, K.C, b, None, fit.loss(*d, weight), weight, case + " loss")


#: (spa, F, hidden, layers, num_filts, act, layn, B, Bg, C)
SHAPES = [("gridcell", 1, 1, 1, 1, "sigmoid", True, 1, 0, 1),
          ("gridcell", 2, 31, 1, 33, "gelu", True, 31, 0, 33),
          ("gridcell", 2, 31, 1, 33, "gelu", True, 1, 30, 33),
          ("theory", 3, 18, 2, 31, "relu", True, 1, 31, 70),
          ("gridcell", 8, 96, 1, 33, "tanh", True, 1, 32, 33),
          ("theory", 1, 513, 1, 31, "leakyrelu", True, 1, 64, 70),
          ("gridcell", 8, 32, 2, 96, "gelu", False, 65, 0, 1),
          ("gridcell", 8, 32, 1, 33, "gelu", True, 32, 0, 70),
          ("gridcell", 3, 12, 2, 8, "tanh", True, 33, 0, 33)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%s_F%d_h%d_l%d_nf%d_%s_ln%d_B%d_Bg%d_C%d" % s)
def test_edge_shapes(fit, tmp_path, shape):
    spa, F, hidden, layers, nf, act, layn, B, Bg, C = shape
    p = make_net(tmp_path, spa, F, hidden, layers, nf, act, layn, C, seed=700 + hidden + B)
    b = batch(B, Bg, C, seed=B + 3 * C)
    if B > 3:
        b["labels"][3] = C                       # outside 0 .. C - 1: matches no column
    fit.begin(p, C, p.class_emb)
    d = on_gpu(b)
    weight = 0.75
    flat, l3 = fit.grad(*d, weight)
    check(p, C, b, flat, l3, weight, "shape")
    # without row ids on the gathered locations; a capped grid; panels of 32 classes (three, the last ragged, at C = 70);
    # another stream: the same bits
    outs = {"no row ids": fit.grad(d[0][d[1].long()].contiguous(), None, d[2], d[3], weight), "max_grid 1": fit.grad(*d, weight, max_grid=1),
            "panels of 32": fit.grad(*d, weight, panel_cols=32, max_grid=2)}
    if C == 70:
        assert cn.plan(p.kind, F, p.widths, True, layn, C, B + Bg, 0, 32)["n_panels"] == 3
    torch.cuda.synchronize()                     # (a fit has ONE workspace: its calls on two streams are ordered by the caller)
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        outs["another stream"] = fit.grad(*d, weight)
    s.synchronize()
    for what, (g2, l2) in outs.items():
        assert torch.equal(flat, g2) and torch.equal(l3, l2), what


def test_bits_after_three_steps_across_grids_panels_and_streams(fit, golden):
    case = "tanh_three"
    p = K.case_params(golden, case)
    b = batch(65, 63, K.C, seed=5)
    d = on_gpu(b)
    adam = dict(lr=1e-2, weight=0.5, weight_decay=0.01)

    def run(**kw):
        fit.begin(p, K.C, p.class_emb)
        out = [*fit.grad(*d, 0.5, **kw)]
        out += [fit.step(*d, **adam, **kw) for _ in range(3)]
        return out + [fit.flat_params()]
    want = run()
    assert not torch.equal(want[2], want[3]) and fit.steps == 3
    for kw in (dict(max_grid=1), dict(panel_cols=32), dict(panel_cols=64, max_grid=3), dict(dropout=0.0, seed=99), dict()):
        for a, c in zip(want, run(**kw)):
            assert torch.equal(a, c), kw
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        got = run()
    s.synchronize()
    for a, c in zip(want, got):
        assert torch.equal(a, c), "another stream"


#: (spa, F, hidden, layers, num_filts, act, layn, B, Bg, C, panel_cols): three panels of 32 classes with the last ragged, a
#: ragged 32-row tile and a K that is no multiple of 8; then one class, rows over two tiles, no background, one panel
HEAD_SHAPES = [("gridcell", 3, 12, 2, 33, "tanh", True, 33, 31, 70, 32), ("gridcell", 8, 32, 2, 96, "gelu", False, 65, 0, 1, 0)]


@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=lambda s: "nf%d_C%d_B%d_Bg%d_panel%d" % (s[4], s[9], s[7], s[8], s[10]))
def test_head_of_a_csp_fit_is_the_head_fit(fit, tmp_path, shape):
    """The head of a CSP fit is the class-head fit on the CSP fit's embeddings, bit for bit - gradient, loss scalars and
    an Adam step: both run the one head pass of headfit_host.h.  No tolerance anywhere."""
    spa, F, hidden, layers, nf, act, layn, B, Bg, C, panel_cols = shape
    p = make_net(tmp_path, spa, F, hidden, layers, nf, act, layn, C, seed=900 + nf)
    d = on_gpu(batch(B, Bg, C, seed=B + C))
    weight, adam = 0.75, dict(lr=1e-2, weight_decay=0.01)
    fit.begin(p, C, p.class_emb)
    _, emb = fit.loss(*d, weight, want_emb=True)
    flat, l3 = fit.grad(*d, weight, panel_cols=panel_cols)
    if panel_cols:
        assert cn.plan(p.kind, F, p.widths, True, layn, C, B + Bg, 0, panel_cols)["n_panels"] == 3
    head = hn.HeadFit(DEV)
    head.begin(C, nf, p.class_emb)
    rows = (emb[:B], None, d[2], emb[B:] if Bg else None)
    dW, l3h = head.grad(*rows, weight, panel_cols=panel_cols)
    assert torch.equal(dW, cn.split_unpacked(flat, p, C)["class_emb"]) and torch.equal(l3h, l3)
    fit.step(*d, weight=weight, panel_cols=panel_cols, **adam)
    head.step(*rows, weight=weight, panel_cols=panel_cols, **adam)
    assert (fit.steps, head.steps) == (1, 1)
    W = head.weights()
    assert torch.equal(W, cn.split_unpacked(fit.flat_params(), p, C)["class_emb"])
    assert not torch.equal(W.cpu(), torch.from_numpy(np.ascontiguousarray(p.class_emb, dtype=np.float32)))


@pytest.mark.parametrize("case,wd", (("gelu_ln_skip", 0.0), ("relu_theory", 0.01)))
def test_step_is_adam_on_the_gradient_launchs_bits(fit, golden, case, wd):
    """Steps 1-3 against float64 Adam applied to range_cspfit_grad's bits, under Adam's bound alone (AdamRef, e_g = 0)."""
    p = K.case_params(golden, case)
    b = batch(33, 31, K.C, seed=6)
    d = on_gpu(b)
    fit.begin(p, K.C, p.class_emb)
    traj = R.Trajectory(p, p.class_emb, lr=3e-3, weight_decay=wd)
    start = fit.flat_params().double().cpu().numpy()
    for t in range(1, 4):
        g, _ = fit.grad(*d, 1.0)
        fit.step(*d, lr=3e-3, weight_decay=wd, want_loss=False)
        assert fit.steps == t
        traj.apply(cn.split_unpacked(g.double().cpu().numpy(), p, K.C))
        now = cn.split_unpacked(fit.flat_params().double().cpu().numpy(), p, K.C)
        for name, a in traj.adam.items():
            err = np.abs(now[name] - a.w)
            assert (err <= a.e_w).all(), (t, name, float((err / a.e_w).max()))
            assert a.e_w.max() < 0.01 * 3 * 3e-3
    assert np.abs(fit.flat_params().double().cpu().numpy() - start).max() > 0.5 * 3e-3 * 3


@pytest.mark.parametrize("shape", (("gridcell", 8, 32, 2, 24, "gelu", True), ("theory", 2, 513, 1, 31, "tanh", True),
                                   ("gridcell", 4, 20, 1, 12, "sigmoid", False)))
def test_training_forward_is_range_csp_encode(fit, tmp_path, shape):
    """The embeddings of the training forward (dropout 0) are the bits of the inference kernel for the same network."""
    spa, F, hidden, layers, nf, act, layn = shape
    p = make_net(tmp_path, spa, F, hidden, layers, nf, act, layn, 5, seed=800 + hidden)
    b = batch(70, 27, 5, seed=9)
    d = on_gpu(b)
    fit.begin(p, 5, p.class_emb)
    _, emb = fit.loss(*d, 1.0, want_emb=True)
    eng = fit.engine
    eng.set_csp(p.kind, p.freq_list, p.widths, p.weights, p.biases, p.ln_gamma, p.ln_beta, csp.ACTIVATIONS[p.activation],
                p.skip_connection, p.use_layn)
    want = eng.csp_encode(dev(np.concatenate([b["locs"][b["rows"]], b["bg"]]), np.float64))
    assert torch.equal(emb, want)


def test_dropout(fit, tmp_path):
    # one layer of 96 sigmoid outputs on 64 rows: an output is 0 exactly where it was dropped
    p1 = make_net(tmp_path, "gridcell", 4, 8, 0, 96, "sigmoid", False, 3, seed=31)
    b = batch(40, 24, 3, seed=31)
    d = on_gpu(b)
    fit.begin(p1, 3, p1.class_emb)
    _, emb = fit.loss(*d, 1.0, dropout=0.5, seed=1234567890123, want_emb=True)
    kept = (emb != 0).cpu().numpy()
    assert np.array_equal(kept, R.drop_keep(1234567890123, 0, 0, 64, 96, 0.5))
    assert abs(int(kept.sum()) - 0.5 * kept.size) <= 5 * np.sqrt(kept.size * 0.25)
    # gradients under p = 0.5 against the restatement given the same mix, on a network with skip and LayerNorm
    p = make_net(tmp_path, "gridcell", 4, 16, 2, 12, "gelu", True, 33, seed=32)
    b = batch(33, 31, 33, seed=32)
    d = on_gpu(b)
    fit.begin(p, 33, p.class_emb)
    fit.step(*d, lr=1e-3, dropout=0.5, seed=7)               # the step count enters the mix: test it at 1
    now = fit.trained()
    flat, l3 = fit.grad(*d, 1.0, dropout=0.5, seed=7)
    drop = R.drop_factors(7, 1, p.widths, 64, 0.5)
    check(now, 33, b, flat, l3, 1.0, "dropout", drop=drop, Wc=now.class_emb)
    flat0, l30 = fit.grad(*d, 1.0)
    assert not torch.equal(flat, flat0)
    for kw in (dict(max_grid=1), dict(panel_cols=32, max_grid=2)):
        g2, l2 = fit.grad(*d, 1.0, dropout=0.5, seed=7, **kw)
        assert torch.equal(flat, g2) and torch.equal(l3, l2)
    g3, l33 = fit.grad(*d, 1.0, dropout=0.0, seed=7)
    assert torch.equal(flat0, g3) and torch.equal(l30, l33)
    with pytest.raises(_native.RangeNativeError, match="dropout_p"):
        fit.grad(*d, 1.0, dropout=1.0)


@pytest.mark.parametrize("case", tuple(K.CASES))
def test_reference_trajectory(fit, golden, case):
    """Six steps fed the fixture's batches and negatives: every parameter within the bound carried over the steps
    around the float64 trajectory, which holds the reference's float32 parameters too (tests/test_cspfit_cpu.py)."""
    p = K.case_params(golden, case)
    lr, wd, weight = (float(v) for v in golden[case + "_hyper"])
    fit.begin(p, K.C, p.class_emb)
    traj = R.Trajectory(p, p.class_emb, lr=lr, weight_decay=wd)
    anchored = R.Trajectory(p, p.class_emb, lr=lr, weight_decay=wd)
    locs_dev = dev(golden[f"{case}_train_locs"], np.float64)
    for i in range(K.STEPS):
        locs, labels, bg, rows = K.step_batch(golden, case, i)
        X0 = csp_refs.features(p.spa_enc_type, np.concatenate([locs, bg]), p.freq_list)
        r = traj.step(X0, labels, K.B, weight)
        args = (locs_dev, dev(rows, np.int32), dev(labels, np.int32), dev(bg, np.float64))
        # re-anchored: the gradient at the GPU's OWN parameters against the restatement there, under the one-step bounds
        # (no parameter uncertainty: the float32 parameters are the restatement's inputs); then the step against float64
        # Adam on those gradient bits, which carries Adam's few roundings only
        now = fit.trained()
        g_bits, _ = fit.grad(*args, weight)
        here = R.loss_and_grads(now, now.class_emb, X0, labels, K.B, weight)
        got = cn.split_unpacked(g_bits.double().cpu().numpy(), p, K.C)
        for name, g in here["grads"].items():
            assert (np.abs(got[name] - g) <= here["bounds"][name]).all(), (i, name)
        l3 = fit.step(*args, lr, weight=weight, weight_decay=wd)
        assert abs(float(l3[0]) - here["loss"]) <= here["e_loss"]
        anchored.apply(got)
        after = cn.split_unpacked(fit.flat_params().double().cpu().numpy(), p, K.C)
        for name, a in anchored.adam.items():
            assert (np.abs(after[name] - a.w) <= a.e_w).all(), (i, name)
        assert abs(float(l3[0]) - r["loss"]) <= r["e_loss"]
    now = cn.split_unpacked(fit.flat_params().double().cpu().numpy(), p, K.C)
    for name, a in traj.adam.items():
        err = np.abs(now[name] - a.w)
        print(f"{case} {name}: |GPU - f64| max {err.max():.3e}, |GPU - reference| max {np.abs(now[name] - golden[f'{case}_final_{name}']).max():.3e}, "
              f"bound median {np.median(a.e_w):.3e}")
        assert (err <= a.e_w).all(), name
    # Adam's own bound over the six steps stays below 1 % of their movement: the re-anchored chain decides
    assert max(a.e_w.max() for a in anchored.adam.values()) < 0.01 * K.STEPS * lr
    assert fit.steps == K.STEPS


def test_saturated_logits_and_a_nan_location(fit, golden):
    case = "gelu_ln_skip"
    p = K.case_params(golden, case)
    # |z| about 30: class_emb scaled up
    big = dataclasses.replace(p, class_emb=(p.class_emb * np.float32(40.0)))
    b = batch(33, 31, K.C, seed=41)
    d = on_gpu(b)
    fit.begin(big, K.C, big.class_emb)
    flat, l3 = fit.grad(*d, 1.0)
    ref = check(big, K.C, b, flat, l3, 1.0, "saturated")
    assert np.abs(ref["z"]).max() > 25.0
    # a NaN location: NaN in every gradient its row reaches - all of them, as torch (the fixture's nan_* records)
    fit.begin(p, K.C, p.class_emb)
    b["locs"][b["rows"][3], 0] = np.nan
    d = on_gpu(b)
    flat, l3 = fit.grad(*d, 1.0)
    got = cn.split_unpacked(flat.cpu().numpy(), p, K.C)
    assert np.isnan(l3.cpu().numpy()[0]) and np.isnan(float(golden["nan_loss"]))
    for name, g in got.items():
        assert float(np.isnan(g).mean()) == float(golden[f"nan_grad_isnan_{name}"]) == 1.0, name


def saturate(p, b, target=30.0):
    """``p`` with the first and the last layer's weight and bias scaled so that the largest |Z| of each is `target` on the
    batch ``b`` (float32 scales; the last layer's after the first's)."""
    for l in (0, len(p.widths) - 1):
        ref = R.loss_and_grads(p, p.class_emb, features(p, b), b["labels"], b["B"], 1.0)
        s = np.float32(target / np.abs(ref["caches"][l]["Z"]).max())
        ws, bs = list(p.weights), list(p.biases)
        ws[l], bs[l] = ws[l] * s, bs[l] * s
        p = dataclasses.replace(p, weights=ws, biases=bs)
    return p


@pytest.mark.parametrize("act,layn", (("sigmoid", False), ("tanh", True), ("gelu", True), ("relu", True), ("leakyrelu", False)))
def test_saturated_pre_activations(fit, tmp_path, act, layn):
    """|Z| up to 30 in a hidden layer and in the last layer: act and act' at saturation (sigmoid's p (1 - p), tanh's
    1 - t^2 cancelling, gelu's cdf + z pdf with the exponential underflowing), gradients finite and inside the bounds."""
    C = 33
    p = make_net(tmp_path, "gridcell", 4, 16, 2, 12, act, layn, C, seed=60 + len(act))
    b = batch(33, 31, C, seed=61)
    p = saturate(p, b)
    fit.begin(p, C, p.class_emb)
    d = on_gpu(b)
    flat, l3 = fit.grad(*d, 1.0)
    ref = check(p, C, b, flat, l3, 1.0, "saturated " + act)
    for l in (0, 2):
        z = ref["caches"][l]["Z"]
        assert 29.0 < np.abs(z).max() < 31.0 and (np.abs(z) > 15.0).mean() > 0.02 and z.min() < -15.0 and z.max() > 15.0, (l, np.abs(z).max())
    g, l2 = fit.grad(*d, 1.0, max_grid=1, panel_cols=32)
    assert torch.equal(flat, g) and torch.equal(l3, l2)


def test_refusals(tmp_path, golden):
    a = cn.CspFit(DEV)
    lib, h = a.lib, a._h
    out = torch.zeros(8, dtype=torch.float32, device=DEV)
    assert lib.range_cspfit_params(h, out.data_ptr(), None) != 0
    assert "no CSP fit begun" in lib.range_last_error().decode()
    with pytest.raises(_native.RangeNativeError, match="no CSP fit begun"):
        a.flat_params()
    p = K.case_params(golden, "gelu_ln_skip")
    a.begin(p, K.C, None)
    assert not cn.split_unpacked(a.flat_params().cpu().numpy(), p, K.C)["class_emb"].any()      # NULL: a zero head
    # outside the envelope: a refused begin leaves the fit alone
    with pytest.raises(_native.RangeNativeError, match="envelope"):
        a.begin(p, 32769, None)
    assert a.num_classes == K.C
    x = torch.zeros((8200, 2), dtype=torch.float64, device=DEV)
    lab = torch.zeros(8200, dtype=torch.int32, device=DEV)
    l3 = torch.zeros(3, dtype=torch.float32, device=DEV)
    for B, Bg in ((8193, 0), (4097, 4096), (0, 4)):
        assert lib.range_cspfit_loss(h, x.data_ptr(), 8200, None, lab.data_ptr(), B, x.data_ptr() if Bg else None, Bg, 1.0, 0.0, 0,
                                     l3.data_ptr(), None, None) != 0
    assert "8192" in lib.range_last_error().decode() or "must be" in lib.range_last_error().decode()
    assert lib.range_cspfit_step(h, x.data_ptr(), 8200, None, lab.data_ptr(), 4, None, 0, 1.0, 1e-3, 1.5, 0.999, 1e-8, 0.0, 0.0, 0,
                                 None, None) != 0               # beta1 outside [0, 1)
    with pytest.raises(ValueError):
        a.loss(x, None, lab, None)
    assert a.steps == 0
    a.loss(x[:4], None, lab[:4], None)                               # ... and the context still works
    # the workspace cap: two layers of 1024 on 8192 rows need more than 512 MiB less the head's share
    wide = make_net(tmp_path, "theory", 8, 1024, 1, 1024, "relu", True, 4, seed=55)
    a.begin(wide, 4, None)
    assert lib.range_cspfit_loss(h, x.data_ptr(), 8200, None, lab.data_ptr(), 8192, None, 0, 1.0, 0.0, 0, l3.data_ptr(), None, None) != 0
    assert "workspace" in lib.range_last_error().decode()
    a.loss(x[:64], None, lab[:64], None)
    a.engine.close()


# ------------------------------------------------------------------------------------------------ model level
N_CLASSES, N_POINTS, N_HELD = 12, 2000, 400


def planted_task():
    """12 classes, each owning a 30-degree band of longitude; 2000 points, the last 400 held out."""
    rng = np.random.default_rng(11)
    locs = np.stack([rng.uniform(-180, 180, N_POINTS), rng.uniform(-80, 80, N_POINTS)], axis=1)
    classes = np.minimum(((locs[:, 0] + 180.0) / 30.0).astype(np.int64), N_CLASSES - 1)
    return locs, classes


def top1(model, locs, classes):
    probs = model.loc_model(torch.from_numpy(locs), return_feats=False)
    return float((probs.argmax(1).cpu().numpy() == classes).mean())


def test_fit_location_model_on_a_planted_task(tmp_path):
    """From an untrained ('xavier') encoder: training every layer beats the class head fitted behind the same frozen
    untrained encoder on the same data - the point of the feature; the trained network installs with set_network,
    round-trips through save_csp_checkpoint and evaluates unchanged."""
    from range_amd import csp_eval, load_model
    ck = synth.write_csp_checkpoint(str(tmp_path / "csp.pth.tar"), spa_enc_type="gridcell", F=8, hidden=32, layers=1, num_filts=32,
                                    num_classes=N_CLASSES, min_radius=1.0, max_radius=360.0, dropout=0.0)
    model = load_model("CSP", pretrained_path=ck, device=DEV)
    locs, classes = planted_task()
    n_train = N_POINTS - N_HELD
    kw = dict(epochs=6, batch_size=128, lr=5e-3, neg_rand_type="sphere", balanced=False, seed=3)
    start = csp_fit.xavier_params(model.loc_model.csp_params, N_CLASSES, 3)
    res = csp_fit.fit_location_model(model, locs[:n_train], classes[:n_train], N_CLASSES, init="xavier",
                                     val=(locs[n_train:], classes[n_train:]), **kw)
    assert res.steps == 6 * ((n_train + 127) // 128) and len(res.train_losses) == 6 and len(res.val_losses) == 6
    assert res.train_losses[-1] < res.train_losses[0] and res.val_losses[-1] < res.val_losses[0]
    assert res.params.class_emb.shape == (N_CLASSES, 32) and all(w.dtype == np.float32 for w in res.params.weights)
    # the frozen-encoder head fit behind the SAME untrained encoder, same data and budget
    frozen = load_model("CSP", pretrained_path=ck, device=DEV)
    frozen.loc_model.set_network(dataclasses.replace(start, class_emb=None, num_classes=0))
    hres = head_fit.fit_class_head(frozen, locs[:n_train], classes[:n_train], N_CLASSES, init=start.class_emb, **kw)
    frozen.loc_model.set_class_head(hres.weights)
    model.loc_model.set_network(res.params)
    acc_full, acc_head = top1(model, locs[n_train:], classes[n_train:]), top1(frozen, locs[n_train:], classes[n_train:])
    print(f"held-out top-1: trained encoder {acc_full:.3f}, frozen encoder + fitted head {acc_head:.3f}")
    assert acc_full > acc_head and acc_full > 3.0 / N_CLASSES
    # set_network against a model loaded from save_csp_checkpoint's file: bit for bit
    path = csp.save_csp_checkpoint(str(tmp_path / "trained.pth.tar"), res.params)
    again = load_model("CSP", pretrained_path=path, device=DEV, class_head=True)
    x = torch.from_numpy(locs[n_train:])
    assert torch.equal(model.loc_model(x), again.loc_model(x))
    assert torch.equal(model.loc_model(x, return_feats=False), again.loc_model(x, return_feats=False))
    held_classes, split = classes[n_train:], np.zeros(N_HELD, dtype=np.int64)
    pa, acc_a = csp_eval.compute_acc_batch(None, held_classes, split, locs[n_train:], prior_type="gridcell", prior=model.loc_model,
                                           return_acc=True)
    pb, acc_b = csp_eval.compute_acc_batch(None, held_classes, split, locs[n_train:], prior_type="gridcell", prior=again.loc_model,
                                           return_acc=True)
    assert np.array_equal(np.asarray(pa), np.asarray(pb)) and acc_a == acc_b


def test_fit_location_model_against_the_restated_loop(tmp_path):
    """fit_location_model fed ``batches=`` against the float64 restatement of the same loop (cspfit_cases.CMP: two epochs
    of three batches, a halving lr, weight decay, a background weight, dropout 0.25 by the seed and the step counter):
    every parameter inside the carried bound - below lr / 2 for more than 90 % of the entries, tests/test_cspfit_cpu.py -,
    the epochs' mean losses, and the held-out predictions on every row the bound does not excuse (at most 5 %)."""
    from range_amd import load_model
    c = K.CMP
    ck = K.compare_checkpoint(tmp_path)
    model = load_model("CSP", pretrained_path=ck, device=DEV)
    ref = K.compare_restatement(csp.read_csp_checkpoint(ck))
    locs, classes, batches = K.compare_task()
    n_train = c["points"] - c["held"]
    res = csp_fit.fit_location_model(model, locs[:n_train], classes[:n_train], c["classes"], epochs=c["epochs"], batch_size=c["bs"],
                                     lr=c["lr"], lr_decay=c["lr_decay"], weight_decay=c["weight_decay"], rand_sample_weight=c["weight"],
                                     dropout=c["dropout"], init="xavier", seed=c["seed"], batches=batches)
    assert res.steps == c["epochs"] * c["steps"]
    got = R.get_params(R.net_of(res.params), res.params.class_emb)
    for name, a in ref["traj"].adam.items():
        err = np.abs(got[name] - a.w)
        print(f"{name}: |fit - f64| max {err.max():.3e} ({err.max() / c['lr']:.4f} lr), bound median {np.median(a.e_w) / c['lr']:.3f} lr")
        assert (err <= a.e_w).all(), name
    for got_loss, (want, bound) in zip(res.train_losses, ref["losses"]):
        assert abs(got_loss - want) <= bound
    model.loc_model.set_network(res.params)
    pred = model.loc_model(torch.from_numpy(ref["held_locs"]), return_feats=False).argmax(1).cpu().numpy()
    excused = ~ref["decided"]
    print(f"compared run: {int(excused.sum())} of {c['held']} held-out rows excused")
    assert excused.mean() <= K.CMP_EXCUSED_CAP
    assert np.array_equal(pred[ref["decided"]], ref["top"][ref["decided"]])
