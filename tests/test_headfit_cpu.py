"""The class-head fit, CPU side (no GPU): the float64 restatement the GPU tests compare the kernels with
(tests/headfit_refs.py) against what the REFERENCE's own embedding_loss and torch.optim.Adam recorded
(tests/golden/headfit.npz, written by make_golden_headfit.py); the derived bounds (headfit_refs: module docstring)
must hold for the reference's float32 results - a bound the reference breaks is wrong - and must catch every planted
defect; ``rand_locations`` and the sampler of range_amd/head_fit.py; the launch plan under the host sanitizers; the
binding's symbol table against include/range_headfit.h."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import headfit_refs as H
from range_amd import _headfit_native, head_fit

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("base", "wd", "rsw")
STEPS, B = 6, 48


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "headfit.npz"))


def step_inputs(golden, case, i):
    p = f"{case}_s{i}_"
    W = golden[f"{case}_w0"] if i == 0 else golden[f"{case}_s{i - 1}_w"]
    emb = golden[p + "emb"]
    lr, wd, weight = (float(v) for v in golden[f"{case}_hyper"])
    return dict(X=emb[:B], Xbg=emb[B:], labels=golden[p + "labels"], W=W, weight=weight, lr=lr, wd=wd,
                loss=float(golden[p + "loss"]), grad=golden[p + "grad"], w=golden[p + "w"])


def restated(s, defect=None):
    return H.loss_and_grad(s["X"], s["labels"], s["Xbg"], s["W"], s["weight"], defect)


def test_fixture_logits_are_unsaturated(golden):
    for case in CASES:
        for i in range(STEPS):
            assert np.abs(restated(step_inputs(golden, case, i))["z"]).max() <= 6.0
        assert {0, 69} <= set(golden[f"{case}_s0_labels"].tolist())
    assert len(set(golden["base_s1_rows"].tolist())) < B           # a repeated row id


@pytest.mark.parametrize("case", CASES)
def test_reference_loss_and_gradient_inside_the_derived_bounds(golden, case):
    worst_g = worst_l = 0.0
    for i in range(STEPS):
        s = step_inputs(golden, case, i)
        ref = restated(s)
        gb, lb = H.grad_bound(ref, s["W"]), H.loss_bound(ref, s["W"], B, s["weight"])
        err_g, err_l = np.abs(s["grad"] - ref["dW"]), abs(s["loss"] - ref["loss"])
        print(f"{case} step {i}: grad err {err_g.max():.3e} (bound at it {gb.flat[err_g.argmax()]:.3e}, |g| max "
              f"{np.abs(ref['dW']).max():.3e}); loss err {err_l:.3e} (bound {lb:.3e})")
        assert (err_g <= gb).all() and err_l <= lb
        worst_g, worst_l = max(worst_g, float((err_g / gb).max())), max(worst_l, err_l / lb)
    # the bounds are not vacuous either: they stay below 1e-3 of the largest gradient entry / of the loss
    assert gb.max() < 1e-3 * np.abs(ref["dW"]).max() and lb < 1e-3 * abs(ref["loss"])


@pytest.mark.parametrize("defect", ("no_label", "no_eps", "div_B", "weight_on_batch"))
def test_planted_defects_break_the_bounds(golden, defect):
    case = "rsw" if defect == "weight_on_batch" else "base"
    s = step_inputs(golden, case, 0)
    ref, bad = restated(s), restated(s, defect)
    gb, lb = H.grad_bound(ref, s["W"]), H.loss_bound(ref, s["W"], B, s["weight"])
    assert (np.abs(bad["dW"] - s["grad"]) > gb).any(), "the gradient bound does not see the defect"
    assert abs(bad["loss"] - s["loss"]) > lb, "the loss bound does not see the defect"


@pytest.mark.parametrize("case", CASES)
def test_adam_on_the_references_gradients(golden, case):
    """AdamRef fed the fixture's own float32 gradients: class_emb within the carried bound at every step."""
    s0 = step_inputs(golden, case, 0)
    ad = H.AdamRef(s0["W"], lr=s0["lr"], weight_decay=s0["wd"])
    for i in range(STEPS):
        s = step_inputs(golden, case, i)
        ad.step(s["grad"])
        err = np.abs(ad.w - s["w"])
        print(f"{case} step {i}: |w - ref| max {err.max():.3e}, bound max {ad.e_w.max():.3e}")
        assert (err <= ad.e_w).all()
    # not vacuous: an Adam step moves an entry by about lr; the bound stays below 1 % of the six steps' movement
    assert ad.e_w.max() < 0.01 * STEPS * s0["lr"]


@pytest.mark.parametrize("case", CASES)
def test_restated_trajectory_follows_the_reference(golden, case):
    """Loss, gradient and Adam restated end to end from w0 and the recorded embeddings: the reference's float32
    class_emb stays inside the bound accumulated over the six steps."""
    s0 = step_inputs(golden, case, 0)
    ad = H.AdamRef(s0["W"], lr=s0["lr"], weight_decay=s0["wd"])
    for i in range(STEPS):
        s = step_inputs(golden, case, i)
        ref = H.loss_and_grad(s["X"], s["labels"], s["Xbg"], ad.w, s["weight"])
        ad.step(ref["dW"], H.grad_bound(ref, ad.w, ad.e_w))
        err = np.abs(ad.w - s["w"])
        print(f"{case} step {i}: |w - ref| max {err.max():.3e}, bound median {np.median(ad.e_w):.3e} max {ad.e_w.max():.3e}")
        assert (err <= ad.e_w).all()
    assert np.median(ad.e_w) < 0.05 * STEPS * s0["lr"]          # (the bound means something for most entries)


def test_missing_bias_correction_breaks_the_bound(golden):
    s0 = step_inputs(golden, "base", 0)
    good, bad = H.AdamRef(s0["W"], lr=s0["lr"]), H.AdamRef(s0["W"], lr=s0["lr"], defect="no_bias_correction")
    good.step(s0["grad"])
    bad.step(s0["grad"])
    assert (np.abs(bad.w - s0["w"]) > good.e_w).any()


@pytest.mark.parametrize("kind", ("spherical", "sphericalold", "uniform"))
def test_rand_locations_is_the_references(golden, kind):
    u, want = golden[f"rand_{kind}_u"], golden[f"rand_{kind}_loc"]
    got = head_fit.rand_locations(u, kind)
    assert got.dtype == np.float32 and got.shape == want.shape
    if kind == "sphericalold":         # cos / sin of two float32 libraries: a few ulp of the largest value
        assert np.abs(got.astype(np.float64) - want).max() <= 4 * 2.0 ** -23 * 180.0
    else:
        assert np.array_equal(got, want)
    assert np.abs(H.rand_locations64(u, kind) - want).max() <= 8 * 2.0 ** -23 * 180.0
    for case in CASES:                 # ... and the batches' own negatives
        k = str(golden[f"{case}_neg"])
        if k == kind:
            got = head_fit.rand_locations(golden[f"{case}_s0_u"], k)
            assert np.abs(got.astype(np.float64) - golden[f"{case}_s0_bg"]).max() <= 4 * 2.0 ** -23 * 180.0


def test_spherical_negatives_cover_one_octant_and_sphere_the_globe():
    u = np.random.default_rng(0).random((4000, 3), dtype=np.float32)
    s = head_fit.rand_locations(u, "spherical")
    assert s[:, 0].min() >= 0 and s[:, 0].max() < 180 and s[:, 1].min() >= 0 and s[:, 1].max() < 90
    g = head_fit.rand_locations(u, "sphere")
    assert g[:, 0].min() < -170 and g[:, 0].max() > 170 and g[:, 1].min() < -80 and g[:, 1].max() > 80
    # area-uniform: sin(lat) is uniform on [-1, 1)
    assert abs(np.sin(np.radians(g[:, 1].astype(np.float64))).mean()) < 0.05
    assert np.abs(H.rand_locations64(u, "sphere") - g).max() < 1e-4
    with pytest.raises(ValueError):
        head_fit.rand_locations(u, "gaussian")
    with pytest.raises(ValueError):
        head_fit.rand_locations(u.astype(np.float64), "spherical")


def test_balanced_indices_restates_the_sampler():
    rng = np.random.default_rng(3)
    classes = np.concatenate([np.full(250, 4), np.full(3, 0), np.full(100, 9), np.full(1, 7)])
    rng.shuffle(classes)
    a = head_fit.balanced_indices(classes, 100, np.random.default_rng(5))
    assert H.balanced_epoch_stats(a, classes, 100) and len(a) == 100 + 3 + 100 + 1
    assert np.array_equal(a, head_fit.balanced_indices(classes, 100, np.random.default_rng(5)))
    assert not np.array_equal(a, head_fit.balanced_indices(classes, 100, np.random.default_rng(6)))
    assert not np.array_equal(np.sort(a), a)                        # shuffled
    assert not H.balanced_epoch_stats(np.arange(len(classes)), classes, 100)


def test_fit_refuses_bad_arguments_on_the_host():
    x = torch.zeros((4, 3), dtype=torch.float32)
    with pytest.raises(ValueError):
        head_fit.fit_head_on_features(x, [0, 1, 0, 1], lambda n, s, r: None)        # not on the GPU
    with pytest.raises(ValueError):
        head_fit.fit_class_head(object(), np.zeros((2, 2)), [0, 1], neg_rand_type="gaussian")


def test_symbols_are_the_headers():
    with open(os.path.join(REPO, "include", "range_headfit.h")) as f:
        header = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    assert set(re.findall(r"\b(range_headfit_[a-z0-9_]+)\s*\(", header)) == set(_headfit_native.SYMBOLS)
    src = open(os.path.join(REPO, "range_amd", "csrc", "headfit_host.h")).read()
    for name in _headfit_native.SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", src), name
    # the five earlier headers are as they were: nothing of the fit in them
    for other in ("range_hip.h", "range_neighbors.h", "range_probe.h", "range_map.h", "range_cluster.h"):
        assert "headfit" not in open(os.path.join(REPO, "include", other)).read()


def test_headfit_plan_under_sanitizers(tmp_path):
    """host_plan.h: headfit_plan (tests/native/headfit_plan.cpp) compiled with g++ under AddressSanitizer and
    UndefinedBehaviorSanitizer and run on the CPU."""
    exe = str(tmp_path / "headfit_plan")
    src = os.path.join(REPO, "tests", "native", "headfit_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    src, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "headfit_plan ok" in p.stdout, p.stdout + p.stderr
