"""The CSP encoder fit, CPU side (no GPU): the float64 restatement the GPU tests compare the kernels with
(tests/cspfit_refs.py) against central differences of its own loss and against what the REFERENCE's own model,
embedding_loss and torch.optim.Adam recorded (tests/golden/cspfit.npz, written by make_golden_cspfit.py); the derived
bounds (cspfit_refs: module docstring) must hold for the reference's float32 results and must catch every planted
defect; the dropout mix; ``save_csp_checkpoint``; the launch plan under the host sanitizers; the binding's symbol
table against include/range_cspfit.h."""
import os
import re
import subprocess

import numpy as np
import pytest

import csp_refs
import cspfit_cases as K
import cspfit_refs as R
from range_amd import _cspfit_native, csp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = tuple(K.CASES)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "cspfit.npz"))


@pytest.fixture(scope="module")
def nets(golden):
    return {c: K.case_params(golden, c) for c in CASES}


def step_inputs(golden, p, case, i):
    locs, labels, bg, _ = K.step_batch(golden, case, i)
    X0 = csp_refs.features(p.spa_enc_type, np.concatenate([locs, bg]), p.freq_list)
    return X0, labels


def restated(golden, nets, case, defect=None):
    p = nets[case]
    X0, labels = step_inputs(golden, p, case, 0)
    return R.loss_and_grads(p, p.class_emb, X0, labels, K.B, float(golden[case + "_hyper"][2]), defect=defect)


def test_fixture_covers_what_it_should(nets):
    acts = {nets[c].activation for c in CASES}
    assert acts == {"sigmoid", "relu", "leakyrelu", "tanh", "gelu"}
    live = {c: [i + 1 < len(nets[c].widths) and nets[c].skip_connection and w.shape[0] == w.shape[1]
                for i, w in enumerate(nets[c].weights)] for c in CASES}
    assert any(any(v) for v in live.values()) and not any(live["sigmoid_dead"]) and any(live["relu_theory"])
    assert {len(nets[c].widths) for c in CASES} >= {1, 2, 4}
    assert {nets[c].use_layn for c in CASES} == {True, False}
    assert all(nets[c].dropout == 0.0 and sum(w.size for w in nets[c].weights) < 5000 for c in CASES)


@pytest.mark.parametrize("case", CASES)
def test_gradients_match_central_differences(golden, nets, case):
    """The backward of the restatement against central differences of its own float64 loss: independent of torch."""
    p = nets[case]
    X0, labels = step_inputs(golden, p, case, 0)
    weight = float(golden[case + "_hyper"][2])
    r = R.loss_and_grads(p, p.class_emb, X0, labels, K.B, weight)
    net = R.net_of(p)
    base = R.get_params(net, p.class_emb)
    rng = np.random.default_rng(1)
    h = 1e-5
    for name, g in r["grads"].items():
        flat = base[name].ravel()
        scale = np.abs(g).max()
        for j in rng.choice(flat.size, min(6, flat.size), replace=False):
            vals = []
            for sgn in (1, -1):
                traj = R.Trajectory(net, p.class_emb)
                traj.adam[name].w.ravel()[j] = flat[j] + sgn * h
                n2, W2 = traj.current()
                vals.append(R.float64_loss(n2, W2, X0, labels, K.B, weight))
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(fd - g.ravel()[j]) <= 1e-6 * (abs(g.ravel()[j]) + scale) + 1e-10, (name, j, fd, g.ravel()[j])


@pytest.mark.parametrize("case", CASES)
def test_reference_gradients_and_loss_inside_the_derived_bounds(golden, nets, case):
    r = restated(golden, nets, case)
    worst = 0.0
    for name, g in r["grads"].items():
        ref = golden[f"{case}_grad_{name}"]
        err, b = np.abs(ref - g), r["bounds"][name]
        print(f"{case} {name}: err {err.max():.3e}, bound at it {b.flat[err.argmax()]:.3e}, |g| max {np.abs(g).max():.3e}, "
              f"worst ratio {(err / b).max():.3f}")
        assert (err <= b).all(), name
        worst = max(worst, float((err / b).max()))
        if name in ("class_emb", f"w{len(nets[case].widths) - 1}"):
            # the bound means something where the chain of worst cases is short; it grows about tenfold per layer below
            assert np.median(b) < 5e-2 * np.abs(g).max(), name
    err_l = abs(float(golden[case + "_s0_loss"]) - r["loss"])
    assert err_l <= r["e_loss"] and r["e_loss"] < 5e-2 * abs(r["loss"])
    err_e = np.abs(golden[case + "_emb"] - r["E"])
    assert (err_e <= r["e_E"]).all()
    print(f"{case}: worst gradient ratio {worst:.3f}, loss ratio {err_l / r['e_loss']:.3f}, embedding ratio {(err_e / r['e_E']).max():.3f}")


DEFECT_CASE = {"no_skip_grad": "gelu_noln_skip", "act_prime_at_a": "tanh_three", "tanh_gelu": "gelu_ln_skip", "ln_no_mean": "gelu_ln_skip",
               "unbiased_var": "relu_theory", "db_mean": "sigmoid_dead", "no_out_act": "leaky_nohidden"}


@pytest.mark.parametrize("defect", sorted(DEFECT_CASE))
def test_planted_defects_break_the_bounds(golden, nets, defect):
    case = DEFECT_CASE[defect]
    good, bad = restated(golden, nets, case), restated(golden, nets, case, defect)
    broken = [name for name in good["grads"] if (np.abs(bad["grads"][name] - golden[f"{case}_grad_{name}"]) > good["bounds"][name]).any()]
    assert broken, "no gradient bound sees the defect"
    print(defect, "seen by", broken)


def test_unscaled_mask_breaks_the_bounds(golden, nets):
    """Dropout has no reference to follow (its masks are the project's own): the defect against the restatement."""
    case = "gelu_ln_skip"
    p = nets[case]
    X0, labels = step_inputs(golden, p, case, 0)
    good = R.loss_and_grads(p, p.class_emb, X0, labels, K.B, 1.0, drop=R.drop_factors(7, 0, p.widths, X0.shape[0], 0.5))
    bad = R.loss_and_grads(p, p.class_emb, X0, labels, K.B, 1.0, drop=R.drop_factors(7, 0, p.widths, X0.shape[0], 0.5, "mask_unscaled"))
    assert any((np.abs(bad["grads"][k] - good["grads"][k]) > good["bounds"][k]).any() for k in good["grads"])


@pytest.mark.parametrize("case", CASES)
def test_restated_trajectory_follows_the_reference(golden, nets, case):
    """Six Adam steps restated end to end: the reference's float32 parameters stay inside the carried bound."""
    p = nets[case]
    lr, wd, weight = (float(v) for v in golden[case + "_hyper"])
    traj = R.Trajectory(p, p.class_emb, lr=lr, weight_decay=wd)
    for i in range(K.STEPS):
        X0, labels = step_inputs(golden, p, case, i)
        r = traj.step(X0, labels, K.B, weight)
        assert abs(float(golden[f"{case}_s{i}_loss"]) - r["loss"]) <= r["e_loss"], i
        if i in (2, K.STEPS - 1):
            tag = "mid" if i == 2 else "final"
            for name, a in traj.adam.items():
                err = np.abs(golden[f"{case}_{tag}_{name}"] - a.w)
                print(f"{case} {tag} {name}: err {err.max():.3e}, bound median {np.median(a.e_w):.3e} max {a.e_w.max():.3e}")
                assert (err <= a.e_w).all(), (tag, name)


def test_compared_run_decides_on_the_cpu(tmp_path):
    """The model-level comparison of tests/test_gpu_cspfit.py (cspfit_cases.compare_restatement), restatement alone: at
    the chosen seed the rows its bound excuses stay inside the cap, and the carried bound is no blanket - below lr / 2 for
    more than 90 % of every tensor's entries, its median below lr / 4, against a movement of about 4.5 lr."""
    r = K.compare_restatement(csp.read_csp_checkpoint(K.compare_checkpoint(tmp_path)))
    excused = float((~r["decided"]).mean())
    print(f"compared run: {excused:.3f} of the held-out rows excused")
    assert excused <= K.CMP_EXCUSED_CAP
    lr = K.CMP["lr"]
    start = R.get_params(R.net_of(r["start"]), r["start"].class_emb)
    for name, a in r["traj"].adam.items():
        moved = np.abs(a.w - start[name])
        print(f"{name}: e_w / lr median {np.median(a.e_w) / lr:.3f}, share below lr / 2 {(a.e_w < 0.5 * lr).mean():.3f}, moved / lr median "
              f"{np.median(moved) / lr:.2f}")
        assert (a.e_w < 0.5 * lr).mean() > 0.9 and np.median(a.e_w) < 0.25 * lr
        assert np.median(moved) > 2.0 * lr
    for loss, bound in r["losses"]:
        assert bound < 1e-3 * loss


def test_missing_bias_correction_breaks_the_bound(golden, nets):
    case = "gelu_ln_skip"
    p = nets[case]
    lr, wd, _ = (float(v) for v in golden[case + "_hyper"])
    grads = {k: golden[f"{case}_grad_{k}"] for k in R.param_names(R.net_of(p))}
    good, bad = R.Trajectory(p, p.class_emb, lr=lr, weight_decay=wd), R.Trajectory(p, p.class_emb, lr=lr, weight_decay=wd,
                                                                                  defect="no_bias_correction")
    good.apply(grads)
    bad.apply(grads)
    assert any((np.abs(bad.adam[k].w - good.adam[k].w) > good.adam[k].e_w).any() for k in grads)


def test_nan_location_as_torch(golden, nets):
    """What torch did with a NaN location (recorded by the generator): a NaN loss and NaN in every gradient the row
    reaches - all of them here, the row's embedding being NaN in every column; the restatement agrees."""
    assert np.isnan(golden["nan_loss"])
    case = CASES[0]
    p = nets[case]
    locs, labels, bg, _ = K.step_batch(golden, case, 0)
    locs = locs.copy()
    locs[3, 0] = np.nan
    with np.errstate(invalid="ignore"):
        X0 = csp_refs.features(p.spa_enc_type, np.concatenate([locs, bg]), p.freq_list)
        r = R.loss_and_grads(p, p.class_emb, X0, labels, K.B, 1.0)
    for name, g in r["grads"].items():
        assert float(golden[f"nan_grad_isnan_{name}"]) == float(np.isnan(g).mean()), name


def test_dropout_mix():
    keep = R.drop_keep(5, 3, 1, 64, 96, 0.5)
    n = keep.size
    assert abs(keep.sum() - 0.5 * n) <= 5 * np.sqrt(n * 0.25)
    assert np.array_equal(keep, R.drop_keep(5, 3, 1, 64, 96, 0.5))
    for other in ((6, 3, 1), (5, 4, 1), (5, 3, 2), (5 + (1 << 32), 3, 1)):
        assert not np.array_equal(keep, R.drop_keep(*other, 64, 96, 0.5))
    # a row's mask does not depend on how many rows there are
    assert np.array_equal(keep[:7], R.drop_keep(5, 3, 1, 7, 96, 0.5))
    assert R.drop_keep(5, 3, 1, 64, 96, 0.25).mean() > 0.7
    assert int(R.mix(0)) == 0 and int(R.mix(1)) != 1


@pytest.mark.parametrize("case", ("gelu_ln_skip", "leaky_nohidden"))
def test_save_csp_checkpoint_round_trip(golden, nets, case, tmp_path):
    p = nets[case]
    path = csp.save_csp_checkpoint(str(tmp_path / "net.pth.tar"), p)
    q = csp.read_csp_checkpoint(path, class_head=True)
    for a, b in zip(p.weights + p.biases + [p.class_emb], q.weights + q.biases + [q.class_emb]):
        assert a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for a, b in zip(p.ln_gamma + p.ln_beta, q.ln_gamma + q.ln_beta):
        assert (a is None) == (b is None) and (a is None or np.array_equal(a.view(np.uint32), b.view(np.uint32)))
    assert (q.spa_enc_type, q.frequency_num, q.activation, q.use_layn, q.skip_connection, q.widths, q.num_classes, q.dropout) == \
        (p.spa_enc_type, p.frequency_num, p.activation, p.use_layn, p.skip_connection, p.widths, p.num_classes, p.dropout)
    assert np.array_equal(q.freq_list, p.freq_list)
    # without a head: written and read without one
    import dataclasses
    bare = dataclasses.replace(p, class_emb=None, num_classes=0)
    path = csp.save_csp_checkpoint(str(tmp_path / "bare.pth.tar"), bare)
    assert csp.read_csp_checkpoint(path).class_emb is None
    with pytest.raises(ValueError):
        csp.read_csp_checkpoint(path, class_head=True)


def test_reader_and_writer_refusals(nets, tmp_path):
    import dataclasses

    import torch
    p = nets["gelu_ln_skip"]
    with pytest.raises(ValueError):
        csp.save_csp_checkpoint(str(tmp_path / "x"), dataclasses.replace(p, weights=[w.astype(np.float64) for w in p.weights]))
    with pytest.raises(NotImplementedError):
        csp.save_csp_checkpoint(str(tmp_path / "x"), dataclasses.replace(p, spa_enc_type="rbf"))
    path = csp.save_csp_checkpoint(str(tmp_path / "ok.pth.tar"), p)
    ck = torch.load(path, weights_only=True)
    for key, val, exc in (("spa_enc_type", "rbf", NotImplementedError), ("freq_init", "random", NotImplementedError),
                          ("frequency_num", 65, ValueError), ("num_hidden_layer", 9, ValueError), ("spa_f_act", "swish", NotImplementedError)):
        bad = {"params": dict(ck["params"], **{key: val}), "state_dict": ck["state_dict"]}
        torch.save(bad, str(tmp_path / "bad.pth.tar"))
        with pytest.raises(exc):
            csp.read_csp_checkpoint(str(tmp_path / "bad.pth.tar"))


def test_symbols_are_the_headers():
    with open(os.path.join(REPO, "include", "range_cspfit.h")) as f:
        header = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    assert set(re.findall(r"\b(range_cspfit_[a-z0-9_]+)\s*\(", header)) == set(_cspfit_native.SYMBOLS)
    src = open(os.path.join(REPO, "range_amd", "csrc", "cspfit_host.h")).read()
    for name in _cspfit_native.SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", src), name
    for other in ("range_hip.h", "range_headfit.h", "range_neighbors.h", "range_probe.h", "range_map.h", "range_cluster.h"):
        assert "cspfit" not in open(os.path.join(REPO, "include", other)).read()


def test_unpacked_layout_is_the_restatements_order(nets):
    for case in CASES:
        p = nets[case]
        names = [n for n, _, _ in _cspfit_native.unpacked_layout(p, K.C)]
        assert names == R.param_names(R.net_of(p))


def test_cspfit_plan_under_sanitizers(tmp_path):
    """host_plan.h: cspfit_plan (tests/native/cspfit_plan.cpp) compiled with g++ under AddressSanitizer and
    UndefinedBehaviorSanitizer and run on the CPU: every row and column covered exactly once at the edge shapes."""
    exe = str(tmp_path / "cspfit_plan")
    src = os.path.join(REPO, "tests", "native", "cspfit_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    src, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "cspfit_plan ok" in p.stdout, p.stdout + p.stderr
