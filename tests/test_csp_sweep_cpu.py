"""The CSP sweep networks (tests/csp_sweep_cases.py), CPU side (no GPU): every network is sane (finite, torch's
float32 operators within 1e-5 relative of the float64 restatement), every network can tell a wrong kernel
from a right one (each planted defect of csp_refs.DEFECTS that applies to it moves the restatement by more than
the bound the GPU test allows the kernel), the saturated networks reach where float32 expf overflows, and the
launch plan gives each case the tile height its name says (tests/native/csp_plan.cpp, whose copy of the width
lists is compared with the table here and whose packing check runs under the host sanitizers in
tests/test_csp_cpu.py)."""
import os
import subprocess

import numpy as np
import pytest

import csp_refs as R
import csp_sweep_cases as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = [("sweep", n) for n in S.SWEEP] + [("saturated", a) for a in S.SATURATED_ACTS]


def _net(group, name):
    return (S.network(name), S.SWEEP[name]["T"]) if group == "sweep" else (S.saturated(name), S.SATURATED[name]["T"])


def test_the_table():
    """Between them the cases reach all ten kernel instantiations and the layer counts the kernel's loops differ by."""
    combos = {(kw["T"], kw["act"]) for kw in S.SWEEP.values()} | {(kw["T"], kw["act"]) for kw in S.SATURATED.values()}
    assert combos >= {(T, a) for T in (32, 64) for a in ("sigmoid", "relu", "leakyrelu", "tanh", "gelu")}
    assert {len(kw["widths"]) for kw in S.SWEEP.values()} >= {1, 2, 3, 4, 6, 9}
    for name, kw in S.SWEEP.items():
        widest = max([S.PER_FREQ[kw["spa_enc_type"]] * kw["F"]] + kw["widths"])
        assert kw["T"] == (64 if widest <= 512 else 32), name
        # a hidden LayerNorm of width 1 gives beta whatever comes in: nothing before it would be tested
        assert not (kw["use_layn"] and 1 in kw["widths"][:-1]), name
        net = S.network(name)
        assert S.widths(net) == kw["widths"] and all(w.dtype == np.float32 for w in net["weights"])
        assert [g is not None for g in net["ln_gamma"]] == [kw["use_layn"] and i + 1 < len(kw["widths"])
                                                            for i in range(len(kw["widths"]))]
    assert np.array_equal(S.network("t64_w1")["freq_list"], [3.7])
    assert S.batch(32).shape == (67, 2) and np.array_equal(S.batch(64), S.queries()[:131])


def test_make_network_follows_the_checkpoint_writer():
    """With one hidden width, make_network draws the tensors tools/synth.py: make_csp_checkpoint draws."""
    from tools import synth
    kw = dict(spa_enc_type="theory", F=5, act="tanh", use_layn=True, skip=True, seed=12)
    sd = synth.make_csp_checkpoint(hidden=24, layers=2, num_filts=7, min_radius=0.1, max_radius=360.0, **kw)["state_dict"]
    net = S.make_network(widths=[24, 24, 7], **kw)
    for i in range(3):
        pre = f"loc_enc.spa_enc.ffn.layers.{i}."
        assert np.array_equal(net["weights"][i], sd[pre + "linear.weight"].numpy())
        assert np.array_equal(net["biases"][i], sd[pre + "linear.bias"].numpy())
        if i < 2:
            assert np.array_equal(net["ln_gamma"][i], sd[pre + "layernorm.weight"].numpy())
            assert np.array_equal(net["ln_beta"][i], sd[pre + "layernorm.bias"].numpy())
    scaled = S.make_network(widths=[24, 24, 7], scale0=40.0, **kw)
    assert np.array_equal(scaled["weights"][0], net["weights"][0] * np.float32(40.0))
    assert all(np.array_equal(a, b) for a, b in zip(scaled["weights"][1:], net["weights"][1:]))


@pytest.mark.parametrize("group,name", ALL)
def test_case_is_sane(group, name):
    net, T = _net(group, name)
    want, f32 = S.restatement(net), S.reference_f32(net)
    assert want.shape == f32.shape == (S.N_REF, S.widths(net)[-1]) and f32.dtype == np.float32
    assert np.isfinite(want).all() and np.isfinite(f32).all()
    e, scale = S.e_ref(net), float(np.abs(want).max())
    rows = 2 * T + 3
    e_batch = float(np.abs(f32[:rows].astype(np.float64) - want[:rows]).max())
    print(f"{name}: E_ref = {e:.3e} (first {rows} rows: {e_batch:.3e}), max|out| = {scale:.4f}, "
          f"E_ref / max|out| = {e / scale:.2e}, GPU bound {S.bound(net):.3e}")
    assert e <= 1e-5 * scale
    assert S.bound(net) == 4.0 * max(e, 2.0 ** -23 * scale)


@pytest.mark.parametrize("act", S.SATURATED_ACTS)
def test_saturated_reaches_the_overflow(act):
    net = S.saturated(act)            # (asserts the reach itself)
    pre = S.pre_activations(net, S.batch(S.SATURATED[act]["T"]))
    print(f"{act}: layer 0 pre-activations from {pre.min():.1f} to {pre.max():.1f}")
    assert pre.max() > S.EXPF_OVERFLOW and pre.min() < -S.EXPF_OVERFLOW
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(np.float32(-pre.min()))) and np.isinf(np.exp(np.float32(pre.max())))   # float32 expf
    assert np.array_equal(net["weights"][1], S.make_network(**{k: v for k, v in S.SATURATED[act].items()
                                                              if k not in ("T", "scale0")})["weights"][1])


@pytest.mark.parametrize("name", list(S.SWEEP))
def test_a_planted_defect_exceeds_the_bound(name):
    """Every defect that applies to the case moves the restatement of the GPU batch beyond the GPU test's bound."""
    net, T = _net("sweep", name)
    q, bound = S.batch(T), S.bound(net)
    base = S.restatement(net)[:len(q)]
    applies = S.applicable_defects(net)
    over = {d: float(np.abs(R.encode(net, q, defect=d) - base).max()) / bound for d in R.DEFECTS}
    print(name, {d: f"{v:.3g}" + ("" if d in applies else " (n/a)") for d, v in over.items()})
    for d in applies:
        assert over[d] > 1.0, (d, over[d])


def test_every_defect_and_tile_height_is_covered():
    seen = {(d, S.SWEEP[n]["T"]) for n in S.SWEEP for d in S.applicable_defects(S.network(n))}
    assert seen == {(d, T) for d in R.DEFECTS for T in (32, 64)}


def test_plan_gives_the_tile_heights(tmp_path):
    """host_plan.h: csp_plan on the table's networks.  tests/native/csp_plan.cpp holds the width lists for its
    packing check; `--sweep` prints them with the plan's tile height and the waves' column tiles."""
    exe = str(tmp_path / "csp_plan")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(REPO, "tests", "native", "csp_plan.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe, "--sweep"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    print(p.stdout)
    got = {}
    for line in p.stdout.splitlines():
        name, *fields = line.split()
        got[name] = dict(f.split("=") for f in fields)
    sat = got.pop("saturated")
    assert set(got) == set(S.SWEEP)
    want_sat = next(iter(S.SATURATED.values()))
    for name, kw, g in [(n, S.SWEEP[n], got[n]) for n in S.SWEEP] + [("saturated", want_sat, sat)]:
        assert (g["kind"], int(g["F"]), [int(w) for w in g["widths"].split(",")], bool(int(g["skip"])), bool(int(g["layn"]))) == \
            (kw["spa_enc_type"], kw["F"], kw["widths"], kw["skip"], kw["use_layn"]), name
        assert int(g["T"]) == kw["T"] and int(g["layers"]) == len(kw["widths"]), name
    # the weight ring's depths and the idle waves the sweep is there to reach
    ntw = {int(v) for g in got.values() for v in g["ntw"].split(",")}
    assert ntw >= {1, 2, 4, 5, 8}
    assert any("3" in g["idle_waves"].split(",") for g in got.values())
