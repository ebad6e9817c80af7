"""The location-encoder sweep (tests/enc_sweep_cases.py), CPU side (no GPU): the float64 oracle stays within a tenth
of the GPU bound of an 80-bit long-double restatement for every case; it agrees with two fixtures the reference's
closed form produced beyond L = 40; every planted defect moves e-hat far beyond the bound; the cases' launch plans
(tests/native/enc_sweep_plan.cpp, built here with g++) reach every entry of the five launch tables of encoder_host.h
but the two no plan can reach; the plan's invariants hold over the whole envelope under AddressSanitizer /
UndefinedBehaviorSanitizer; and the host checks accept what the sweep runs."""
import os
import re
import subprocess

import numpy as np
import pytest

import enc_sweep_cases as S
from oracle import range_oracle as O
from tools import synth

CSRC = os.path.join(S.REPO, "range_amd", "csrc")


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return S.build_plan_program(tmp_path_factory.mktemp("enc_sweep_plan"))


def test_the_tables():
    """What the sweep is there to hold: the neighbours of the round-count steps, both modes, every kernel width, a
    padded width beyond L = 40, the layer counts, and a 32-query case per width."""
    sweep = S.SWEEP.values()
    assert {c[0] for c in sweep} >= {41, 47, 48, 55, 56, 57, 63, 64}
    assert {c[3] for c in sweep} == {"analytic", "closed-form"}
    assert {S.kernel_hidden_width(c[1]) for c in sweep if c[0] > 40} == set(S.KERNEL_WIDTHS)
    assert any(c[0] > 40 and S.kernel_hidden_width(c[1]) != c[1] for c in sweep)
    assert {c[2] for c in sweep} >= {1, 2, 3, 4, 5, 7}
    assert S.SWEEP["L64_H256_n7"][:3] == (64, 256, 7) and S.SWEEP["L10_H64_n7"][:3] == (10, 64, 7)
    assert all(1 <= c[0] <= 64 and 1 <= c[1] <= 1024 and 1 <= c[2] <= 7 for c in S.CASES.values())
    # one L = 10 case per width that has 32-query workgroups, L = 64 at two widths
    assert sorted(c[1] for c in S.WG32.values() if c[0] == 10) == [64, 128, 192, 256, 320, 384, 448, 512]
    assert len({c[1] for c in S.WG32.values() if c[0] == 64}) == 2
    assert set(S.ROUTES) == {n for n, c in S.SWEEP.items() if c[0] > 40} and set(S.IN_TURN) <= set(S.SWEEP)
    assert len({S.seed_of(n) for n in S.CASES}) == len(S.CASES)
    # the rows: the fixed ones first, three quarters of the rest within |lat| <= 45, all within 89.999 but the poles
    q = S.queries(128)
    assert q.shape == (128, 2) and not q.flags.writeable and np.array_equal(q[:7], S.FIXED_ROWS)
    assert np.signbit(q[6]).all() and {90.0, -90.0, 0.0, 0.001} <= set(q[:7, 1]) and {-180.0, 180.0} <= set(q[:7, 0])
    lat = np.abs(S.queries(3000)[7:, 1])
    assert lat.max() <= 89.999 and 0.74 < (lat <= 45.0).mean() < 0.76
    assert np.array_equal(S.queries(1), S.FIXED_ROWS[:1]) and np.abs(S.equator_queries(200)[:, 1]).max() <= 5.0
    assert S.bound("L64_H512_n2") == 2e-12 and S.bound("L64_H600_n2") == S.bound("L64_H1024_n2") == 4e-12


@pytest.mark.parametrize("case", list(S.CASES))
def test_oracle_against_long_double(case):
    """The float64 oracle against its long-double restatement on 128 rows: a tenth of the bound the kernel gets."""
    L, hidden, layers, mode, _ = S.CASES[case]
    q = S.queries(128)
    ld = S.encode_ld(q, S.weights(case), L, mode)
    err = float(np.abs(S.oracle(case, 128) - ld).max())
    print(f"{case}: max |oracle - long double| = {err:.3e}, bound / 10 = {S.bound(case) / 10:.1e}")
    assert np.isfinite(ld).all() and np.abs(np.linalg.norm(ld, axis=1) - 1.0).max() < 1e-15
    assert err <= S.bound(case) / 10


def test_long_double_restatement_is_its_own():
    """encode_ld shares no feature code with the oracle, and its features are the oracle's to float64 rounding."""
    import inspect
    assert "sh_features" not in inspect.getsource(S.encode_ld) + inspect.getsource(S.features_ld)
    assert np.finfo(S.LD).eps < 2e-19
    q = S.queries(64)
    for mode in ("analytic", "closed-form"):
        d = np.abs(S.features_ld(q, 64, mode).astype(np.float64) - O.sh_features(q, 64, mode)).max()
        print(f"L = 64 {mode}: max |features - long double| = {d:.2e}")
        assert d < 1e-12


@pytest.mark.parametrize("tag", list(S.E_GOLDEN))
def test_oracle_against_the_fixtures(tag):
    """The reference's closed form through the reference's SirenNet (tests/golden/make_golden_enc_sweep.py), normalised
    as tests/test_gpu_parity.py: test_encoder_vs_reference_golden does: no further from the oracle than recorded."""
    path = os.path.join(S.GOLDEN, tag + ".npz")
    assert os.path.getsize(path) < 300 * 1024
    z = np.load(path)
    L, hidden, layers, mode = int(z["L"]), int(z["hidden"]), int(z["num_hidden_layers"]), str(z["mode"])
    assert tag == f"enc_closedform_L{L}_H{hidden}_n{layers}" and mode == "closed-form" and int(z["seed"]) == S.FIXTURE_SEED[tag]
    q = z["lonlat"]
    assert np.array_equal(q, S.queries(S.FIXTURE_ROWS, S.FIXTURE_SEED[tag])) and z["embedding"].shape == (S.FIXTURE_ROWS, 256)
    ref = z["embedding"] / np.linalg.norm(z["embedding"], axis=1, keepdims=True)
    w = synth.make_encoder_weights(L, hidden, 256, layers, int(z["seed"]))
    e = float(np.abs(O.encode(q, w, L, mode) - ref).max())
    print(f"{tag}: max |oracle - reference| = {e:.3e} (recorded {S.E_GOLDEN[tag]:.3e}); "
          f"long double - reference = {np.abs(S.encode_ld(q, w, L, mode) - ref).max():.3e}")
    assert e <= S.E_GOLDEN[tag]
    assert 4 * S.E_GOLDEN[tag] < 2e-12 / 10          # the GPU test's bound is the kernel's own, to a tenth


@pytest.mark.parametrize("case", list(S.SWEEP))
def test_planted_defects(case):
    """Every defect that applies to the case moves e-hat by more than 10 x the bound on at least half of 128 rows."""
    q, base, bound = S.queries(128), S.oracle(case, 128), S.bound(case)
    applies = S.applicable_defects(case)
    assert applies
    for d in applies:
        moved = np.abs(S.encode_with_defect(case, q, d) - base).max(axis=1)
        rows = int((moved > 10 * bound).sum())
        print(f"{case} {d}: median move {np.median(moved):.2e}, {rows} of {len(q)} rows beyond 10 x bound")
        assert rows >= len(q) // 2, (d, rows)


def test_every_defect_is_planted_somewhere():
    seen = {d for n in S.SWEEP for d in S.applicable_defects(n)}
    assert seen == set(S.DEFECTS) and len(S.DEFECTS) == 7
    assert any(S.SWEEP[n][0] > 40 for n in S.SWEEP if "odd_order_sign" in S.applicable_defects(n))
    assert any(S.SWEEP[n][2] >= 5 for n in S.SWEEP if "hidden_2_and_3_exchanged" in S.applicable_defects(n))
    # without a defect nothing moves
    q = S.queries(16)
    w = S.weights("L41_H64_n1")
    assert np.array_equal(O.encode(q, w, 41, "analytic", features=O.sh_features(q, 41, "analytic")), O.encode(q, w, 41, "analytic"))


def test_launch_table_coverage(plan_exe):
    """With 256 CUs the plans of the cases' GPU runs reach every entry of ENC_TILE, ENC_L1_PART, ENC_L2_PART, ENC_REST
    and ENC_MAIN but UNREACHABLE, and every ENC_MAIN entry of up to 8 tiles in both workgroup sizes.  A new table
    entry without a case fails here."""
    tables = S.launch_tables()
    assert set(tables) == {"ENC_TILE", "ENC_L1_PART", "ENC_L2_PART", "ENC_REST", "ENC_MAIN"}
    entries = {(t, nt) for t, nts in tables.items() for nt in nts}
    assert len(entries) == sum(len(v) for v in tables.values()) == 28
    assert {nt * 64 for nt in tables["ENC_MAIN"]} == set(S.KERNEL_WIDTHS)
    reached, main32, main16, seen = set(), set(), set(), {}
    for name in S.CASES:
        rows = S.case_rows(name)
        for row, d in zip(rows, S.plans(plan_exe, rows)):
            reached |= d["tables"]
            for e in d["tables"]:
                seen.setdefault(e, (name, row[4:]))
            if d["main32"]:
                main32.add(d["H"] // 64)
            if d["main16"]:
                main16.add(d["H"] // 64)
            # what the comments of the cases file promise
            if name in S.WG32 and (row[4], row[5]) == (1, 1):
                assert d["n_wg32"] > 0, (name, row)
    for e in sorted(seen):
        print(e, "first reached by", seen[e])
    assert S.UNREACHABLE <= entries and not (reached & S.UNREACHABLE)
    assert reached == entries - S.UNREACHABLE, sorted(entries - S.UNREACHABLE - reached)
    assert main32 == {nt for nt in tables["ENC_MAIN"] if nt <= 8} and main16 >= set(tables["ENC_MAIN"])
    # the forms the batches are chosen for
    by = {}
    for name in S.SWEEP:
        rows = [r for r in S.case_rows(name) if (r[4], r[5]) == (1, 1)]
        for d in S.plans(plan_exe, rows):
            by.setdefault(name, []).append(d)
    every = [d for ds in by.values() for d in ds]
    assert any(d["one_launch"] and d["KP"] == 7 and d["L"] > 40 for d in every)
    assert {d["part2_cols"] for d in every if d["one_launch"] and d["tiles"] > 32} >= {64, 128, 256}
    assert any(not d["one_launch"] and d["S2"] > 1 and d["layers"] != 2 for d in every)
    assert any(d["S"] > 1 and d["KP"] > 1 for d in every) and any(d["main16"] and d["L"] > 40 for d in every)
    assert {d["n_rounds"] for d in every} >= {6, 7, 8, 9} and {d["max_round"] for d in every if d["L"] == 64} == {512}


def test_no_plan_reaches_the_unreachable_entries(plan_exe):
    """Over L = 1..64, every kernel width, 1..7 layers, the sweep's batch sizes and both switches at 256 CUs: the set
    of table entries reached is every entry but UNREACHABLE."""
    p = subprocess.run([plan_exe, "--reach"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    reached = {(ln.split()[0], int(ln.split()[1])) for ln in p.stdout.splitlines()}
    entries = {(t, nt) for t, nts in S.launch_tables().items() for nt in nts}
    assert reached == entries - S.UNREACHABLE


def test_plan_invariants_under_sanitizers(tmp_path):
    """enc_sweep_plan --sweep built with -fsanitize=address,undefined: the slot plan a permutation, main_B + split_B
    = B, every tile covered once, tiles x S x KP within the CUs, part widths a table has, workspaces and LDS rows
    that cover what the kernels write, LDS within 160 KiB over the whole envelope with and without the table."""
    exe = S.build_plan_program(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    p = subprocess.run([exe, "--sweep"], capture_output=True, text=True, timeout=600)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "enc_sweep_plan ok" in p.stdout and "FAILED" not in p.stdout
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr


def test_host_checks_accept_what_the_sweep_runs(plan_exe):
    """range_set_encoder takes 7 hidden layers and refuses 8; L = 64 at 512 and 1024 columns fits the LDS cap with
    and without the table.  The plan program restates the LDS sizes of encoder_host.h: the two texts are compared."""
    host = open(os.path.join(CSRC, "encoder_host.h")).read()
    kern = open(os.path.join(CSRC, "encoder_kernel.h")).read()
    plan_src = open(S.PLAN_SRC).read()
    max_layers = int(re.search(r"constexpr int ENC_MAX_LAYERS = (\d+);", kern).group(1))
    assert "if (NL < 1 || NL + 1 > ENC_MAX_LAYERS) return fail(RANGE_ERR_INVALID" in host
    assert 7 + 1 <= max_layers < 8 + 1
    assert "if (L < 1 || L > 64) return fail(RANGE_ERR_INVALID" in host
    assert int(re.search(r"constexpr int ENC_QTILE = (\d+);", kern).group(1)) == 32
    assert int(re.search(r"constexpr int ENC_SLOTS_PER_ROUND = (\d+);", kern).group(1)) == 4
    squeeze = lambda s: re.sub(r"\s+", "", s)                                   # noqa: E731
    for host_text, plan_text in (
            ("const int lds_main = (H > 512 ? 16 : ENC_QTILE) * std::max(plan.max_round, H);",
             "return (H > 512 ? 16 : QTILE) * std::max(plan.max_round, H);"),
            ("const size_t lds_bytes = (size_t)(lds_main + 16 * ENC_QTILE) * sizeof(double);",
             "return (size_t)(lds_main_doubles(plan, H) + 16 * QTILE) * sizeof(double);"),
            ("const size_t lds = c->enc.lds_base + (size_t)ENC_QTILE * L * sizeof(double);",
             "return lds_bytes(plan, H) + (size_t)QTILE * L * sizeof(double);")):
        assert squeeze(host_text) in squeeze(host) and squeeze(plan_text) in squeeze(plan_src)
    assert host.count("> 160 * 1024") == 2
    for d in S.plans(plan_exe, [(S.N_CU, 64, H, 2, 1, 1, 300) for H in (512, 1024)]):
        print(f"L = 64, H = {d['H']}: {d['lds']} B of LDS, {d['lds_table']} B with the table")
        assert d["lds"] < d["lds_table"] <= 160 * 1024
        assert (d["n_slots"], d["n_rounds"], d["max_round"], d["kp0"]) == (33, 9, 512, 512)
    d40, = S.plans(plan_exe, [(S.N_CU, 40, 512, 2, 1, 1, 300)])
    assert (d40["n_slots"], d40["n_rounds"], d40["max_round"], d40["kp0"]) == (21, 6, 320, 200)


@pytest.mark.parametrize("case", list(S.TABLE))
def test_table_mode_near_the_equator(case):
    """The generated polynomials beyond L = 40, evaluated in numpy through the Siren: within |lat| <= 5 they equal the
    exact basis and move little when the latitude moves by one ulp - what lets the GPU test hold the kernel's table
    mode to 2e-12 there.  Both figures stay below 2e-13."""
    L, hidden, layers, mode, _ = S.CASES[case]
    t = S.table(L)
    assert int(np.max(t.p2)) == L - 1 <= 127 and int(np.max(t.cnt)) == L // 2 and int(np.max(t.kx)) < L
    q = np.array(S.equator_queries(S.TABLE_NEAR_EQUATOR))
    w = S.weights(case)
    e = O.encode(q, w, L, features=t.evaluate(q))
    exact = float(np.abs(e - O.encode(q, w, L, mode)).max())
    q1 = q.copy()
    q1[:, 1] = np.nextafter(q[:, 1], np.inf)
    moved = float(np.abs(O.encode(q1, w, L, features=t.evaluate(q1)) - e).max())
    print(f"{case}: {len(t.coef)} terms; |lat| <= 5: max |table - exact| = {exact:.2e}, one ulp of latitude moves it {moved:.2e}")
    assert exact < 2e-13 and moved < 2e-13
