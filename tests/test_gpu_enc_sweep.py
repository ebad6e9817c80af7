"""GPU tests of the SatCLIP location encoder over its envelope (encoder_kernel.h; range_set_encoder,
range_set_sh_table, range_encode, range_encode_raw, range_forward), through _native.HipEngine only: the cases of
tests/enc_sweep_cases.py - L = 41 .. 64, 1 to 7 hidden layers, every kernel width in every launch form, 32-query
workgroups at every width that has them - against the float64 oracle within the project's bound (2e-12; 4e-12 beyond
512 columns), which tests/test_enc_sweep_cpu.py holds to a tenth of that against long double and shows to tell seven
planted defects apart; two fixtures the reference's closed form produced beyond L = 40; the three launch routes
against each other; NaN rows at the edges of tiles and workgroups; the reference's generated polynomials beyond
L = 40; networks of very different size in turn on one engine; the whole forward at L = 64.
Run with ``pytest -m gpu``."""
import os

import numpy as np
import pytest
import torch

import enc_sweep_cases as S
from oracle import range_oracle as O
from range_amd import _native
from range_amd.bank import prepare_bank
from tools import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.tensor(np.asarray(a), device=DEV)          # (a copy: the shared rows are read-only)


def sh_mode(mode):
    return _native.SH_ANALYTIC if mode == "analytic" else _native.SH_CLOSED_FORM


def install(eng, name, table=None):
    L, hidden, layers, mode, _ = S.CASES[name]
    ws, bs = S.weight_lists(S.weights(name))
    eng.set_encoder(L, hidden, layers, 256, sh_mode(mode), ws, bs, sh_table=table)
    return eng


def engine_of(name, table=None):
    return install(_native.HipEngine(DEV), name, table)


def encode(eng, q):
    e64, e32, xq = eng.encode(dev(q))
    return e64.cpu().numpy(), e32.cpu().numpy(), xq.cpu().numpy()


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return S.build_plan_program(tmp_path_factory.mktemp("enc_sweep_plan"))


@pytest.fixture(scope="module")
def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def plan_line(d):
    return (f"B={d['B']} split={d['split']} fused={d['fused']}: main {d['main_B']} ({d['n_wg32']} x 32 of {d['grid']}), split "
            f"{d['split_B']} (tiles {d['tiles']}, S {d['S']} x KP {d['KP']}, one_launch {d['one_launch']}, S2 {d['S2']}, "
            f"parts {d['part_cols']} / {d['part2_cols']}) -> {sorted(d['tables'])}")


def check_against_the_oracle(eng, name, B, want=None):
    """One batch of a case: e64 within the bound, e32 its rounding, xq, unit norm, the raw output, a second call
    bit for bit.  -> (e64, e32, xq, err)."""
    q = S.queries(B)
    want = S.oracle(name, B) if want is None else want
    e64, e32, xq = encode(eng, q)
    assert e64.shape == (B, 256) and e64.dtype == np.float64 and e32.dtype == np.float32 and xq.shape == (B, 4)
    err = float(np.abs(e64 - want).max())
    print(f"{name} B={B}: max |gpu - oracle| = {err:.3e}, err / bound = {err / S.bound(name):.3f}")
    assert err <= S.bound(name)
    assert np.array_equal(e32, e64.astype(np.float32))
    assert np.abs(xq[:, :3] - O.query_xyz(q)).max() <= 1.2e-7 and np.all(xq[:, 3] == 0)
    assert np.abs(np.linalg.norm(e64, axis=1) - 1.0).max() < 1e-13
    raw = eng.encode_raw(dev(q)).cpu().numpy()
    assert np.abs(raw / np.linalg.norm(raw, axis=1, keepdims=True) - e64).max() < 1e-13
    again = encode(eng, q)
    assert np.array_equal(again[0], e64) and np.array_equal(again[1], e32) and np.array_equal(again[2], xq)
    return e64, e32, xq, err


@pytest.mark.parametrize("case", list(S.SWEEP))
def test_sweep_against_the_oracle(case, plan_exe, n_cu):
    L, hidden, layers, mode, batches = S.CASES[case]
    eng = engine_of(case)
    worst = 0.0
    for B, d in zip(batches, S.plans(plan_exe, [(n_cu, L, hidden, layers, 1, 1, B) for B in batches])):
        print(f"{case} on {n_cu} CUs: {plan_line(d)}")
        worst = max(worst, check_against_the_oracle(eng, case, B)[3])
    print(f"{case}: largest err / bound = {worst / S.bound(case):.3f}")


@pytest.mark.parametrize("tag", list(S.E_GOLDEN))
def test_reference_fixtures_beyond_L40(tag):
    """The reference's own closed form + SirenNet: the kernel within 4 x (the oracle's recorded distance to the
    reference) + the kernel's bound against the oracle."""
    z = np.load(os.path.join(S.GOLDEN, tag + ".npz"))
    L, hidden, layers, mode = int(z["L"]), int(z["hidden"]), int(z["num_hidden_layers"]), str(z["mode"])
    w = synth.make_encoder_weights(L, hidden, 256, layers, int(z["seed"]))
    ws, bs = S.weight_lists(w)
    eng = _native.HipEngine(DEV)
    eng.set_encoder(L, hidden, layers, 256, sh_mode(mode), ws, bs)
    ref = z["embedding"] / np.linalg.norm(z["embedding"], axis=1, keepdims=True)
    e64 = encode(eng, z["lonlat"])[0]
    err, bound = float(np.abs(e64 - ref).max()), 4 * S.E_GOLDEN[tag] + 2e-12
    print(f"{tag}: max |gpu - reference| = {err:.3e}, bound = {bound:.3e}, err / bound = {err / bound:.3f}")
    assert err <= bound


@pytest.mark.parametrize("case", list(S.ROUTES))
def test_three_launch_routes(case, monkeypatch, plan_exe, n_cu):
    """The default engine, RANGE_ENC_SPLIT=0 (the one-kernel encoder) and RANGE_ENC_FUSED=0 (the split as separate
    launches): each within the bound of the oracle, pairwise within 5e-13, xq bit-equal."""
    L, hidden, layers, mode, _ = S.CASES[case]
    engines = {"default": engine_of(case)}
    for key, var in (("split=0", "RANGE_ENC_SPLIT"), ("fused=0", "RANGE_ENC_FUSED")):
        monkeypatch.setenv(var, "0")
        engines[key] = _native.HipEngine(DEV)
        monkeypatch.delenv(var)
        install(engines[key], case)
    switches = {"default": (1, 1), "split=0": (0, 1), "fused=0": (1, 0)}
    for B in S.ROUTE_BATCHES:
        q, want, got = S.queries(B), S.oracle(case, B), {}
        for (key, eng), d in zip(engines.items(), S.plans(plan_exe, [(n_cu, L, hidden, layers, *switches[k], B) for k in engines])):
            e64, e32, xq = encode(eng, q)
            err = float(np.abs(e64 - want).max())
            print(f"{case} {key} on {n_cu} CUs: {plan_line(d)}: err / bound = {err / S.bound(case):.3f}")
            assert err <= S.bound(case), key
            assert np.array_equal(e32, e64.astype(np.float32)), key
            got[key] = (e64, xq)
        keys = list(got)
        for i, a in enumerate(keys):
            for b in keys[i + 1:]:
                assert np.abs(got[a][0] - got[b][0]).max() < 5e-13, (a, b, B)
                assert np.array_equal(got[a][1], got[b][1]), (a, b, B)


@pytest.mark.parametrize("case", list(S.WG32))
def test_32_query_workgroups_on_every_width(case, plan_exe, n_cu):
    """Batches whose main launch holds 32-query workgroups: against the oracle; then NaN and infinite coordinates at
    the edges of a 16-query tile, a 32-query workgroup and the change of workgroup size - those rows NaN, every other
    row of all three outputs the clean call's bit for bit."""
    L, hidden, layers, mode, batches = S.CASES[case]
    eng = engine_of(case)
    for B, d in zip(batches, S.plans(plan_exe, [(n_cu, L, hidden, layers, 1, 1, B) for B in batches])):
        print(f"{case} on {n_cu} CUs: {plan_line(d)}")
        n32 = d["n_wg32"]
        assert n32 > 0 or n_cu != S.N_CU, "the batch is chosen for 32-query workgroups on 256 CUs"
        e64, e32, xq, _ = check_against_the_oracle(eng, case, B)
        bad = sorted({r for r in (0, 15, 16, 31, 32, 32 * n32 - 1, 32 * n32, B - 1) if 0 <= r < B})
        q = np.array(S.queries(B))
        for i, r in enumerate(bad):
            q[r] = [(np.nan, 10.0), (np.inf, 0.0), (20.0, -np.inf), (20.0, np.nan)][i % 4]
        g64, g32, gxq = encode(eng, q)
        assert np.isnan(g64[bad]).all() and np.isnan(g32[bad]).all()
        rest = np.setdiff1d(np.arange(B), bad)
        assert np.array_equal(g64[rest], e64[rest]) and np.array_equal(g32[rest], e32[rest]) and np.array_equal(gxq[rest], xq[rest])
        # and clean again behind the NaN batch
        assert np.array_equal(encode(eng, S.queries(B))[0], e64)


def set_table_through_the_abi(eng, L, t):
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)   # noqa: E731
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)     # noqa: E731
    arrs = [f64(t.front), f64(t.a0), f64(t.a2), i32(t.p2), i32(t.kx), i32(t.off), i32(t.cnt)]
    coef, powr = f64(t.coef), i32(t.pow)
    _native._check(eng.lib, eng.lib.range_set_sh_table(eng._h, L, *[a.ctypes.data for a in arrs], coef.shape[0],
                                                       coef.ctypes.data, powr.ctypes.data))


@pytest.mark.parametrize("case", list(S.TABLE))
def test_table_mode_beyond_L40(case):
    """The reference's generated polynomials at L = 48 and 64 (p2 up to 63, 32 terms a function, a 64-entry power
    table a query): within |lat| <= 5, where their numpy evaluation equals the exact basis to 2e-15, the kernel within
    2e-12 of that evaluation through the Siren; pole to pole, where the polynomials mean nothing by the reference's own
    design, finite and of unit norm; and back to the exact basis once the encoder is set without a table."""
    L, hidden, layers, mode, _ = S.CASES[case]
    t, w = S.table(L), S.weights(case)
    eng = engine_of(case, table=t)
    q = np.array(S.equator_queries(S.TABLE_NEAR_EQUATOR))
    e64, e32, xq = encode(eng, q)
    want = O.encode(q, w, L, features=t.evaluate(q))
    err = float(np.abs(e64 - want).max())
    print(f"{case}: |lat| <= 5: max |gpu - table in numpy| = {err:.3e} (err / 2e-12 = {err / 2e-12:.3f}), "
          f"max |gpu - exact basis| = {np.abs(e64 - O.encode(q, w, L, mode)).max():.3e}")
    assert err <= 2e-12
    assert np.array_equal(e32, e64.astype(np.float32))
    qp = S.queries(S.TABLE_POLE_TO_POLE)
    p64, p32, pxq = encode(eng, qp)
    assert np.isfinite(p64).all() and np.isfinite(p32).all() and np.isfinite(pxq).all()
    assert np.abs(np.linalg.norm(p64, axis=1) - 1.0).max() < 1e-13
    if L == 64:
        # a table of another degree is refused, and nothing changes
        with pytest.raises(_native.RangeNativeError, match="table for L=48"):
            set_table_through_the_abi(eng, 48, S.table(48))
        assert np.array_equal(encode(eng, q)[0], e64) and np.array_equal(encode(eng, qp)[0], p64)
    install(eng, case)                   # no table: the exact recurrence
    back = encode(eng, qp)[0]
    err = float(np.abs(back - S.oracle(case, S.TABLE_POLE_TO_POLE)).max())
    print(f"{case}: without the table again: err / bound = {err / S.bound(case):.3f}")
    assert err <= 2e-12


def test_deep_and_shallow_nets_in_turn():
    """One engine holds (64, 1024, 2), (10, 64, 7), (64, 256, 7) and (41, 64, 1) in turn: each result is that of a
    fresh engine that only ever held that network.  8 hidden layers are refused, and the network before still answers."""
    eng = _native.HipEngine(DEV)
    for case in S.IN_TURN:
        B = S.CASES[case][4][1]
        q = S.queries(B)
        got = encode(install(eng, case), q)
        assert np.abs(got[0] - S.oracle(case, B)).max() <= S.bound(case), case
        fresh = encode(engine_of(case), q)
        assert all(np.array_equal(a, b) for a, b in zip(got, fresh)), case
    L, hidden = 10, 64
    w8 = synth.make_encoder_weights(L, hidden, 256, 8, 3)
    ws, bs = S.weight_lists(w8)
    assert len(ws) == 9
    with pytest.raises(_native.RangeNativeError, match="num_hidden_layers 8 unsupported"):
        eng.set_encoder(L, hidden, 8, 256, _native.SH_ANALYTIC, ws, bs)
    assert all(np.array_equal(a, b) for a, b in zip(encode(eng, q), got))


def test_forward_at_L64():
    """range_forward behind an L = 64 encoder: its embedding half is range_encode's e64 bit for bit, its retrieval half
    within the project's 2e-5 of the float64 retrieval from that e-hat."""
    case = S.FORWARD_CASE
    assert S.CASES[case][0] == 64
    locs, vals, keys = synth.make_bank(S.FORWARD_BANK_ROWS, 64)
    bank, obank = prepare_bank(locs, vals, keys), O.prep_bank(locs, vals, keys)
    eng = engine_of(case)
    eng.set_bank(bank.keys, bank.values, bank.xyz)
    for B in S.FORWARD_BATCHES:
        q = S.queries(B, seed=1)
        out = eng.forward(dev(q), _native.MODEL_RANGE_PLUS, 0.5).cpu().numpy()
        e64 = encode(eng, q)[0]
        assert out.shape == (B, 1280) and np.array_equal(out[:, 1024:], e64)
        assert np.abs(e64 - O.encode(q, S.weights(case), 64, S.CASES[case][3])).max() <= S.bound(case)
        err = float(np.abs(out[:, :1024] - O.retrieve64(e64, q, obank, "RANGE+", 0.5)).max())
        print(f"forward at L = 64, B = {B}: retrieval half max err = {err:.3e}")
        assert err <= 2e-5
