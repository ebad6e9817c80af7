"""GPU tests of the CSP location encoder over its envelope (csp_kernel.h; range_set_csp, range_csp_encode[_grid]),
through the C ABI only: the networks of tests/csp_sweep_cases.py - all five activations at both tile heights,
1 to 8 column tiles a wave, widths that change from layer to layer, 1 to 9 layers, F = 1 and 64 - against the
numpy float64 restatement (tests/csp_refs.py) within 4 * max(E_ref, 2^-23 max|out|), E_ref from torch's float32
CPU operators over 1024 locations (csp_sweep_cases.bound; tests/test_csp_sweep_cpu.py shows each network tells
a planted defect from that bound); rows bit for bit across batch sizes and a capped grid; NaN rows followed by
clean tiles on the same workgroup; saturated activations; networks of very different size in turn on one engine.
Run with ``pytest -m gpu``."""
import numpy as np
import pytest

import csp_sweep_cases as S
from range_amd import _native
from test_gpu_csp import DEV, abi_call, dev, install

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    return _native.HipEngine(DEV)


def within_the_bound(engine, name, net, T):
    """Installs ``net``, encodes its GPU batch -> (the result, err / bound); prints the figures."""
    width, tile = install(engine, net)
    assert (width, tile) == (S.widths(net)[-1], T)
    q = S.batch(T)
    got = abi_call(engine, dev(q))
    want = S.restatement(net)[:len(q)]
    assert got.dtype == np.float32 and got.shape == want.shape == (2 * T + 3, width)
    err, bound = float(np.abs(got.astype(np.float64) - want).max()), S.bound(net)
    print(f"{name}: max|gpu - restatement| = {err:.3e}, E_ref = {S.e_ref(net):.3e}, bound = {bound:.3e}, "
          f"err / bound = {err / bound:.3f}")
    return got, err, bound


@pytest.mark.parametrize("case", list(S.SWEEP))
def test_sweep_within_the_bound(engine, case):
    got, err, bound = within_the_bound(engine, case, S.network(case), S.SWEEP[case]["T"])
    assert np.isfinite(got).all()
    assert err <= bound


@pytest.mark.parametrize("case", list(S.SWEEP))
def test_sweep_rows_bit_for_bit(engine, case):
    """Row i of every batch is row i of the 2T + 3 call, also where one workgroup walks all three tiles."""
    net, T = S.network(case), S.SWEEP[case]["T"]
    assert install(engine, net)[1] == T
    x = dev(S.batch(T))
    full = abi_call(engine, x)
    assert np.isfinite(full).all()
    for B in (1, T - 1, T, T + 1):
        assert np.array_equal(abi_call(engine, x[:B]), full[:B]), B
    assert np.array_equal(abi_call(engine, x, max_grid=1), full)
    for B in (1, T - 1, T, T + 1):
        assert np.array_equal(abi_call(engine, x[:B], max_grid=1), full[:B]), B


@pytest.mark.parametrize("max_grid", [1, 0])
@pytest.mark.parametrize("case", ["t32_leaky_mixed", "t64_mixed"])
def test_nan_rows_do_not_leak_across_tiles(engine, case, max_grid):
    """NaN and infinite coordinates in the first two tiles, a third tile behind them - with max_grid = 1 on the
    same workgroup's LDS rows: the three rows are NaN, every other row is the clean run's bit for bit."""
    net, T = S.network(case), S.SWEEP[case]["T"]
    assert install(engine, net)[1] == T
    B = 3 * T + 5
    q = S.queries()[:B].copy()
    clean = abi_call(engine, dev(q), max_grid=max_grid)
    assert np.isfinite(clean).all()
    bad = [0, T - 1, T + 2]
    q[0], q[T - 1], q[T + 2] = (np.nan, 10.0), (np.inf, 0.0), (20.0, -np.inf)
    got = abi_call(engine, dev(q), max_grid=max_grid)
    assert np.isnan(got[bad]).all()
    rest = np.setdiff1d(np.arange(B), bad)
    assert np.array_equal(got[rest], clean[rest])
    # and the tiles after a NaN tile on a workgroup that ran clean tiles only before: the clean run again
    q2 = S.queries()[:B].copy()
    assert np.array_equal(abi_call(engine, dev(q2), max_grid=max_grid), clean)


@pytest.mark.parametrize("act", S.SATURATED_ACTS)
def test_saturated_activations(engine, act):
    """Layer 0's pre-activations beyond +-88.8 (csp_sweep_cases.saturated asserts it): expf(-v) overflows, tanhf
    and erff are at their limits - the outputs stay finite and within the bound."""
    got, err, bound = within_the_bound(engine, "saturated_" + act, S.saturated(act), S.SATURATED[act]["T"])
    assert np.isfinite(got).all()
    assert err <= bound


def test_a_narrow_network_after_a_wide_one(engine):
    """One engine holds a 1024-wide network, the smallest one, a 1024-square one in turn (two tile heights, a
    1000-fold change in parameter size): each result is that of a fresh engine that only ever held that network."""
    for case in ("t32_relu_1024", "t64_w1", "t32_tanh_1024sq"):
        net, T = S.network(case), S.SWEEP[case]["T"]
        x = dev(S.batch(T))
        assert install(engine, net) == (S.widths(net)[-1], T)
        got = abi_call(engine, x)
        fresh = _native.HipEngine(DEV)
        assert install(fresh, net) == (S.widths(net)[-1], T)
        assert np.array_equal(abi_call(fresh, x), got), case
