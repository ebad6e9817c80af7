"""The host side of the context-lifecycle tests (tests/lifecycle.py): every setter of the public headers has a
test that replaces what it installed, the exactness premise of every tuple the GPU files compare bit for bit, the
poison's properties - without them the GPU tests would prove nothing - and a planted stale row that the emulator
must show for every poison kind."""
import os
import re

import numpy as np
import pytest

import exact_dense_cases as D
import lifecycle as L
from tools import exact_bank as X

HERE = os.path.dirname(os.path.abspath(__file__))


# -- setter coverage ---------------------------------------------------------------------------------------------
def test_the_parser_finds_the_known_setters():
    found = L.setter_entry_points()
    assert set(found) == set(L.HEADERS)
    names = [n for v in found.values() for n in v]
    assert len(names) == len(set(names))
    for known in ("range_set_encoder", "range_set_sh_table", "range_set_bank", "range_set_keys", "range_set_pv_mode",
                  "range_set_temperatures", "range_set_csp", "range_set_csp_head"):
        assert known in found["range_hip.h"], known
    assert found["range_neighbors.h"] == ["range_set_neighbors", "range_set_kde_points"]
    assert found["range_map.h"] == ["range_map_reserve"] and found["range_cluster.h"] == ["range_cluster_reserve"]


def test_every_setter_has_a_lifecycle_case():
    """A new ``range_set_*`` / ``range_*_reserve`` without a test that calls it on a context which already holds an
    earlier installation fails here."""
    names = [n for v in L.setter_entry_points().values() for n in v]
    missing = [n for n in names if n not in L.SETTER_CASES]
    assert not missing, f"setters without a lifecycle case (tests/lifecycle.py: SETTER_CASES): {missing}"
    stale = [n for n in L.SETTER_CASES if n not in names]
    assert not stale, f"SETTER_CASES names entry points no header declares: {stale}"
    for name, (module, test) in L.SETTER_CASES.items():
        with open(os.path.join(HERE, module + ".py")) as f:
            text = f.read()
        assert re.search(rf"^def {test}\(", text, flags=re.M), f"{name}: {module}.{test} does not exist"
        assert "pytest.mark.gpu" in text


# -- the exactness premise -----------------------------------------------------------------------------------------
def _premise_ids():
    return [p[0] for p in list(L.premises()) + list(L.model_premises())]


@pytest.mark.parametrize("what", sorted(set(w.split(" B=")[0] for w in _premise_ids())))
def test_exactness_premise(what):
    """assert_bank_margin for every (bank, queries, beta, temperatures) of the GPU files; the walk's queries ask for
    every class of their bank."""
    hit = 0
    for name, bank, q, beta, ts, tg, stats_only in list(L.premises()) + list(L.model_premises()):
        if name.split(" B=")[0] != what:
            continue
        hit += 1
        X.assert_bank_margin(bank, q, beta, ts, tg, stats_only=stats_only)
        if not stats_only:
            want = X.expect(bank, q, beta, tg > 0)
            assert want.shape == (len(q.sem), X.VAL_DIM) and np.isfinite(want).all()
        if name.startswith("routes"):
            assert X.covered(bank, q)
            wv, wi = X.topk_expect(bank, q, L.topk_k(bank.n))
            assert wi.max() < bank.n
    assert hit


def test_the_workspace_calls_ask_for_disjoint_classes():
    big, small = L.ws_classes(True), L.ws_classes(False)
    assert len(big) and len(small) and not set(big) & set(small)
    for B in L.WS_SMALL_B + (L.WS_MID_B,):
        assert not set(L.ws_queries(B, False).sem) & set(L.ws_queries(L.WS_BIG_B, True).sem)


@pytest.mark.parametrize("name,B,beta", [("n108", 17, 0.25), ("n4099", 65, 0.75)])
def test_dense_premise(name, B, beta):
    bank = D.bank(name)
    assert beta in D.betas(name)
    q = X.queries(bank, B, seed=B, perturb=D.perturbed(name))
    X.assert_bank_margin(bank, q, beta, X.dense_tau(48), X.dense_tau(48))


def test_dense_temperature_premise():
    for name, tau, beta in L.DENSE_TEMPS:
        bank, c = D.bank(name), L.dense_forward_class(name)
        assert beta in D.betas(name) and bank.sem_size[c] > 1 and bank.grade[bank.sem == c].max() > 0
        for B in L.DENSE_TEMPS_B:
            q = X.forward_queries(bank, c, B, B)
            X.assert_bank_margin(bank, q, beta, tau, tau)
            X.expect(bank, q, beta)


# -- the poison ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", L.KINDS)
def test_poison_bank(kind):
    keys, values, xyz = L.poison_bank(L.PRED_N, kind)
    assert keys.dtype == values.dtype == xyz.dtype == np.float32
    assert keys.shape == (L.PRED_N, X.KEY_DIM) and values.shape == (L.PRED_N, X.VAL_DIM) and xyz.shape == (L.PRED_N, 3)
    assert np.array_equal((keys.astype(np.float64) ** 2).sum(1), np.ones(L.PRED_N))
    assert np.array_equal((xyz.astype(np.float64) ** 2).sum(1), np.ones(L.PRED_N))
    if kind == "huge":
        assert np.array_equal(np.abs(values), np.full_like(values, L.FLT_MAX))
        assert (np.sign(values[:, 0]) != np.sign(values[:, 1])).all()
    elif kind == "one":
        assert (values == 3.0).all()
    else:
        assert np.isnan(values).all()


@pytest.mark.parametrize("n", L.SUCCESSORS)
def test_every_query_meets_poison_behind_the_padding(n):
    """Behind the successor's padded rows the allocation still holds poison rows at similarity exactly 1 with every
    query, in both heads - and in every 512-row stretch, whatever tile a kernel might over-read."""
    keys, _, xyz = L.poison_bank(L.PRED_N, "one")
    for q in (L.route_queries(n), L.forward_queries(n, 33)):
        lo = L.n_pad(n)
        for hi in (lo + X.N_DIRS, L.PRED_N):
            s = q.e32.astype(np.float64) @ keys[lo:hi].astype(np.float64).T
            g = q.xq[:, :3].astype(np.float64) @ xyz[lo:hi].astype(np.float64).T
            assert ((s == 1.0).sum(1) >= 1).all() and ((g == 1.0).sum(1) >= 1).all()


# -- a planted defect ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,B", [(1, 2), (17, 4), (4099, 2)])
@pytest.mark.parametrize("kind", L.KINDS)
def test_one_stale_row_changes_the_result(kind, n, B):
    """The float32 pipeline over the successor's rows gives the expectation; with ONE row of the poisoned predecessor
    from behind the padding admitted it does not - for every kind, in the statistics and in the output."""
    bank = L.exact(n)
    q0 = L.route_queries(n)
    q = X.Queries(q0.sem[:B], q0.geo[:B], q0.e32[:B], q0.xq[:B])
    want, want_st = X.expect(bank, q, L.BETA), X.expect_stats(bank, q, L.TAU, L.TAU)
    st, out = X.emulate(bank, q, L.BETA, L.TAU, L.TAU, seed=1, parts=3)
    assert np.array_equal(out, want) and np.array_equal(st, want_st)
    keys, _, _ = L.poison_bank(L.PRED_N, kind)
    s = q.e32[:1].astype(np.float64) @ keys.astype(np.float64).T
    row = L.n_pad(n) + int(np.flatnonzero(s[0, L.n_pad(n):] == 1.0)[0])
    st, out = X.emulate(L.with_stale_rows(bank, kind, [row]), q, L.BETA, L.TAU, L.TAU, seed=1, parts=3)
    hit = q.sem == q.sem[0]
    assert (st[hit, 1] == want_st[hit, 1] + 1).all(), "the stale row is missing from l_sem"
    assert (out[hit] != want[hit]).any(axis=1).all(), f"a stale {kind} row left the output alone"
