"""Tunable retrieval temperatures on the GPU (`-m gpu`): ``model.args.temp`` / ``args.geo_temp`` are
live as in the reference (range.py:215, 234), the defaults stay bit for bit, and temperatures above
43 - where the constant shift m = tau log2(e) underflows as a whole - run pass 1 with a running
maximum (range_amd/csrc/pass1_sharp.h) and the unchanged pass 2.

Accuracy above 43 is judged per output element from the float64 sensitivity of the softmax to its
logits, not from a guessed constant:

    tol = 2e-5 + 4 (beta tau_sem d_sem S_sem + (1 - beta) tau_geo d_geo S_geo),
    S_h[q, c] = sum_i p_i |v_ic - o_c|   (float64; p, o: head h's weights and output),
    d_geo = 2^-22 (three float32 products), d_sem = the largest |topk_stream value - float64 similarity|
    over the queries' top 16 (topk_stream returns the float32 scan's logits bit for bit and is not the
    code under test); the factor 4 covers rows beyond the top 16, second order and pass 2's rounding.
"""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import range_oracle as O
from range_amd import _native
from tools import synth
from range_amd.bank import PreparedBank
from test_gpu_round6 import _antipodal_case, _dev, _engine, _params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L, H = 10, 64
ONE = 7                   # the value column that holds the constant 1
LOG2E = 1.4426950408889634
D_GEO = 2.0 ** -22
SHARP = [(100.0, 40.0), (12.0, 200.0), (1000.0, 1000.0)]
NO_KEEP = {"RANGE_KEEP_LOGITS": "0"}


def _soft(z):
    p = np.exp(z - z.max(axis=1, keepdims=True))
    return p / p.sum(axis=1, keepdims=True)


def _lse(z):
    m = z.max(axis=1)
    return m + np.log(np.exp(z - m[:, None]).sum(axis=1))


def _head(z, tau, V):
    """float64 weights' output and sensitivity S[q, c] = sum_i p_i |v_ic - o_c| of one head (torch
    float64 on the GPU: the N x 1024 differences of 70 queries take seconds on the CPU)."""
    zt, Vt = torch.from_numpy(z * tau).to(DEV), torch.from_numpy(V).to(DEV)
    p = torch.softmax(zt, dim=1)
    o = p @ Vt
    S = torch.stack([(p[q][:, None] * (Vt - o[q]).abs()).sum(0) for q in range(p.shape[0])])
    return o.cpu().numpy(), S.cpu().numpy()


class Case:
    """A bank (value column ONE = 1), 70 queries (smaller batches are their prefixes), the float64
    logits of the queries' e-hat, and engines over the bank."""

    def __init__(self, obank, qn, w, enc):
        self.obank, self.qn, self.w, self.enc = obank, qn, w, enc
        self.bank = PreparedBank(obank.keys, obank.values, obank.xyz)
        self.N = obank.keys.shape[0]
        self.V = obank.values.astype(np.float64)
        self.x = _dev(qn)
        self._eng, self._heads = {}, {}
        e64, e32, _ = self.engine().encode(self.x)
        self.e = e64.cpu().numpy()
        self.s, self.g = O.logits64(self.e, qn, obank)
        k = min(16, self.N)
        tv, ti = self.engine().topk_stream(e32, k)
        ti = ti.cpu().numpy()
        self.d_sem = float(np.abs(tv.cpu().numpy().astype(np.float64) - np.take_along_axis(self.s, ti, axis=1)).max())

    def engine(self, keep=True):
        if keep not in self._eng:
            self._eng[keep] = _engine(self.enc, self.bank, env=None if keep else NO_KEEP)
        return self._eng[keep]

    def head(self, which, tau):
        if (which, tau) not in self._heads:
            self._heads[which, tau] = _head(self.s if which == "sem" else self.g, tau, self.V)
        return self._heads[which, tau]

    def expect(self, ts, tg, beta, B):
        """float64 output (B, 1024) and the tolerance per element."""
        oh, Sh = self.head("sem", ts)
        if not tg:
            return oh[:B], 2e-5 + 4 * ts * self.d_sem * Sh[:B]
        og, Sg = self.head("geo", tg)
        return ((1 - beta) * og[:B] + beta * oh[:B],
                2e-5 + 4 * (beta * ts * self.d_sem * Sh[:B] + (1 - beta) * tg * D_GEO * Sg[:B]))

    def check(self, out, ts, tg, beta, what):
        """``out`` (B, 1280) against the float64 expectation; returns the largest err / tol."""
        B = out.shape[0]
        assert np.isfinite(out).all(), what
        ref, tol = self.expect(ts, tg, beta, B)
        ratio = float((np.abs(out[:, :1024] - ref) / tol).max())
        print(f"{what}: N={self.N} B={B} tau=({ts:g}, {tg:g}) beta={beta} d_sem={self.d_sem:.2e} max err/tol={ratio:.3f}")
        assert ratio <= 1.0, (what, ratio)
        return ratio


@functools.lru_cache(maxsize=None)
def _case(N, seed=77):
    w, enc = _params(L, H)
    locs, vals, keys = synth.make_bank(N, seed)
    vals = vals.copy()
    vals[:, ONE] = 1.0
    return Case(O.prep_bank(locs, vals, keys), synth.make_queries(70, seed=9, lat_max=90.0), w, enc)


def _files(tmp_path, N=1000):
    ck = synth.write_checkpoint(str(tmp_path / "e.ckpt"), L=L, hidden=H, seed=5)
    db = synth.write_bank(str(tmp_path / "db.npz"), N, 77)
    return ck, db


# ----------------------------------------------------------------------------------------------
# up to 43: the default kernels, live attributes
# ----------------------------------------------------------------------------------------------
def test_default_temperatures_bit_for_bit(tmp_path):
    from range_amd import load_model
    ck, db = _files(tmp_path)
    kw = dict(pretrained_path=ck, device=DEV, db_path=db)
    plus, plus_x = load_model("RANGE+", **kw), load_model("RANGE+", temp=12.0, geo_temp=40.0, **kw)
    rng_, rng_x = load_model("RANGE", **kw), load_model("RANGE", temp=15.0, **kw)
    assert (plus_x.args.temp, plus_x.args.geo_temp, rng_x.args.temp) == (12.0, 40.0, 15.0)
    assert (plus.args.temp, plus.args.geo_temp, rng_.args.temp) == (12.0, 40.0, 15.0)
    for B in (5, 40):
        q = _dev(synth.make_queries(B, seed=9, lat_max=90.0))
        assert np.array_equal(plus(q), plus_x(q)) and np.array_equal(rng_(q), rng_x(q))
        # C ABI: range_set_temperatures(0, 0) = the defaults; explicit defaults = the defaults
        ref = plus.engine.forward(q, _native.MODEL_RANGE_PLUS, 0.5).cpu().numpy()
        plus.engine.set_temperatures(25.0, 20.0)
        other = plus.engine.forward(q, _native.MODEL_RANGE_PLUS, 0.5).cpu().numpy()
        assert not np.array_equal(other[:, :1024], ref[:, :1024])
        plus.engine.set_temperatures(0.0, 0.0)
        assert np.array_equal(plus.engine.forward(q, _native.MODEL_RANGE_PLUS, 0.5).cpu().numpy(), ref)
        assert np.array_equal(plus(q), ref)


@pytest.mark.parametrize("B", [7, 20, 40])
def test_args_temp_and_geo_temp_are_live(B, tmp_path, monkeypatch):
    """B = 7 / 20: the one-pass route with one / two query tiles, 40: the two passes - all with
    non-default constants."""
    from range_amd import load_model
    ck, db = _files(tmp_path)
    kw = dict(pretrained_path=ck, device=DEV, db_path=db)
    qn = synth.make_queries(B, seed=9, lat_max=90.0)
    q = _dev(qn)
    m = load_model("RANGE+", **kw)
    base = m(q)
    m.args.temp = 25.0
    m.args.geo_temp = 20.0
    live = m(q)
    assert not np.array_equal(live[:, :1024], base[:, :1024])
    assert np.array_equal(live, load_model("RANGE+", temp=25, geo_temp=20, **kw)(q))
    assert np.array_equal(m(q, return_device=True).cpu().numpy(), live)
    sw = m.sweep(q, (0.5,))                  # (H and G apart, blended in float32: the same float64 bound)
    # the oracle at (25, 20): the project's bounds, unchanged (tau <= 43 keeps the error model)
    locs, vals, keys = synth.make_bank(1000, 77)
    obank = O.prep_bank(locs, vals, keys)
    e = live[:, 1024:]
    s, g = O.logits64(e, qn, obank)
    V = obank.values.astype(np.float64)
    want = 0.5 * (_soft(g * 20.0) @ V) + 0.5 * (_soft(s * 25.0) @ V)
    np.testing.assert_allclose(live[:, :1024], want, rtol=0, atol=2e-5)
    np.testing.assert_allclose(sw[0][:, :1024], want, rtol=0, atol=2e-5)
    monkeypatch.setattr(O, "TEMP_RANGE_PLUS", 25.0)
    monkeypatch.setattr(O, "TEMP_GEO", 20.0)
    np.testing.assert_allclose(live, O.retrieve(e, qn, obank, "RANGE+", 0.5), rtol=0, atol=1e-4)
    # RANGE: temp alone
    r = load_model("RANGE", **kw)
    rbase = r(q)
    r.args.temp = 25.0
    rl = r(q)
    np.testing.assert_allclose(rl[:, :1024], _soft(s * 25.0) @ V, rtol=0, atol=2e-5)
    monkeypatch.setattr(O, "TEMP_RANGE", 25.0)
    np.testing.assert_allclose(rl, O.retrieve(e, qn, obank, "RANGE", None), rtol=0, atol=1e-4)
    # back to the defaults: the default output, bit for bit
    m.args.temp, m.args.geo_temp, r.args.temp = 12.0, 40.0, 15.0
    assert np.array_equal(m(q), base) and np.array_equal(r(q), rbase)
    # outside (0, 1000]: the error names the limit
    m.args.temp = 1001.0
    with pytest.raises(ValueError, match="at most 1000"):
        m(q)
    m.args.temp = 12.0


# ----------------------------------------------------------------------------------------------
# above 43: the running-max pass 1
# ----------------------------------------------------------------------------------------------
RATIOS = {}


@pytest.mark.parametrize("N", [9, 1000, 20011])
@pytest.mark.parametrize("ts,tg", SHARP)
def test_sharp_routes(ts, tg, N):
    """Pad rows and lane groups without a row (N = 9), several splits (20 011); B = 1 and 20: the
    small-batch bypass (two passes: the one-pass kernel keeps the constant shift), pad queries; 70: two
    query tiles; pass 2 on kept logits and recomputing."""
    c = _case(N)
    worst = 0.0
    for keep in (True, False):
        eng = c.engine(keep)
        eng.set_temperatures(ts, tg)
        try:
            for B in (1, 20, 70):
                x = c.x[:B].contiguous()
                for model, t_geo, beta in ((_native.MODEL_RANGE, 0.0, 1.0), (_native.MODEL_RANGE_PLUS, tg, 0.0),
                                           (_native.MODEL_RANGE_PLUS, tg, 0.5), (_native.MODEL_RANGE_PLUS, tg, 1.0)):
                    out = eng.forward(x, model, beta).cpu().numpy()
                    if max(ts, t_geo) > 43.0 or B > 32:      # (two passes; RANGE at tau_sem = 12, B <= 32: the one-pass kernel)
                        assert eng.kept_queries() == (B if keep else 0)
                    worst = max(worst, c.check(out, ts, t_geo, beta, f"forward keep={keep}"))
                    # normalisation: the constant column comes back as 1 whatever tau (both passes use the same logits)
                    assert np.abs(out[:, ONE] - 1.0).max() <= 2e-5, (B, beta, np.abs(out[:, ONE] - 1.0).max())
                    assert np.array_equal(out[:, 1024:], c.e[:B])
                if keep:
                    host = eng.forward_host(x, _native.MODEL_RANGE_PLUS, 0.5)
                    assert np.array_equal(host, eng.forward(x, _native.MODEL_RANGE_PLUS, 0.5).cpu().numpy())
        finally:
            eng.set_temperatures(0.0, 0.0)
    RATIOS[ts, tg, N] = worst
    print(f"largest err/tol at tau=({ts:g}, {tg:g}), N={N}: {worst:.3f}")


def test_sharp_statistics_and_forced_splits():
    """(m + log2 l) / log2 e of scan_stats at (100, 200) against the float64 log-sum-exp, within tau d +
    1e-5; the same through three forced splits, whose kept logits then serve pass 2."""
    ts, tg = 100.0, 200.0
    for N in (9, 1000, 20011):
        c = _case(N)
        eng = c.engine()
        e64, e32, xq = eng.encode(c.x)
        want = np.stack([_lse(c.s * ts), _lse(c.g * tg)], axis=1)
        tol = np.array([ts * c.d_sem + 1e-5, tg * D_GEO + 1e-5])
        runs = [("plain", eng.scan_stats(e32, xq, ts, tg, keep_logits=True))]
        if N == 1000:
            runs.append(("three splits", eng.scan_stats_at(e32, xq, ts, tg, 0, 70, n_splits=3)))
        for what, st_dev in runs:
            st = st_dev.cpu().numpy().astype(np.float64)
            got = np.stack([(st[:, 0] + np.log2(st[:, 1])) / LOG2E, (st[:, 2] + np.log2(st[:, 3])) / LOG2E], axis=1)
            err = np.abs(got - want).max(axis=0)
            print(f"statistics {what}: N={N} err (sem, geo) = {err}, tol = {tol}")
            assert (err <= tol).all(), (what, N, err, tol)
            # m is the largest scaled logit (to float32 rounding of k and the product)
            np.testing.assert_allclose(st[:, 0], (c.s * ts).max(axis=1) * LOG2E, rtol=0, atol=ts * LOG2E * (c.d_sem + 3e-7))
            assert eng.kept_queries() == 70
            out = eng.finalize(eng.attend_kept(0, xq, ts, tg, 0.5, st_dev), e64).cpu().numpy()
            c.check(out, ts, tg, 0.5, f"attend_kept after {what}")
            assert np.abs(out[:, ONE] - 1.0).max() <= 2e-5
        # RANGE: no geographic head -> {., ., NEG_BIG, 0}
        st = eng.scan_stats(e32, xq, ts, 0.0).cpu().numpy()
        assert (st[:, 2] == np.float32(-1e30)).all() and (st[:, 3] == 0).all()


def test_sweep_and_load_model_at_sharp_temperatures(tmp_path):
    from range_amd import load_model
    c = _case(1000)
    ck = synth.write_checkpoint(str(tmp_path / "e.ckpt"), L=L, hidden=H, seed=5)
    db = str(tmp_path / "db.npz")
    locs, vals, keys = synth.make_bank(1000, 77)
    vals[:, ONE] = 1.0
    np.savez(db, locs=locs, image_embeddings=vals, satclip_embeddings=keys)
    m = load_model("RANGE+", pretrained_path=ck, device=DEV, db_path=db, temp=100.0, geo_temp=200.0)
    betas = (0.0, 0.5, 1.0)
    sw = m.sweep(c.x, betas)
    for j, b in enumerate(betas):
        c.check(sw[j], 100.0, 200.0, b, "sweep")
        assert np.abs(sw[j][:, ONE] - 1.0).max() <= 2e-5
    for B in (20, 70):
        out = m(c.x[:B].contiguous())
        c.check(out, 100.0, 200.0, 0.5, "load_model(temp=100, geo_temp=200)")
    # live, across the threshold and back
    m.args.temp, m.args.geo_temp = 12.0, 40.0
    d = load_model("RANGE+", pretrained_path=ck, device=DEV, db_path=db)
    assert np.array_equal(m(c.x), d(c.x))
    d.args.geo_temp = 1000.0
    c.check(d(c.x), 12.0, 1000.0, 0.5, "args.geo_temp = 1000")


# ----------------------------------------------------------------------------------------------
# extremes
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 16, 10_000])
def test_antipodal_bank_at_tau_1000(N):
    """Every geographic logit ~ -1 and query 0's semantic ones too: the constant shift would give terms
    of 2^-2885 - 0 / 0."""
    enc, obank, qn, w = _antipodal_case(N, 40)
    c = Case(obank, qn, w, enc)
    eng = c.engine()
    eng.set_temperatures(1000.0, 1000.0)
    for B in (7, 40):
        for model, tg, beta in ((_native.MODEL_RANGE, 0.0, 1.0), (_native.MODEL_RANGE_PLUS, 1000.0, 0.0),
                                (_native.MODEL_RANGE_PLUS, 1000.0, 0.5)):
            c.check(eng.forward(c.x[:B].contiguous(), model, beta).cpu().numpy(), 1000.0, tg, beta, "antipodal")


def _planted_case(N, B, row):
    rng = np.random.default_rng(3)
    w, enc = _params(L, H)
    qn = np.stack([-150.0 + rng.uniform(-0.25, 0.25, B), -20.0 + rng.uniform(-0.25, 0.25, B)], axis=1)
    e0 = O.encode(qn[:1], w, L)[0]
    locs = np.stack([30.0 + rng.uniform(-0.5, 0.5, N), 20.0 + rng.uniform(-0.5, 0.5, N)], axis=1)
    keys = -e0[None, :] + 0.01 * rng.standard_normal((N, 256))
    locs[row] = qn[0]
    keys[row] = e0
    vals = rng.standard_normal((N, 1024)).astype(np.float32)
    return enc, O.prep_bank(locs, vals, keys), qn, vals


@pytest.mark.parametrize("ts,tg", [(100.0, 200.0), (1000.0, 1000.0)])
def test_one_planted_row_in_the_last_of_three_splits(ts, tg):
    """Query 0: one row at similarity +1 (its own e-hat and location) among rows at -1, in the last
    split of three: the first two splits' m are 2 tau log2(e) below the third's."""
    N, B, row = 1000, 40, 901
    enc, obank, qn, vals = _planted_case(N, B, row)
    eng = _engine(enc, PreparedBank(obank.keys, obank.values, obank.xyz))
    e64, e32, xq = eng.encode(_dev(qn))
    st = eng.scan_stats_at(e32, xq, ts, tg, 0, B, n_splits=3)
    m = st.cpu().numpy()[0]
    assert abs(m[0] - ts * LOG2E) < 1e-3 * ts and abs(m[2] - tg * LOG2E) < 1e-3 * tg
    for beta in (0.0, 0.5, 1.0):
        out = eng.finalize(eng.attend_kept(0, xq, ts, tg, beta, st), e64).cpu().numpy()
        assert np.isfinite(out).all()
        np.testing.assert_allclose(out[0, :1024], vals[row], rtol=0, atol=2e-5)
    eng.set_temperatures(ts, tg)
    for beta in (0.0, 0.5, 1.0):
        out = eng.forward(_dev(qn), _native.MODEL_RANGE_PLUS, beta).cpu().numpy()
        np.testing.assert_allclose(out[0, :1024], vals[row], rtol=0, atol=2e-5)
    np.testing.assert_allclose(eng.forward(_dev(qn[:5]), _native.MODEL_RANGE, 1.0).cpu().numpy()[0, :1024], vals[row], rtol=0, atol=2e-5)


def test_nan_and_infinite_coordinates_at_tau_100():
    c = _case(1000)
    eng = c.engine()
    eng.set_temperatures(100.0, 0.0)
    try:
        good = c.qn[:40].copy()
        bad = good.copy()
        bad[3] = [np.nan, 10.0]
        bad[17] = [10.0, np.inf]
        for model in (_native.MODEL_RANGE_PLUS, _native.MODEL_RANGE):
            ref = eng.forward(_dev(good), model, 0.5).cpu().numpy()
            out = eng.forward(_dev(bad), model, 0.5).cpu().numpy()
            eng.check_async_error()
            isnan = np.isnan(out).all(axis=1)
            assert np.array_equal(np.flatnonzero(isnan), [3, 17]) and not np.isnan(out[~isnan]).any()
            assert np.array_equal(out[~isnan], ref[~isnan])          # the neighbours: bit for bit
        # the statistics of a NaN query are NaN (fmaxf drops it from m; the exp2 terms keep it in l)
        _, e32, xq = eng.encode(_dev(bad))
        st = eng.scan_stats(e32, xq, 100.0, 200.0).cpu().numpy()
        assert np.isnan(st[3, 1]) and np.isnan(st[3, 3]) and np.isnan(st[17, 1]) and np.isnan(st[17, 3])
        assert np.isfinite(np.delete(st, [3, 17], axis=0)).all()
    finally:
        eng.set_temperatures(0.0, 0.0)


# ----------------------------------------------------------------------------------------------
# two shards at engine level
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planted", [False, True])
def test_two_shards_at_engine_level(planted):
    """Half the bank each, scan_stats_at -> merge_stats -> attend -> finalize against the single engine
    within the project's shard bound; ``planted``: the one row at +1 sits in shard 1 only, so the two
    shards' m differ by hundreds."""
    ts, tg, N, B = 100.0, 200.0, 1000, 40
    if planted:
        enc, obank, qn, vals = _planted_case(N, B, 901)
    else:
        c = _case(N)
        enc, obank, qn = c.enc, c.obank, c.qn[:B]
    bank = PreparedBank(obank.keys, obank.values, obank.xyz)
    cut = N // 2
    full, a, b = _engine(enc, bank), _engine(enc, bank.rows(0, cut), 0), _engine(enc, bank.rows(cut, N), cut)
    e64, e32, xq = full.encode(_dev(qn))
    full.set_temperatures(ts, tg)
    for beta in (0.0, 0.5, 1.0):
        parts = torch.stack([a.scan_stats_at(e32, xq, ts, tg, 0, B), b.scan_stats_at(e32, xq, ts, tg, 0, B)])
        st = full.merge_stats(parts)
        if planted:
            p = parts.cpu().numpy()
            assert p[1, 0, 0] - p[0, 0, 0] > 1.9 * ts * LOG2E and p[1, 0, 2] - p[0, 0, 2] > 1.9 * tg * LOG2E
        two = full.finalize(torch.stack([a.attend_kept(0, xq, ts, tg, beta, st), b.attend_kept(0, xq, ts, tg, beta, st)]), e64).cpu().numpy()
        one = full.forward(_dev(qn), _native.MODEL_RANGE_PLUS, beta).cpu().numpy()
        assert np.isfinite(two).all()
        np.testing.assert_allclose(two, one, rtol=0, atol=2e-6)
        if planted:
            np.testing.assert_allclose(two[0, :1024], vals[901], rtol=0, atol=2e-5)


# ----------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------
def test_refusals():
    c = _case(1000)
    _, e32, xq = c.engine().encode(c.x)
    with pytest.raises(_native.RangeNativeError, match="range_topk_stream"):
        c.engine(False).scan_stats(e32, xq, 100.0, 40.0, topk=4)
    # (a context that keeps its logits takes the top-k from them, at any temperature)
    _, tv, ti = c.engine().scan_stats(e32, xq, 100.0, 40.0, topk=4)
    np.testing.assert_allclose(tv.cpu().numpy(), np.sort(c.s, axis=1)[:, ::-1][:, :4], rtol=0, atol=1e-6)
    for bad in (1001.0, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_native.RangeNativeError, match="at most 1000"):
            c.engine().scan_stats(e32, xq, bad, 40.0)
        if bad != 0.0:
            with pytest.raises(_native.RangeNativeError, match="at most 1000"):
                c.engine().set_temperatures(bad, 0.0)
    with pytest.raises(_native.RangeNativeError, match="at most 1000"):
        c.engine().scan_stats(e32, xq, 12.0, 1001.0)
    with pytest.raises(_native.RangeNativeError, match="at most 1000"):
        c.engine().attend(e32, xq, 12.0, 1001.0, 0.5, torch.ones((70, 4), device=DEV))
