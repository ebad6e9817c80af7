"""Temperature sweeps from one scan (`-m gpu`): ``Engine.stats_kept`` - pass 1's softmax statistics at
other temperatures from the logits a scan kept (range_amd/csrc/pass1_kept.h), bit for bit what
``scan_stats`` / ``scan_stats_at`` gives - and ``sweep(coords, betas, temps=, geo_temps=)`` on top of it.

The yardstick of the statistics is a second engine created with RANGE_KEEP_LOGITS=0: same bank, same
splits, and the scanning engine's kept state is not disturbed."""
import numpy as np
import pytest
import torch

from range_amd import _native
from tools import synth
from range_amd.bank import PreparedBank
from test_gpu_round6 import _dev, _engine
from test_gpu_temperatures import DEV, L, H, NO_KEEP, ONE, SHARP, Case, _case, _planted_case

pytestmark = pytest.mark.gpu
# constant shift, the cap, running maximum by either head, the extreme, no geographic head
PAIRS = [(12.0, 40.0), (25.0, 20.0), (43.0, 43.0), (100.0, 40.0), (12.0, 200.0), (1000.0, 1000.0), (15.0, 0.0)]
assert set(SHARP) <= set(PAIRS)


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    bad = np.argwhere(g != w)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), got.cpu().numpy()[tuple(bad[0])], want.cpu().numpy()[tuple(bad[0])])


@pytest.mark.parametrize("N,scan_at", [(9, (12.0, 40.0)), (1000, (12.0, 40.0)), (20011, (12.0, 40.0)), (1000, (100.0, 200.0))])
def test_statistics_bit_for_bit(N, scan_at):
    """N = 9: pad rows and lane groups without a row; 1000: one split; 20 011: several splits and a
    masked last block.  Seven pairs in ONE call, each against scan_stats of that pair; each alone."""
    c = _case(N)
    eng, ref = c.engine(), c.engine(False)
    _, e32, xq = eng.encode(c.x)
    eng.scan_stats(e32, xq, *scan_at, keep_logits=True)
    assert eng.kept_queries() == 70 and ref.kept_queries() == 0
    got = eng.stats_kept(0, xq, PAIRS)
    assert got.shape == (len(PAIRS), 70, 4) and got.dtype == torch.float32
    for p, (ts, tg) in enumerate(PAIRS):
        want = ref.scan_stats(e32, xq, ts, tg)
        assert np.isfinite(want.cpu().numpy()).all()
        _same_bits(got[p], want, f"N={N} pair ({ts:g}, {tg:g}) of the seven")
        _same_bits(eng.stats_kept(0, xq, [(ts, tg)])[0], want, f"N={N} pair ({ts:g}, {tg:g}) alone")
    assert eng.kept_queries() == 70
    no_geo = got[PAIRS.index((15.0, 0.0))].cpu().numpy()
    assert (no_geo[:, 2] == np.float32(-1e30)).all() and (no_geo[:, 3] == 0).all()


def test_chunk_offset_and_nine_pairs():
    """The second chunk of a scan in two chunks with three forced splits; nine pairs = two launches."""
    c = _case(1000)
    qn = synth.make_queries(130, seed=21, lat_max=90.0)
    eng, ref = c.engine(), c.engine(False)
    _, e32, xq = eng.encode(_dev(qn))
    for lo, hi in ((0, 64), (64, 130)):
        eng.scan_stats_at(e32[lo:hi], xq[lo:hi], 12.0, 40.0, lo, 130, n_splits=3)
    assert eng.kept_queries() == 130
    nine = PAIRS + [(30.0, 30.0), (50.0, 0.0)]
    got = eng.stats_kept(64, xq[64:].contiguous(), nine, n_splits=3)
    assert got.shape == (9, 66, 4)
    for p, (ts, tg) in enumerate(nine):
        want = ref.scan_stats_at(e32[64:].contiguous(), xq[64:].contiguous(), ts, tg, 64, 130, n_splits=3)
        _same_bits(got[p], want, f"chunk [64, 130) pair ({ts:g}, {tg:g})")
    # ... and differ from the chunk's own choice of splits only in l's last bits, never in the shift of a constant pair
    auto = eng.stats_kept(64, xq[64:].contiguous(), PAIRS[:1])
    assert np.array_equal(auto[0, :, 0].cpu().numpy(), got[0, :, 0].cpu().numpy())


def _model_files(tmp_path):
    ck = synth.write_checkpoint(str(tmp_path / "e.ckpt"), L=L, hidden=H, seed=5)
    db = str(tmp_path / "db.npz")
    locs, vals, keys = synth.make_bank(1000, 77)
    vals[:, ONE] = 1.0
    np.savez(db, locs=locs, image_embeddings=vals, satclip_embeddings=keys)
    return ck, db


BETAS, TEMPS, GEO_TEMPS = (0.0, 0.5, 1.0), (12.0, 25.0, 100.0), (40.0, 200.0)
SWEEPS = {}


def test_sweep_against_float64(tmp_path):
    from range_amd import load_model
    c = _case(1000)
    ck, db = _model_files(tmp_path)
    m = load_model("RANGE+", pretrained_path=ck, device=DEV, db_path=db)
    sw = m.sweep(c.x, betas=BETAS, temps=TEMPS, geo_temps=GEO_TEMPS)
    SWEEPS["kept"] = sw
    emb = m(c.x)[:, 1024:]                     # (the model's own e-hat: its harmonics follow the reference's polynomials)
    assert isinstance(sw, np.ndarray) and sw.shape == (3, 2, 3, 70, 1280) and sw.dtype == np.float64
    for i, ts in enumerate(TEMPS):
        for j, tg in enumerate(GEO_TEMPS):
            for b, beta in enumerate(BETAS):
                c.check(sw[i, j, b], ts, tg, beta, "temperature sweep")
                assert np.abs(sw[i, j, b][:, ONE] - 1.0).max() <= 2e-5
                assert np.array_equal(sw[i, j, b][:, 1024:], emb)
    # both temperatures on the same side of 43: today's beta sweep at those temperatures, bit for bit
    for ts, tg in ((12.0, 40.0), (25.0, 40.0), (100.0, 200.0)):
        m.args.temp, m.args.geo_temp = ts, tg
        assert np.array_equal(sw[TEMPS.index(ts), GEO_TEMPS.index(tg)], m.sweep(c.x, BETAS)), (ts, tg)
    m.args.temp, m.args.geo_temp = 12.0, 40.0
    dev = m.sweep(c.x, betas=BETAS, temps=TEMPS, geo_temps=GEO_TEMPS, return_device=True)
    assert torch.is_tensor(dev) and dev.is_cuda and np.array_equal(dev.cpu().numpy(), sw)
    # the defaults of the lists: args.temp / args.geo_temp / args.beta
    one = m.sweep(c.x, temps=(25.0,))
    assert one.shape == (1, 1, 1, 70, 1280) and np.array_equal(one[0, 0, 0], sw[1, 0, 1])
    # RANGE: row i = model(coords) at args.temp = temps[i] (70 queries: the two passes)
    r = load_model("RANGE", pretrained_path=ck, device=DEV, db_path=db)
    rs = r.sweep(c.x, temps=(15.0, 100.0))
    assert rs.shape == (2, 70, 1280)
    for i, ts in enumerate((15.0, 100.0)):
        r.args.temp = ts
        assert np.array_equal(rs[i], r(c.x)), ts
        c.check(rs[i], ts, 0.0, 1.0, "RANGE temperature sweep")


def test_sweep_without_kept_logits(tmp_path, monkeypatch):
    from range_amd import load_model
    c = _case(1000)
    ck, db = _model_files(tmp_path)
    if "kept" not in SWEEPS:
        SWEEPS["kept"] = load_model("RANGE+", pretrained_path=ck, device=DEV, db_path=db).sweep(
            c.x, betas=BETAS, temps=TEMPS, geo_temps=GEO_TEMPS)
    monkeypatch.setenv("RANGE_KEEP_LOGITS", "0")
    m = load_model("RANGE+", pretrained_path=ck, device=DEV, db_path=db)
    monkeypatch.delenv("RANGE_KEEP_LOGITS")
    sw = m.sweep(c.x, betas=BETAS, temps=TEMPS, geo_temps=GEO_TEMPS)
    assert m.engine.kept_queries() == 0
    assert np.array_equal(sw, SWEEPS["kept"])


@pytest.mark.parametrize("planted", [False, True])
def test_two_shards_at_engine_level(planted):
    """Per-shard stats_kept merged by merge_stats == per-shard scan_stats_at merged, bit for bit; the
    finalized two-shard result against the single engine within the project's shard bound."""
    N, B = 1000, 40
    if planted:
        enc, obank, qn, vals = _planted_case(N, B, 901)
    else:
        c = _case(N)
        enc, obank, qn = c.enc, c.obank, c.qn[:B]
    bank = PreparedBank(obank.keys, obank.values, obank.xyz)
    cut = N // 2
    full = _engine(enc, bank)
    shards = [_engine(enc, bank.rows(0, cut), 0), _engine(enc, bank.rows(cut, N), cut)]
    refs = [_engine(enc, bank.rows(0, cut), 0, env=NO_KEEP), _engine(enc, bank.rows(cut, N), cut, env=NO_KEEP)]
    e64, e32, xq = full.encode(_dev(qn))
    for s in shards:
        s.scan_stats_at(e32, xq, 12.0, 40.0, 0, B)
        assert s.kept_queries() == B
    pairs = [(100.0, 200.0), (12.0, 40.0), (1000.0, 1000.0)]
    local = [s.stats_kept(0, xq, pairs) for s in shards]
    for p, (ts, tg) in enumerate(pairs):
        st = full.merge_stats(torch.stack([l[p] for l in local]))
        want = full.merge_stats(torch.stack([r.scan_stats_at(e32, xq, ts, tg, 0, B) for r in refs]))
        _same_bits(st, want, f"merged shards at ({ts:g}, {tg:g})")
        two = full.finalize(torch.stack([s.attend_kept(0, xq, ts, tg, 0.5, st) for s in shards]), e64).cpu().numpy()
        full.set_temperatures(ts, tg)
        one = full.forward(_dev(qn), _native.MODEL_RANGE_PLUS, 0.5).cpu().numpy()
        full.set_temperatures(0.0, 0.0)
        assert np.isfinite(two).all()
        np.testing.assert_allclose(two, one, rtol=0, atol=2e-6)


def test_nan_and_infinite_coordinates():
    c = _case(1000)
    eng, ref = c.engine(), c.engine(False)
    bad = c.qn[:40].copy()
    bad[3] = [np.nan, 10.0]
    bad[17] = [10.0, np.inf]
    _, e32, xq = eng.encode(_dev(bad))
    eng.scan_stats(e32, xq, 12.0, 40.0, keep_logits=True)
    got = eng.stats_kept(0, xq, [(100.0, 200.0)])[0]
    want = ref.scan_stats(e32, xq, 100.0, 200.0)
    g, w = got.cpu().numpy(), want.cpu().numpy()
    assert np.isnan(g[3, 1]) and np.isnan(g[3, 3]) and np.isnan(g[17, 1]) and np.isnan(g[17, 3])
    assert np.array_equal(g, w, equal_nan=True)
    keep = np.delete(np.arange(40), [3, 17])
    assert np.isfinite(g[keep]).all()
    _same_bits(got[keep], want[keep], "rows beside the NaN queries")


def test_refusals(tmp_path):
    from range_amd import load_model
    c = _case(1000)
    enc, bank = c.enc, c.bank
    eng = _engine(enc, bank)
    _, e32, xq = eng.encode(c.x)
    with pytest.raises(_native.RangeNativeError, match="no kept logits"):
        eng.stats_kept(0, xq, [(12.0, 40.0)])
    eng.scan_stats(e32, xq, 12.0, 40.0, keep_logits=True)
    with pytest.raises(_native.RangeNativeError, match="multiple of 64"):
        eng.stats_kept(32, xq[32:].contiguous(), [(12.0, 40.0)])
    with pytest.raises(_native.RangeNativeError, match="exceed the 70 kept"):
        eng.stats_kept(64, xq[:7].contiguous(), [(12.0, 40.0)])
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1001.0):
        with pytest.raises(_native.RangeNativeError, match="at most 1000"):
            eng.stats_kept(0, xq, [(12.0, 40.0), (bad, 40.0)])
        if bad > 0 or bad != bad:
            with pytest.raises(_native.RangeNativeError, match="at most 1000"):
                eng.stats_kept(0, xq, [(12.0, bad)])
    with pytest.raises(_native.RangeNativeError, match="n_taus"):
        eng.stats_kept(0, xq, [])
    with pytest.raises(_native.RangeNativeError, match="n_splits"):
        eng.stats_kept(0, xq, [(12.0, 40.0)], n_splits=-1)
    assert eng.stats_kept(0, xq, [(12.0, 40.0)]).shape == (1, 70, 4)       # (the refusals left the kept state alone)
    eng.set_bank(bank.keys[:500], bank.values[:500], bank.xyz[:500])
    with pytest.raises(_native.RangeNativeError, match="no kept logits|bank changed"):
        eng.stats_kept(0, xq, [(12.0, 40.0)])
    # the Python layer
    ck, db = _model_files(tmp_path)
    m = load_model("RANGE+", pretrained_path=ck, device=DEV, db_path=db)
    for kw in (dict(temps=()), dict(geo_temps=[]), dict(temps=(12.0,), betas=())):
        with pytest.raises(ValueError, match="must not be empty"):
            m.sweep(c.x, **kw)
    with pytest.raises(ValueError, match="at most 1000"):
        m.sweep(c.x, temps=(12.0, 1001.0))
    r = load_model("RANGE", pretrained_path=ck, device=DEV, db_path=db)
    with pytest.raises(ValueError, match="RANGE\\+ only"):
        r.sweep(c.x, temps=(15.0,), geo_temps=(40.0,))
    with pytest.raises(ValueError, match="RANGE\\+ only"):
        r.sweep(c.x, (0.5,), temps=(15.0,))
    b = load_model("RANGE+", pretrained_path=ck, device=DEV, db_path=db, pv_mode="bf16x3")
    with pytest.raises(ValueError, match="bf16x3"):
        b.sweep(c.x, temps=(12.0, 100.0))
    with pytest.raises(ValueError, match="bf16x3"):
        b.sweep(c.x, geo_temps=(200.0,))
