"""GPU tests of the CSP location encoders 'CSP' / 'CSP_INat' (csp_kernel.h; range_set_csp, range_csp_encode):
the fused kernel through the C ABI against the numpy float64 restatement (tests/csp_refs.py, whose distance
to the reference's recorded float32 outputs tests/test_csp_cpu.py measures from tests/golden/csp_encoders.npz),
row independence bit for bit at the tile edges, the grid-stride walk, the model, the batch driver and the
hand-over to the probe.

Bound per fixture case: max |gpu - restatement| <= 4 * max(E_ref(case), 2^-23 max|out|) (csp_refs.gpu_bound:
E_ref is the reference's own distance to the restatement, from the fixture).  A network the fixture does not
hold (the 32-row tile needs a width above 512) takes the same rule with E_ref measured on torch's float32
CPU operators - the operators the reference's network is made of.  Run with ``pytest -m gpu``."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import csp_refs as R
from csp_sweep_cases import torch_f32
from range_amd import _native, csp, posenc
from tools import synth

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
SENTINEL = -12345.678
KIND = {"gridcell": posenc.KIND_GRID, "theory": posenc.KIND_THEORY}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "csp_encoders.npz"))


@pytest.fixture(scope="module")
def nets(golden):
    return {c: R.case_network(golden, c) for c in R.CASES}


@pytest.fixture(scope="module")
def engine():
    return _native.HipEngine(DEV)


def install(eng, net):
    """range_set_csp with a csp_refs network; returns (num_filts, tile rows)."""
    widths = [w.shape[0] for w in net["weights"]]
    eng.set_csp(KIND[net["spa_enc_type"]], net["freq_list"], widths, net["weights"], net["biases"], net["ln_gamma"],
                net["ln_beta"], csp.ACTIVATIONS[net["act"]], net["skip"], net["use_layn"])
    assert eng.lib.range_csp_width(eng._h) == widths[-1]
    return widths[-1], eng.lib.range_csp_tile_rows(eng._h)


def abi_call(eng, x, max_grid=None, pad=64):
    """range_csp_encode (``max_grid``: range_csp_encode_grid) on the (B,2) float64 device tensor ``x`` through
    ctypes, on torch's current stream, into a buffer with ``pad`` sentinel floats before and after the output,
    which must come back untouched -> the (B, width) result as a host array."""
    B, width = x.shape[0], eng.lib.range_csp_width(eng._h)
    buf = torch.full((pad + B * width + pad,), SENTINEL, dtype=torch.float32, device=DEV)
    out = buf[pad:pad + B * width]
    stream = torch.cuda.current_stream(eng.device).cuda_stream
    if max_grid is None:
        rc = eng.lib.range_csp_encode(eng._h, x.data_ptr(), B, out.data_ptr(), stream)
    else:
        rc = eng.lib.range_csp_encode_grid(eng._h, x.data_ptr(), B, out.data_ptr(), max_grid, stream)
    assert rc == 0, eng.lib.range_last_error().decode()
    host = buf.cpu().numpy()
    assert (host[:pad] == np.float32(SENTINEL)).all() and (host[pad + B * width:] == np.float32(SENTINEL)).all()
    return host[pad:pad + B * width].reshape(B, width).copy()


def dev(q):
    return torch.from_numpy(np.ascontiguousarray(q, dtype=np.float64)).to(DEV)


@pytest.mark.parametrize("case", R.CASES)
def test_c_abi_within_the_bound(golden, nets, engine, case):
    net, q, ref = nets[case], golden["lonlat"], golden[case + "_out"]
    width, _ = install(engine, net)
    got = abi_call(engine, dev(q))
    assert got.dtype == np.float32 and got.shape == ref.shape == (24, width)
    # NaN / infinite coordinates: NaN where the reference's rows are, the other rows finite
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(got[21:]).all() and np.isfinite(got[:21]).all()
    rows = R.finite_rows(ref)
    want = R.encode(net, q[rows])
    err = float(np.abs(got[rows].astype(np.float64) - want).max())
    bound = R.gpu_bound(golden, case, net)
    print(f"{case}: max|gpu - restatement| = {err:.3e}, E_ref = {R.e_ref(golden, case, net):.3e}, bound = {bound:.3e}, "
          f"max|gpu - reference| = {float(np.abs(got[rows] - ref[rows]).max()):.3e}")
    assert err <= bound


def wide_network(seed=301):
    """hidden 600 (> 512: the 32-row tile; not a multiple of 32), 2 hidden layers with skip + LayerNorm, gelu,
    theory features of F = 9 (54 wide: not a multiple of 8), 70 outputs."""
    s = dict(spa_enc_type="theory", F=9, hidden=600, layers=2, act="gelu", use_layn=True, skip=True, num_filts=70,
             min_radius=0.1, max_radius=360.0, seed=seed)
    sd = synth.make_csp_checkpoint(**s)["state_dict"]
    t = lambda i, k: sd[f"loc_enc.spa_enc.ffn.layers.{i}.{k}"].numpy()   # noqa: E731
    return dict(settings=s, spa_enc_type="theory", act="gelu", skip=True, use_layn=True,
                freq_list=csp.cal_freq_list("geometric", 9, 360.0, 0.1),
                weights=[t(i, "linear.weight") for i in range(3)], biases=[t(i, "linear.bias") for i in range(3)],
                ln_gamma=[t(0, "layernorm.weight"), t(1, "layernorm.weight"), None],
                ln_beta=[t(0, "layernorm.bias"), t(1, "layernorm.bias"), None])


def test_the_32_row_tile(engine):
    """A width above 512 takes the 32-row kernel: within the bound, E_ref from torch's float32 operators."""
    net = wide_network()
    width, T = install(engine, net)
    assert (width, T) == (70, 32)
    q = synth.make_queries(2 * T + 3, seed=91, lat_max=89.9)
    got = abi_call(engine, dev(q))
    want = R.encode(net, q)
    e_ref = float(np.abs(torch_f32(net, R.features("theory", q, net["freq_list"])).astype(np.float64) - want).max())
    bound = 4.0 * max(e_ref, 2.0 ** -23 * float(np.abs(want).max()))
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"wide: max|gpu - restatement| = {err:.3e}, E_ref(torch f32) = {e_ref:.3e}, bound = {bound:.3e}")
    assert err <= bound
    for B in (1, T - 1, T, T + 1):
        assert np.array_equal(abi_call(engine, dev(q[:B])), got[:B]), B


@pytest.mark.parametrize("case", ["a_design", "c_odd"])
def test_rows_are_independent_bit_for_bit(golden, nets, engine, case):
    """Batches cut from one query set: row i of every batch is row i of the largest, on the default and on
    another stream, and from an odd row offset into a larger coordinate tensor."""
    _, T = install(engine, nets[case])
    assert T == 64
    q = synth.make_queries(2 * T + 3, seed=92, lat_max=89.9)
    x = dev(q)
    full = abi_call(engine, x)
    assert np.isfinite(full).all()
    for B in (1, T - 1, T, T + 1):
        assert np.array_equal(abi_call(engine, x[:B]), full[:B]), B
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        on_side = abi_call(engine, x)
    assert np.array_equal(on_side, full)
    off = x[5:5 + T + 1]                     # a view 5 rows into the tensor: contiguous, 16-byte aligned only
    assert off.data_ptr() == x.data_ptr() + 5 * 16
    assert np.array_equal(abi_call(engine, off), full[5:5 + T + 1])


def test_grid_stride_walk(golden, nets, engine):
    """A grid capped below the tile count (the plan's max_grid): same bits as the uncapped launch."""
    _, T = install(engine, nets["b_theory"])
    B = 5 * T + 7
    x = dev(synth.make_queries(B, seed=93, lat_max=89.9))
    full = abi_call(engine, x)
    for cap in (1, 2, 4):
        assert np.array_equal(abi_call(engine, x, max_grid=cap), full), cap
    assert np.array_equal(abi_call(engine, x, max_grid=0), full)


def test_abi_refuses_bad_arguments(nets, engine):
    lib, h = engine.lib, engine._h
    fresh = _native.HipEngine(DEV)
    q = torch.zeros((4, 2), dtype=torch.float64, device=DEV)
    out = torch.zeros((4 * 256 + 4,), dtype=torch.float32, device=DEV)
    assert lib.range_csp_width(fresh._h) == 0 and lib.range_csp_tile_rows(fresh._h) == 0 and lib.range_csp_width(None) == 0
    assert lib.range_csp_encode(fresh._h, q.data_ptr(), 4, out.data_ptr(), None) == -1        # no network set
    install(engine, nets["d_nohidden"])
    ok = (q.data_ptr(), 4, out.data_ptr())
    for i, bad in ((0, None), (0, q.data_ptr() + 4), (1, 0), (1, -3), (2, None), (2, out.data_ptr() + 2)):
        a = list(ok)
        a[i] = bad
        assert lib.range_csp_encode(h, *a, None) == -1, (i, bad)                               # RANGE_ERR_INVALID
    assert lib.range_csp_encode(None, *ok, None) == -1
    assert lib.range_csp_encode_grid(h, *ok, -1, None) == -1
    assert lib.range_csp_encode(h, *ok, None) == 0
    # outside the envelope: refused when the network is set, the installed one stays
    f = np.ones(65)
    w = lambda o, i: np.zeros((o, i), dtype=np.float32)       # noqa: E731
    z = lambda o: np.zeros((o,), dtype=np.float32)            # noqa: E731
    for kind, F, widths in ((posenc.KIND_GRID, 65, [8]), (posenc.KIND_GRID, 4, [1025]), (posenc.KIND_GRID, 4, [1025, 8]),
                            (posenc.KIND_GRID, 4, [8] * 10), (posenc.KIND_SPHEREC, 4, [8])):
        d_in = [posenc.PER_FREQ[kind] * F] + widths[:-1]
        with pytest.raises(_native.RangeNativeError, match="error -1"):
            engine.set_csp(kind, f[:F], widths, [w(o, i) for o, i in zip(widths, d_in)], [z(o) for o in widths],
                           [None] * len(widths), [None] * len(widths), 1, False, False)
    with pytest.raises(_native.RangeNativeError, match="error -1"):
        engine.set_csp(posenc.KIND_GRID, f[:4], [8], [w(8, 16)], [z(8)], [None], [None], 5, False, False)   # activation
    with pytest.raises(_native.RangeNativeError, match="LayerNorm"):
        engine.set_csp(posenc.KIND_GRID, f[:4], [8, 8], [w(8, 16), w(8, 8)], [z(8), z(8)], [None, None], [None, None], 1, False, True)
    assert lib.range_csp_width(h) == 50 and lib.range_abi_version() == 9


@pytest.fixture(scope="module")
def checkpoints(golden, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("csp_ckpt")
    return {c: synth.write_csp_checkpoint(str(tmp / f"{c}.pth.tar"), **R.case_network(golden, c)["settings"]) for c in R.CASES}


@pytest.mark.parametrize("case", R.CASES)
def test_through_the_model(golden, nets, checkpoints, case, capsys):
    from range_amd import load_model
    net, q, ref = nets[case], golden["lonlat"], golden[case + "_out"]
    name = net["name"]
    model = load_model(name, pretrained_path=checkpoints[case], device=DEV)
    assert capsys.readouterr().out.splitlines()[0] == {"CSP": "Using CSP-FMOW", "CSP_INat": "Using CSP-INat"}[name]
    width = ref.shape[1]
    assert model.location_feature_dim == width == model.loc_model.loc_emb_dim
    # the parameter surface: the reference's names, float32, frozen, on the GPU
    sd = model.loc_model.state_dict()
    n = len(net["weights"])
    want_keys = {f"loc_enc.spa_enc.ffn.layers.{i}.linear.{k}" for i in range(n) for k in ("weight", "bias")} | \
                {f"loc_enc.spa_enc.ffn.layers.{i}.layernorm.{k}" for i in range(n) if net["ln_gamma"][i] is not None
                 for k in ("weight", "bias")}
    assert set(sd) == want_keys
    assert np.array_equal(sd["loc_enc.spa_enc.ffn.layers.0.linear.weight"].cpu().numpy(), net["weights"][0])
    params = list(model.parameters())
    assert params and all(p.dtype == torch.float32 and p.device == torch.device(DEV) and not p.requires_grad for p in params)
    rows = R.finite_rows(ref)
    want, bound = R.encode(net, q[rows]), R.gpu_bound(golden, case, net)
    first = None
    for dt in (torch.float64, torch.float32):
        coords = torch.from_numpy(q).to(dt)
        # (float32 coordinates are widened: the restatement of THOSE coordinates is the target)
        tgt = want if dt == torch.float64 else R.encode(net, q[rows].astype(np.float32))
        for c in (coords, coords.to(DEV)):
            for out in (model(c), model(c, return_device=True), model.loc_model(c), model.loc_model(c, return_feats=True)):
                assert type(out).__name__ == str(golden[case + "_type"]) == "Tensor"
                assert out.device == torch.device(DEV) and out.dtype == torch.float32 and out.shape == (24, width)
                o = out.cpu().numpy()
                assert np.array_equal(np.isnan(o), np.isnan(ref))
                assert float(np.abs(o[rows].astype(np.float64) - tgt).max()) <= bound
                if dt == torch.float64:
                    first = o if first is None else first
                    assert np.array_equal(o, first, equal_nan=True)
        empty = model(torch.empty((0, 2), dtype=dt))
        assert empty.shape == (0, width) and empty.dtype == torch.float32 and empty.device == torch.device(DEV)
    # return_topk / sweep raise as they do for the other bank-less models
    wrap = load_model("Wrap", pretrained_path="unused", device=DEV)
    for call in (lambda m: m(torch.from_numpy(q[:4]), return_topk=4), lambda m: m.sweep(torch.from_numpy(q[:4]), [0.5])):
        with pytest.raises(Exception) as want_exc:
            call(wrap)
        with pytest.raises(want_exc.type):
            call(model)
    with pytest.raises(ValueError, match="needs a bank"):
        model(torch.from_numpy(q[:4]), return_topk=4)


def test_a_second_set_replaces_the_first(golden, nets, engine):
    q = dev(golden["lonlat"][:21])
    install(engine, nets["f_tanh"])
    first = abi_call(engine, q)
    install(engine, nets["c_odd"])
    other = abi_call(engine, q)
    assert other.shape == (21, 24) and first.shape == (21, 256)
    install(engine, nets["f_tanh"])
    assert np.array_equal(abi_call(engine, q), first)
    fresh = _native.HipEngine(DEV)
    install(fresh, nets["c_odd"])
    assert np.array_equal(abi_call(fresh, q), other)


@pytest.fixture(scope="module")
def saved(checkpoints, tmp_path_factory):
    """save_embeddings with CSP (the design shape) over a 300-row dataset: train 200 in batches of 128 + 72, val 100."""
    from range_amd import load_model
    from range_amd.save import save_embeddings
    tmp = tmp_path_factory.mktemp("csp_emb")
    model = load_model("CSP", pretrained_path=checkpoints["a_design"], device=DEV)
    q = synth.make_queries(300, seed=94, lat_max=85.0)
    y = 25.0 * np.cos(np.deg2rad(q[:, 1])) + 3.0 * np.sin(np.deg2rad(2 * q[:, 0]))

    def loader(cuts):
        return [(torch.from_numpy(q[i:j]), torch.from_numpy(y[i:j])) for i, j in cuts]

    args = Namespace(embeddings_dir=str(tmp), location_model_name="CSP", task_name="temperature", device=DEV)
    save_embeddings(args, loader(((0, 128), (128, 200))), loader(((200, 300),)), model)
    return args, model, q, y


def test_through_the_driver(saved):
    args, model, q, y = saved
    d = os.path.join(args.embeddings_dir, "CSP")
    assert sorted(os.listdir(d)) == ["temperature_train.npz", "temperature_val.npz"]
    for part, a, b in (("train", 0, 200), ("val", 200, 300)):
        z = np.load(os.path.join(d, f"temperature_{part}.npz"))
        assert sorted(z.files) == ["coords", "embeddings", "y"]                 # range/utils/save.py:37
        assert np.array_equal(z["coords"], q[a:b]) and np.array_equal(z["y"], y[a:b])
        want = model(torch.from_numpy(q[a:b])).cpu().numpy()
        assert z["embeddings"].dtype == np.float32 and z["embeddings"].shape == (b - a, 256)
        assert np.array_equal(z["embeddings"], want)


def test_to_the_probe(saved, capsys):
    """evaluate_npz reads the files save_embeddings wrote: a smoke check of the hand-over, no accuracy asserted."""
    from range_amd import evaluate as ev
    score = ev.evaluate_npz(saved[0])
    assert capsys.readouterr().out.splitlines()[0] == "Regression Model"
    assert np.isfinite(score)
