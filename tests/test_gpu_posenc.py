"""GPU tests of the training-free positional encoders 'Theory' / 's2vec_*' (posenc_kernel.h,
range_posenc_features): the kernel through the C ABI against the reference's recorded outputs
(tests/golden/posenc_encoders.npz) and against the numpy restatement (tests/posenc_refs.py, pinned to the
same fixture by tests/test_posenc_cpu.py) at the tile, wave and row edges; the model, the batch driver
and the hand-over to the probe.  Bounds: posenc_refs (derived there).  Run with ``pytest -m gpu``."""
import ctypes as C
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import posenc_refs as R
from range_amd import _native, posenc
from tools import synth

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
NAMES = tuple(R.KIND_OF_MODEL)
DEV = "cuda:0"
SENTINEL = -12345.678


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "posenc_encoders.npz"))


@pytest.fixture(scope="module")
def engine():
    return _native.HipEngine(DEV)


def abi_call(eng, kind_id, freq, lonlat, pad=64):
    """range_posenc_features through ctypes into a buffer with ``pad`` sentinel doubles before and after
    the output, which must come back untouched -> the (B, width) result as a host array."""
    freq = np.ascontiguousarray(freq, dtype=np.float64)
    q = torch.from_numpy(np.ascontiguousarray(lonlat, dtype=np.float64)).to(DEV)
    B, F = q.shape[0], freq.shape[0]
    width = eng.lib.range_posenc_width(kind_id, F)
    assert width == posenc.PER_FREQ[kind_id] * F
    buf = torch.full((pad + B * width + pad,), SENTINEL, dtype=torch.float64, device=DEV)
    out = buf[pad:pad + B * width]
    rc = eng.lib.range_posenc_features(eng._h, kind_id, freq.ctypes.data, F, q.data_ptr(), B, out.data_ptr(),
                                       torch.cuda.current_stream(eng.device).cuda_stream)
    assert rc == 0, eng.lib.range_last_error().decode()
    host = buf.cpu().numpy()
    assert (host[:pad] == SENTINEL).all() and (host[pad + B * width:] == SENTINEL).all()
    return host[pad:pad + B * width].reshape(B, width)


@pytest.mark.parametrize("name", NAMES)
def test_c_abi_with_the_fixtures_table(golden, engine, name):
    kind = R.KIND_OF_MODEL[name]
    got = abi_call(engine, R.KINDS.index(kind), golden[name + "_freq_list"], golden["lonlat"])
    err = np.abs(got - golden[name + "_f64"])
    print(name, "max |kernel - reference| =", np.nanmax(err))
    R.assert_close(kind, got, golden[name + "_f64"])


@pytest.mark.parametrize("name", NAMES)
def test_edge_shapes(engine, name):
    """B around the wave and the tile (F at the model's value: 16, 32, 48 - tiles cut rows, waves cut
    locations), output between sentinels."""
    kind, f = R.KIND_OF_MODEL[name], posenc.freq_list(name)
    q = synth.make_queries(257, seed=77, lat_max=90.0)
    ref = R.encode(kind, q, f)
    for B in (1, 63, 64, 65, 257):
        got = abi_call(engine, R.KINDS.index(kind), f, q[:B])
        R.assert_close(kind, got, ref[:B])


@pytest.mark.parametrize("kind", ["spherem", "theory"])
@pytest.mark.parametrize("F", [1, 16, 33, 64])
def test_random_tables(engine, kind, F):
    """A frequency count that does not divide the wave, a one-frequency row, the largest table."""
    rng = np.random.default_rng(100 + F)
    f = np.exp(rng.uniform(np.log(1e-3), np.log(100.0), size=F))
    q = synth.make_queries(65, seed=78 + F, lat_max=90.0)
    got = abi_call(engine, R.KINDS.index(kind), f, q)
    R.assert_close(kind, got, R.encode(kind, q, f))


def test_one_large_launch(engine):
    """spheremplus, B = 70 000 (287 MB): every row, and position independence - rows [12 345, 12 345 + 65)
    encoded alone equal the same rows of the large call bit for bit."""
    name, B, lo = "s2vec_spheremplus", 70_000, 12_345
    f = posenc.freq_list(name)
    q = synth.make_queries(B, seed=79, lat_max=90.0)
    x = torch.from_numpy(q).to(DEV)
    big = engine.posenc_features(x, posenc.KIND_SPHEREMPLUS, f)
    small = engine.posenc_features(x[lo:lo + 65].contiguous(), posenc.KIND_SPHEREMPLUS, f)
    assert torch.equal(big[lo:lo + 65], small)
    R.assert_close("spheremplus", big.cpu().numpy(), R.encode("spheremplus", q, f))


def test_abi_refuses_bad_arguments(engine):
    lib, h = engine.lib, engine._h
    f = np.ones(4)
    q = torch.zeros((2, 2), dtype=torch.float64, device=DEV)
    out = torch.zeros((2 * 64 + 1,), dtype=torch.float64, device=DEV)
    ok = (posenc.KIND_GRID, f.ctypes.data, 4, q.data_ptr(), 2, out.data_ptr())
    for i, bad in ((0, -1), (0, 6), (1, None), (2, 0), (2, 65), (3, None), (4, 0), (4, -5), (5, None),
                   (5, out.data_ptr() + 8)):
        a = list(ok)
        a[i] = bad
        assert lib.range_posenc_features(h, *a, None) == -1, (i, bad)      # RANGE_ERR_INVALID
    assert lib.range_posenc_features(None, *ok, None) == -1
    assert lib.range_posenc_width(6, 4) == 0 and lib.range_posenc_width(0, 65) == 0 and lib.range_posenc_width(5, 32) == 512
    assert lib.range_abi_version() == 9


@pytest.mark.parametrize("name", NAMES)
def test_through_the_model(golden, name, capsys):
    from range_amd import load_model
    kind = R.KIND_OF_MODEL[name]
    model = load_model(name, pretrained_path="unused", device=DEV)
    assert capsys.readouterr().out.splitlines()[0] == ("Using Theory" if name == "Theory" else "Using sphere2vec")
    lm = model.loc_model
    width = int(golden[name + "_embedding_dim"])
    assert model.location_feature_dim == width == lm.embedding_dim
    assert lm.frequency_num == int(golden[name + "_frequency_num"])
    assert float(lm.min_radius) == float(golden[name + "_min_radius"])
    assert float(lm.max_radius) == float(golden[name + "_max_radius"])
    assert (getattr(lm, "name", None) == name.split("_")[-1]) if name != "Theory" else not hasattr(lm, "name")
    assert len(list(model.parameters())) == 0
    widen = R.own_table_widen(kind, lm.freq_list, golden[name + "_freq_list"])
    q = golden["lonlat"]
    for dt, key in ((torch.float64, "_f64"), (torch.float32, "_f32")):
        coords = torch.from_numpy(q).to(dt)
        for c in (coords, coords.to(DEV)):
            for out in (model(c), model(c, return_device=True), lm(c)):
                assert type(out).__name__ == str(golden[name + "_type"]) == "Tensor"
                assert out.device == torch.device(DEV) and out.dtype == dt and out.shape == (16, width)
                R.assert_close(kind, out.cpu().numpy(), golden[name + key], widen)
        empty = model(torch.empty((0, 2), dtype=dt))
        assert empty.shape == (0, width) and empty.dtype == dt and empty.device == torch.device(DEV)
    # return_topk / sweep raise as they do for the other bank-less models
    wrap = load_model("Wrap", pretrained_path="unused", device=DEV)
    for call in (lambda m: m(torch.from_numpy(q[:4]), return_topk=4), lambda m: m.sweep(torch.from_numpy(q[:4]), [0.5])):
        with pytest.raises(Exception) as want:
            call(wrap)
        with pytest.raises(want.type):
            call(model)
    with pytest.raises(ValueError, match="needs a bank"):
        model(torch.from_numpy(q[:4]), return_topk=4)


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """save_embeddings with s2vec_spheremplus over loaders of 3 batches (300, 300, 41) for train and val."""
    from range_amd import load_model
    from range_amd.save import save_embeddings
    tmp = tmp_path_factory.mktemp("posenc_emb")
    model = load_model("s2vec_spheremplus", pretrained_path="unused", device=DEV)
    q = synth.make_queries(2 * 641, seed=80, lat_max=85.0)
    y = 25.0 * np.cos(np.deg2rad(q[:, 1])) + 3.0 * np.sin(np.deg2rad(2 * q[:, 0]))

    def loader(a):
        return [(torch.from_numpy(q[a + i:a + j]), torch.from_numpy(y[a + i:a + j]))
                for i, j in ((0, 300), (300, 600), (600, 641))]

    args = Namespace(embeddings_dir=str(tmp), location_model_name="s2vec_spheremplus", task_name="temperature",
                     device=DEV)
    assert "_pipeline_staging" not in model.__dict__
    save_embeddings(args, loader(0), loader(641), model)
    return args, model, q, y


def test_through_the_driver(saved):
    args, model, q, y = saved
    d = os.path.join(args.embeddings_dir, "s2vec_spheremplus")
    assert sorted(os.listdir(d)) == ["temperature_train.npz", "temperature_val.npz"]
    for part, a in (("train", 0), ("val", 641)):
        z = np.load(os.path.join(d, f"temperature_{part}.npz"))
        assert sorted(z.files) == ["coords", "embeddings", "y"]                 # range/utils/save.py:37
        assert np.array_equal(z["coords"], q[a:a + 641]) and np.array_equal(z["y"], y[a:a + 641])
        want = model(torch.from_numpy(q[a:a + 641])).cpu().numpy()
        assert z["embeddings"].dtype == np.float64 and z["embeddings"].shape == (641, 512)
        assert np.array_equal(z["embeddings"], want)
    # the pipelined branch ran: its staging buffers live on the model, sized for the largest batch
    pinned, dev = model.__dict__["_pipeline_staging"][2]
    assert all(p is not None and p.is_pinned() and tuple(p.shape) == (300, 512) for p in pinned)
    assert all(b is not None and b.is_cuda and tuple(b.shape) == (300, 512) for b in dev)


def test_driver_keeps_the_coordinates_dtype(saved):
    """float32 loaders: the files hold what model(coords) returns for float32 coordinates."""
    from range_amd.save import EmbeddingPipeline
    _, model, q, _ = saved
    q32 = q[:130].astype(np.float32)
    outs = list(EmbeddingPipeline(model).run([torch.from_numpy(q32[:100]), torch.from_numpy(q32[100:])]))
    want = model(torch.from_numpy(q32)).cpu().numpy()
    assert want.dtype == np.float32 and all(o.dtype == np.float32 for o in outs)
    assert np.array_equal(np.concatenate(outs), want)


def test_to_the_probe(saved, capsys):
    """evaluate_npz reads the files save_embeddings wrote: a smoke check of the hand-over, no accuracy asserted."""
    from range_amd import evaluate as ev
    score = ev.evaluate_npz(saved[0])
    assert capsys.readouterr().out.splitlines()[0] == "Regression Model"
    assert np.isfinite(score)
