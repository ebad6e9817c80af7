"""GPU tests of the checkerboard task (checker_kernel.h, range_nearest_support, range_amd/checker.py,
range_amd/load_dataset.py): the scan through the C ABI against what the reference's own haversine matrix gave
(tests/golden/checker_dataset.npz) and against the numpy restatement (tests/checker_refs.py, pinned to the same
fixture by tests/test_checker_cpu.py) at the wave, tile and chunk edges; ties, the split, exclude_self, NaN;
the dataset, the loaders and one task end to end.  Indices are exact - after the gap between a query's two
nearest supports has been asserted on the restatement - and distances within checker_refs.dist_bound (derived
there).  Run with ``pytest -m gpu``."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import checker_refs as R
from range_amd import _native, checker

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
T = R.TILE
SUPPORTS = (16, 200, 1000)
SETS = ("seed0", "seed1", "grid2000", "grid1537", "rc")
IDX_SENTINEL, DIST_SENTINEL, PAD = -777, -12345.678, 64
INVALID = -1       # RANGE_ERR_INVALID


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "checker_dataset.npz"))


@pytest.fixture(scope="module")
def engine():
    return _native.HipEngine(DEV)


def support(golden, S):
    return np.stack([golden[f"S{S}_lons"], golden[f"S{S}_lats"]], axis=1)


def abi_call(eng, q_deg, s_deg, exclude_self=False, max_chunks=0, want_dist=True, stream=None):
    """range_nearest_support through ctypes, the outputs between sentinels that must come back untouched
    -> (idx, dist or None) as host arrays."""
    q = torch.from_numpy(np.radians(np.ascontiguousarray(q_deg, dtype=np.float64))).to(DEV)
    s = torch.from_numpy(np.radians(np.ascontiguousarray(s_deg, dtype=np.float64))).to(DEV)
    Q, S = q.shape[0], s.shape[0]
    ibuf = torch.full((PAD + Q + PAD,), IDX_SENTINEL, dtype=torch.int64, device=DEV)
    dbuf = torch.full((PAD + Q + PAD,), DIST_SENTINEL, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    st = stream if stream is not None else torch.cuda.current_stream(eng.device)
    rc = eng.lib.range_nearest_support(eng._h, q.data_ptr(), Q, s.data_ptr(), S, int(exclude_self), max_chunks,
                                       ibuf[PAD:].data_ptr(), dbuf[PAD:].data_ptr() if want_dist else None, st.cuda_stream)
    assert rc == 0, eng.lib.range_last_error().decode()
    st.synchronize()
    ih, dh = ibuf.cpu().numpy(), dbuf.cpu().numpy()
    assert (ih[:PAD] == IDX_SENTINEL).all() and (ih[PAD + Q:] == IDX_SENTINEL).all()
    assert (dh[:PAD] == DIST_SENTINEL).all() and (dh[PAD + Q:] == DIST_SENTINEL).all()
    if not want_dist:
        assert (dh == DIST_SENTINEL).all()
    return ih[PAD:PAD + Q], (dh[PAD:PAD + Q] if want_dist else None)


@pytest.mark.parametrize("S", SUPPORTS)
def test_c_abi_against_the_fixture(golden, engine, S):
    s = support(golden, S)
    for tag in SETS:
        idx, dist = abi_call(engine, golden["q_" + tag], s)
        used = R.assert_dist_close(dist, golden[f"S{S}_{tag}_dist"])
        print(f"S={S} {tag}: kernel uses {used:.3f} of the distance bound")
        assert np.array_equal(idx, golden[f"S{S}_{tag}_idx"].astype(np.int64))


@pytest.fixture(scope="module")
def edge_points():
    """257 queries, 2T + 1 supports and the restatement on every prefix pair of the edge test, once."""
    q, s = R.random_points(257, 41), R.random_points(2 * T + 1, 42)
    ref = {}
    for S in (1, 2, T - 1, T, T + 1, 2 * T + 1):
        idx, dist = R.nearest(q, s[:S])
        ref[S] = (idx, dist, R.relative_gap(q, s[:S]) if S >= 2 else np.full(257, np.inf))
    return q, s, ref


@pytest.mark.parametrize("S", [1, 2, T - 1, T, T + 1, 2 * T + 1])
def test_edge_shapes(engine, edge_points, S):
    q, s, ref = edge_points
    idx_ref, dist_ref, gap = ref[S]
    assert gap.min() >= R.GAP_MIN               # the precondition of exact indices, on the restatement
    for Q in (1, 63, 64, 65, 257):
        idx, dist = abi_call(engine, q[:Q], s[:S])
        assert np.array_equal(idx, idx_ref[:Q])
        R.assert_dist_close(dist, dist_ref[:Q])


def test_ties_go_to_the_lower_index(engine):
    """Duplicated support points in one tile, in other tiles, in other chunks: numpy.argmin's answer every time."""
    q, s = R.tie_case(T)
    want = R.term(q, s).argmin(axis=1)
    assert np.array_equal(want[:8], np.arange(8) + 8)
    assert np.array_equal(R.nearest(q, s, chunks=3)[0], want)
    for max_chunks in (1, 2, 3, 4, 0):
        idx, dist = abi_call(engine, q, s, max_chunks=max_chunks)
        assert np.array_equal(idx, want), max_chunks
        assert (dist[:8] == 0.0).all()


def test_result_does_not_depend_on_the_split(engine):
    q, s = R.random_points(257, 43), R.random_points(7 * T + 3, 44)
    one = abi_call(engine, q, s, max_chunks=1)
    assert R.relative_gap(q, s).min() >= R.GAP_MIN
    assert np.array_equal(one[0], R.nearest(q, s)[0])
    for max_chunks in (2, 3, 7, 0):
        got = abi_call(engine, q, s, max_chunks=max_chunks)
        assert np.array_equal(one[0], got[0]) and np.array_equal(one[1], got[1]), max_chunks      # bit for bit


@pytest.mark.parametrize("S", SUPPORTS)
def test_exclude_self_and_the_neighbour_statistic(golden, engine, S):
    s = support(golden, S)
    want = golden[f"S{S}_nn_dist"]
    for max_chunks in (0, 2):
        idx, dist = abi_call(engine, s, s, exclude_self=True, max_chunks=max_chunks)
        assert (idx != np.arange(len(s))).all() and (idx >= 0).all()
        R.assert_dist_close(dist, want)
    for unit, scale in (("deg", 180.0 / np.pi), ("km", 6371.0), ("rad", 1.0)):
        mean, std = checker.calc_avg_distances(S, unit=unit, device=DEV)
        ref, bound = golden[f"S{S}_avg_{unit}"], R.stat_bound(want, scale)
        print(f"S={S} {unit}: |mean - ref| = {abs(mean - ref[0]):.3e}, |std - ref| = {abs(std - ref[1]):.3e}, bound {bound:.3e}")
        assert abs(mean - ref[0]) <= bound and abs(std - ref[1]) <= bound


def test_another_stream_and_no_distances(golden, engine):
    q, s = golden["q_seed0"], support(golden, 1000)
    want = golden["S1000_seed0_idx"].astype(np.int64)
    side = torch.cuda.Stream(device=DEV)
    idx, dist = abi_call(engine, q, s, stream=side, max_chunks=3)
    assert np.array_equal(idx, want)
    R.assert_dist_close(dist, golden["S1000_seed0_dist"])
    for max_chunks in (1, 3):
        idx, none = abi_call(engine, q, s, want_dist=False, max_chunks=max_chunks)
        assert none is None and np.array_equal(idx, want)


def test_nan_never_wins(engine):
    q, s = R.random_points(70, 31), R.random_points(T + 9, 32)
    q[2, 0] = np.nan
    s[4, 1] = np.nan
    s[T + 1, 0] = np.nan
    idx_ref, dist_ref = R.nearest(q, s)
    assert idx_ref[2] == -1 and (np.delete(idx_ref, 2) >= 0).all()
    for max_chunks in (1, 2):
        idx, dist = abi_call(engine, q, s, max_chunks=max_chunks)
        assert idx[2] == -1 and np.isnan(dist[2])
        assert np.array_equal(idx, idx_ref) and not np.isin(idx, (4, T + 1)).any()
        R.assert_dist_close(dist, dist_ref)
    # a support of NaN points only: no query has a valid pair
    idx, dist = abi_call(engine, q[:5], np.full((3, 2), np.nan))
    assert (idx == -1).all() and np.isnan(dist).all()


def test_abi_refuses_bad_arguments(engine):
    lib, h = engine.lib, engine._h
    q = torch.zeros((4, 2), dtype=torch.float64, device=DEV)
    s = torch.ones((4, 2), dtype=torch.float64, device=DEV)
    idx = torch.zeros((4,), dtype=torch.int64, device=DEV)
    dist = torch.zeros((4,), dtype=torch.float64, device=DEV)
    ok = [q.data_ptr(), 4, s.data_ptr(), 4, 0, 0, idx.data_ptr(), dist.data_ptr()]
    assert lib.range_nearest_support(h, *ok, None) == 0
    for i, bad in ((0, None), (2, None), (6, None), (1, 0), (1, -3), (3, 0), (3, -1), (5, -1)):
        a = list(ok)
        a[i] = bad
        assert lib.range_nearest_support(h, *a, None) == INVALID, (i, bad)
    assert lib.range_nearest_support(None, *ok, None) == INVALID
    # exclude_self: the same number of points on both sides, at least two
    a = list(ok)
    a[4] = 1
    assert lib.range_nearest_support(h, *a, None) == 0
    a[1] = 3
    assert lib.range_nearest_support(h, *a, None) == INVALID
    a[1], a[3] = 1, 1
    assert lib.range_nearest_support(h, *a, None) == INVALID
    torch.cuda.synchronize()
    assert lib.range_abi_version() == 9
    with pytest.raises(ValueError):
        engine.nearest_support(q.float(), s)


@pytest.fixture(scope="module")
def loaders():
    from range_amd import get_dataset
    return get_dataset(Namespace(task_name="checker_200", batch_size=1000, num_workers=0, device=DEV))


def test_checker_dataset_at_full_size(golden):
    from range_amd import CheckerDataset
    ds = CheckerDataset(10000, num_classes=16, num_support=200, device=DEV)
    for part, tag in ((ds.train_ds, "train"), (ds.valid_ds, "valid"), (ds.evalu_ds, "eval")):
        coords, y = part.tensors
        assert coords.dtype == torch.float64 and tuple(coords.shape) == (10000, 2) and y.dtype == torch.int64
        assert np.array_equal(y.numpy(), golden[f"full_{tag}_labels"].astype(np.int64))
        if tag != "valid":
            assert np.array_equal(coords.numpy()[::97], golden[f"full_{tag}_coords97"])
    bound = R.stat_bound(golden["S200_nn_dist"], 180.0 / np.pi)
    assert abs(ds.mean_dist - float(golden["full_mean_dist"])) <= bound
    assert abs(ds.std_dist - float(golden["full_std_dist"])) <= bound
    assert (ds.num_samples, ds.num_classes, ds.num_support) == (10000, 16, 200)


def test_get_dataset(golden, loaders):
    train, val, n_classes = loaders
    assert n_classes == 16 and len(train) == len(val) == 10
    for loader, tag in ((train, "train"), (val, "eval")):
        items = list(loader)
        assert all(len(item) == 2 for item in items)                       # (coords, y): what save_embeddings unpacks
        coords, y = items[0]
        assert tuple(coords.shape) == (1000, 2) and coords.dtype == torch.float64 and y.dtype == torch.int64
        assert np.array_equal(torch.cat([i[1] for i in items]).numpy(), golden[f"full_{tag}_labels"].astype(np.int64))
        assert np.array_equal(torch.cat([i[0] for i in items]).numpy()[::97], golden[f"full_{tag}_coords97"])
    with pytest.raises(ValueError, match="non-finite"):
        checker.assign_closest_label(np.array([np.nan]), np.array([0.0]), np.zeros(3), np.zeros(3), np.arange(3), device=DEV)


def test_one_task_end_to_end(golden, loaders, tmp_path, capsys):
    """get_dataset('checker_200') -> load_model('s2vec_grid') -> save_embeddings -> evaluate_npz: the probe's accuracy
    equals the oracle's on the same files and what the reference's evaluate_npz gave on its own embeddings of the
    reference's dataset (accuracies are ratios of counts: identical unless an arg-max is tied to rounding)."""
    from oracle import probe_oracle as po
    from range_amd import evaluate_npz, load_model, save_embeddings
    train, val, _ = loaders
    model = load_model("s2vec_grid", pretrained_path="unused", device=DEV)
    args = Namespace(embeddings_dir=str(tmp_path), location_model_name="s2vec_grid", task_name="checker_200", device=DEV)
    save_embeddings(args, train, val, model)
    capsys.readouterr()
    acc = evaluate_npz(args)
    assert capsys.readouterr().out.splitlines()[0] == str(golden["full_banner"]) == "Classification Model"
    tr = np.load(os.path.join(str(tmp_path), "s2vec_grid", "checker_200_train.npz"))
    va = np.load(os.path.join(str(tmp_path), "s2vec_grid", "checker_200_val.npz"))
    assert np.array_equal(tr["y"], golden["full_train_labels"].astype(np.int64))
    assert np.array_equal(va["y"], golden["full_eval_labels"].astype(np.int64))
    ref = po.probe(tr["embeddings"], tr["y"], va["embeddings"], va["y"], po.task_kind("checker_200"))
    print(f"accuracy {acc}, oracle {ref['score']}, reference {float(golden['full_accuracy'])}")
    assert acc == ref["score"]
    assert acc == float(golden["full_accuracy"])
