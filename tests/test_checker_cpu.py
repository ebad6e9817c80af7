"""The checkerboard task, CPU side (no GPU): the host generation of range_amd/checker.py bit for bit against
what the reference's own checkerboarddataset.py produced (tests/golden/checker_dataset.npz, written by
make_golden_checker.py); the numpy restatement the GPU tests compare the kernel with (tests/checker_refs.py)
against the same fixture - every index, every distance within the derived bound; the gap that makes exact
indices a fair demand; planted defects; the launch plan under the host sanitizers; get_dataset's parsing and
errors."""
import os
import re
import subprocess
from argparse import Namespace

import numpy as np
import pytest

import checker_refs as R
from range_amd import checker

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUPPORTS = (16, 200, 1000)
SETS = ("seed0", "seed1", "grid2000", "grid1537", "rc")
CASES = [(S, tag) for S in SUPPORTS for tag in SETS]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "checker_dataset.npz"))


def support(golden, S):
    return np.stack([golden[f"S{S}_lons"], golden[f"S{S}_lats"]], axis=1)


@pytest.fixture(scope="module")
def restated(golden):
    """The restatement on every recorded case, once: (idx, dist, smallest relative gap)."""
    out = {}
    for S, tag in CASES:
        q, s = golden["q_" + tag], support(golden, S)
        out[S, tag] = R.nearest(q, s) + (R.relative_gap(q, s).min(),)
    return out


def test_fixture_is_small_and_complete(golden, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "checker_dataset.npz")) < 512 * 1024
    assert golden["q_grid1537"].shape == (1536, 2) and golden["q_grid2000"].shape == (2000, 2)
    for S, tag in CASES:
        n = len(golden["q_" + tag])
        for key in ("labels", "idx", "dist"):
            assert golden[f"S{S}_{tag}_{key}"].shape == (n,)
        assert not np.isnan(golden[f"S{S}_{tag}_dist"]).any()
    assert str(golden["full_banner"]) == "Classification Model" and 0.0 < float(golden["full_accuracy"]) <= 1.0


@pytest.mark.parametrize("S", SUPPORTS)
def test_host_generation_is_bitwise_the_references(golden, S):
    lons, lats, labels = checker.generate_fibonaccilattice(S, n_classes=16)
    assert lons.dtype == lats.dtype == np.float64 and labels.dtype == np.int64
    assert np.array_equal(lons, golden[f"S{S}_lons"]) and np.array_equal(lats, golden[f"S{S}_lats"])
    assert np.array_equal(labels, golden[f"S{S}_labels"])
    rc = (np.random.RandomState(3).rand(len(labels)) * 16).astype(int)
    assert np.array_equal(rc, golden[f"S{S}_rc_support_labels"])
    # the recorded labels are the recorded arg-min's labels
    for tag in SETS:
        sup = rc if tag == "rc" else labels
        assert np.array_equal(sup[golden[f"S{S}_{tag}_idx"].astype(np.int64)], golden[f"S{S}_{tag}_labels"])


def test_samples_are_bitwise_the_references(golden):
    for tag, (n, seed) in (("seed0", (1000, 0)), ("seed1", (1000, 1)), ("rc", (500, 3))):
        lons, lats = checker.random_samples(n, seed)
        assert np.array_equal(np.stack([lons, lats], axis=1), golden["q_" + tag])
    for tag, n in (("grid2000", 2000), ("grid1537", 1537)):
        lons, lats, _ = checker.generate_fibonaccilattice(n)
        assert np.array_equal(np.stack([lons, lats], axis=1), golden["q_" + tag])
    lons, lats = checker.random_samples(10000, 0)
    assert np.array_equal(np.stack([lons, lats], axis=1)[::97], golden["full_train_coords97"])
    lons, lats, _ = checker.generate_fibonaccilattice(10000)
    assert np.array_equal(np.stack([lons, lats], axis=1)[::97], golden["full_eval_coords97"])


def test_radians_is_one_rounded_product():
    """What the host hands to the kernel: numpy.radians(x) is x * (pi / 180), bit for bit."""
    x = np.random.default_rng(5).uniform(-400.0, 400.0, size=200_000)
    assert np.array_equal(np.radians(x), x * (np.pi / 180.0))


@pytest.mark.parametrize("S,tag", CASES)
def test_gap_precondition(golden, restated, S, tag):
    """No query of a recorded case has its two nearest supports closer than GAP_MIN relative to each other, none
    is NaN, and the reference's arg-min over the distance is the arg-min over a: no query is excused."""
    idx, dist, gap = restated[S, tag]
    print(f"S={S} {tag}: smallest relative gap {gap:.3e}")
    assert gap >= R.GAP_MIN
    assert (idx >= 0).all() and not np.isnan(dist).any()
    q, s = golden["q_" + tag], support(golden, S)
    a = R.term(q, s)
    assert np.array_equal(a.argmin(axis=1), R.distance(a).argmin(axis=1))


@pytest.mark.parametrize("S,tag", CASES)
def test_restatement_against_the_reference(golden, restated, S, tag):
    idx, dist, _ = restated[S, tag]
    assert np.array_equal(idx, golden[f"S{S}_{tag}_idx"].astype(np.int64))
    used = R.assert_dist_close(dist, golden[f"S{S}_{tag}_dist"])
    print(f"S={S} {tag}: restatement uses {used:.3f} of the distance bound")


@pytest.mark.parametrize("S", SUPPORTS)
def test_restatement_against_long_double(golden, S):
    q, s = golden["q_seed1"], support(golden, S)
    idx, dist = R.nearest(q, s)
    idx_ld, dist_ld = R.nearest_longdouble(q, s)
    assert np.array_equal(idx, idx_ld)
    # one side is (nearly) exact: half of the two-sided bound, plus the rounding of the arguments, which the two
    # float64 sides share and the exact one does not
    err = np.abs(dist.astype(np.longdouble) - dist_ld).astype(np.float64)
    assert (err <= 0.5 * R.dist_bound(dist) + R.argument_bound(dist)).all()


@pytest.mark.parametrize("S", SUPPORTS)
def test_nearest_neighbour_statistic_restated(golden, S):
    s = support(golden, S)
    _, dist = R.nearest(s, s, exclude_self=True, chunks=3)
    R.assert_dist_close(dist, golden[f"S{S}_nn_dist"])
    for unit, scale in (("rad", 1.0), ("km", 6371.0), ("deg", 180.0 / np.pi)):
        d = dist * (6371 if unit == "km" else 1)
        mean, std = (np.rad2deg(d.mean()), np.rad2deg(d.std())) if unit == "deg" else (d.mean(), d.std())
        want = golden[f"S{S}_avg_{unit}"]
        bound = R.stat_bound(golden[f"S{S}_nn_dist"], scale)
        assert abs(mean - want[0]) <= bound and abs(std - want[1]) <= bound


@pytest.mark.parametrize("chunks", [1, 2, 3, 7])
def test_restatement_does_not_depend_on_the_split(golden, chunks):
    q, s = golden["q_seed0"][:300], support(golden, 1000)
    one = R.nearest(q, s, tile=64, chunks=1)
    got = R.nearest(q, s, tile=64, chunks=chunks)
    assert np.array_equal(one[0], got[0]) and np.array_equal(one[1], got[1])


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_a_planted_defect_fails(golden, defect):
    """float32 trigonometry and a dropped cos(lat1) miss the fixture; last-index tie-breaking and a merge that
    ignores the index miss numpy.argmin on duplicated supports."""
    if defect in ("f32trig", "nocos1"):
        q, s = golden["q_seed0"], support(golden, 200)
        idx, dist = R.nearest(q, s, defect=defect)
        with pytest.raises(AssertionError):
            assert np.array_equal(idx, golden["S200_seed0_idx"].astype(np.int64))
            R.assert_dist_close(dist, golden["S200_seed0_dist"])
        return
    q, s = R.tie_case(64)
    want = R.term(q, s).argmin(axis=1)
    assert np.array_equal(want[:8], np.arange(8) + 8)
    for chunks in (1, 2, 3):
        assert np.array_equal(R.nearest(q, s, tile=64, chunks=chunks)[0], want)
    bad = [R.nearest(q, s, tile=64, chunks=chunks, defect=defect)[0] for chunks in (1, 2, 3)]
    assert any(not np.array_equal(b, want) for b in bad)


def test_nan_never_wins():
    q, s = R.random_points(5, 31), R.random_points(9, 32)
    q[2, 0] = np.nan
    s[4, 1] = np.nan
    idx, dist = R.nearest(q, s)
    assert idx[2] == -1 and np.isnan(dist[2])
    ok = [0, 1, 3, 4]
    keep = [j for j in range(9) if j != 4]
    idx_ref, dist_ref = R.nearest(q[ok], s[keep])
    assert np.array_equal(np.asarray(keep)[idx_ref], idx[ok]) and np.array_equal(dist_ref, dist[ok])


def test_checker_plan_under_sanitizers(tmp_path):
    """host_plan.h: checker_plan - for Q in {1, 63, 64, 65, 257, 10 000, 2^33} x S in {1, T-1, T, T+1, 2T+1, 10^5}
    and several max_chunks the walks cover every query and every support point exactly once, workspace sizes, the
    refusals - compiled with g++ under AddressSanitizer and UndefinedBehaviorSanitizer and run on the CPU."""
    exe = str(tmp_path / "checker_plan")
    src = os.path.join(REPO, "tests", "native", "checker_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    src, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "checker_plan ok" in p.stdout, p.stdout + p.stderr
    assert int(re.search(r"tile=(\d+)", p.stdout).group(1)) == R.TILE


def test_host_refuses_non_finite_coordinates():
    with pytest.raises(ValueError, match="non-finite"):
        checker._radians_pairs(np.array([0.0, np.nan]), np.array([0.0, 1.0]), "query points")
    with pytest.raises(ValueError, match="non-finite"):
        checker.nearest_support(np.array([0.0]), np.array([np.inf]), np.array([0.0]), np.array([1.0]), device="cuda:0")
    with pytest.raises(ValueError, match="unit"):
        checker.calculate_average_distance_between_closest_neighbors(np.zeros(4), np.zeros(4), unit="miles")


def test_get_dataset_parsing_and_errors(monkeypatch):
    import range_amd
    from range_amd import load_dataset
    assert range_amd.get_dataset is load_dataset.get_dataset and range_amd.CheckerDataset is checker.CheckerDataset
    seen = {}

    class FakeDataset:
        def __init__(self, **kw):
            seen.update(kw)
            self.train_ds, self.valid_ds, self.evalu_ds = [("t", 0)] * 5, [("v", 0)] * 5, [("e", 0)] * 7

    monkeypatch.setattr(checker, "CheckerDataset", FakeDataset)
    args = Namespace(task_name="checker_200", batch_size=4, num_workers=0, device="cuda:0")
    train, val, n_classes = load_dataset.get_dataset(args)
    assert seen == dict(num_samples=10000, num_classes=16, num_support=200, device="cuda:0") and n_classes == 16
    assert len(train.dataset) == 5 and len(val.dataset) == 7 and train.batch_size == val.batch_size == 4
    assert not train.drop_last and type(train.sampler).__name__ == "SequentialSampler"
    load_dataset.get_dataset(Namespace(task_name="my_checker_run_1000", batch_size=1, num_workers=0))
    assert seen["num_support"] == 1000 and seen["device"] is None
    with pytest.raises(ValueError, match="invalid literal"):
        load_dataset.get_dataset(Namespace(task_name="checker_many", batch_size=1, num_workers=0))
    for task in load_dataset.CSV_TASKS + ("era5-temperature",):
        with pytest.raises(NotImplementedError, match=task):
            load_dataset.get_dataset(Namespace(task_name=task, batch_size=1, num_workers=0))
    with pytest.raises(ValueError, match="Task name not recognized"):
        load_dataset.get_dataset(Namespace(task_name="chess_200", batch_size=1, num_workers=0))
