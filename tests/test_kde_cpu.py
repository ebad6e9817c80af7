"""CPU tests of the KDE geo prior (range_amd/geo_baselines.py: create_kde_grid / KdePrior, csp_eval.compute_acc_batch's
'kde' branch, host_plan.h: kde_plan): the binning reproduces the reference's three arrays bit for bit
(tests/golden/kde_priors.npz); the numpy restatement (tests/kde_refs.py) gives its member sets and its priors within
the derived bound of layer 1; planted defects each exceed the end-to-end bound; the fixed-point emulation is
independent of order and of count-vs-duplicates; the launch plan under the host sanitizers; the seeds of the GPU
sweeps leave out no query; ``compute_acc_batch`` on a numpy stand-in.  No GPU."""
import logging
import os
import re
import subprocess

import numpy as np
import pytest

import kde_refs as K
import neighbor_refs as R
from range_amd import csp_eval
from range_amd import geo_baselines as gb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "kde_priors.npz")
INPUTS = [f"{m}_C{c}" for m in ("haversine", "euclidean") for c in (1, 5, 33)]
QUANTS = (5.0, 1.0, 0.001)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def cases_of(golden, name):
    """(tag, quant, nb, case) of every recorded case of an input set."""
    for n, quant in enumerate(QUANTS):
        tag = f"{name}_q{n}"
        M = len(golden[tag + "_counts"])
        for nb, label in ((1, "1"), (7, "7"), (M, "M")):
            yield tag, quant, nb, f"{tag}_nb{label}"


@pytest.mark.parametrize("name", INPUTS)
def test_binning_bit_for_bit(golden, name):
    s, classes = golden[name + "_s"], golden[name + "_classes"]
    for n, quant in enumerate(QUANTS):
        tag = f"{name}_q{n}"
        want = [golden[tag + k] for k in ("_bclasses", "_blocs", "_counts")]
        for got in (gb.create_kde_grid(classes, s, {"kde_quant": quant}), K.bin_grid(classes, s, quant)):
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
        bclasses, blocs, counts = want
        assert counts.sum() == len(s) and counts.min() >= 1
        # first-occurrence order: the bins' first members ascend
        key = np.floor(np.floor(s / quant) * quant / quant).astype(np.int64)
        first = [int(np.flatnonzero((classes == c) & (key == np.floor(l / quant).astype(np.int64)).all(1))[0])
                 for c, l in zip(bclasses, blocs)]
        assert first == sorted(first) and len(set(first)) == len(first)
        if quant == 0.001:
            # condition (c): the literal hashable_loc differs from floor(x / q) somewhere, and the binning follows it
            assert (key != np.floor(s / quant).astype(np.int64)).any()
    with pytest.raises(AssertionError):
        gb.create_kde_grid(classes, s, {"kde_quant": 0.0})
    bad = s.copy()
    bad[17, 1] = np.inf
    with pytest.raises(ValueError, match="location 17"):
        gb.create_kde_grid(classes, bad, {"kde_quant": 1.0})
    bad[17, 1] = np.nan
    with pytest.raises(ValueError, match="location 17"):
        gb.create_kde_grid(classes, bad, {"kde_quant": 1.0})


@pytest.mark.parametrize("name", INPUTS)
def test_restatement_against_the_reference(golden, name):
    """Members equal; h within the tree's own 4 ulp; priors within layer 1's derived bound; conditions (a), (b), (d)."""
    hav, C = name.startswith("haversine"), int(name.split("_C")[1])
    q, labels, img = golden[name + "_q"], golden[name + "_labels"], golden[name + "_img"]
    assert np.isnan(q[:, 0]).sum() == 1 and np.isnan(q[:, 1]).sum() == 1
    worst = 0.0
    for tag, quant, nb, case in cases_of(golden, name):
        bclasses, blocs, counts = (golden[tag + k] for k in ("_bclasses", "_blocs", "_counts"))
        want, h, members = golden[case + "_prior"], golden[case + "_h"], golden[case + "_members"].astype(bool)
        rows = K.Rows(q, blocs, hav, nb)
        assert np.array_equal(rows.members, members)
        assert np.array_equal(np.isnan(rows.h), np.isnan(h)) and np.isnan(h).sum() == 2
        ok = ~np.isnan(h)
        assert (np.abs(rows.h[ok] - h[ok]) <= 4 * K.ULP * h[ok]).all()
        gap, own = rows.gaps()
        assert gap.min() >= R.GAP_FIXTURE and own.min() >= 2.0 ** -40
        got = K.kde_prior_exact(rows, bclasses, counts, C)
        rel = np.abs(got - want) / want
        bound = K.layer1_bound(members.sum(1), C)
        assert (rel <= bound[:, None]).all(), (case, rel.max())
        worst = max(worst, float(rel.max()))
        assert np.array_equal(want[~ok], np.full((2, C), 1.0 / C))                # the NaN rows: uniform
        np.testing.assert_allclose(want.sum(1), 1.0, rtol=1e-12)
        # (d) and the recorded ranks
        sc = img.astype(np.float64) * want
        lab = sc[np.arange(len(q)), labels][:, None]
        near = np.abs(sc - lab) <= 1e-9 * np.abs(lab)
        near[np.arange(len(q)), labels] = False
        assert not near.any()
        assert np.array_equal(csp_eval.get_label_rank(sc, labels), golden[case + "_ranks"])
        assert np.array_equal(csp_eval.get_label_rank(img.astype(np.float64) * got, labels), golden[case + "_ranks"])
    print(f"{name}: largest |reference - exact| / exact {worst:.3e}")
    assert worst < 1e-14                                                          # the sanity check, not the bound


def test_numpy_exp_is_within_its_unit():
    """kde_refs.U_NUMPY_EXP: numpy's float64 exp against 40-digit decimal arithmetic over the weights' argument
    range, in units of 2^-52."""
    import decimal
    ctx = decimal.Context(prec=40)
    x = np.concatenate([np.linspace(K.ARG_MIN, 0.0, 10001), -np.random.default_rng(3).random(10000) * 2])
    got = np.exp(x)
    worst = max(abs(decimal.Decimal(float(g)) - ctx.exp(decimal.Decimal(float(v)))) for g, v in zip(got, x))
    assert float(worst / decimal.Decimal(K.ULP)) <= K.U_NUMPY_EXP
    assert np.exp(K.ARG_MIN) >= K.W_MIN


def test_planted_defects_exceed_the_end_to_end_bound(golden):
    """Each defect, planted into the restatement, misses the fixture by more than layer 3's bound on some row of
    some case.  scikit-learn's expression order for the haversine dist stays within it (a few ulp on a): it is not a
    defect this fixture can see, and not listed."""
    def worst_excess(name, **defect):
        hav, C = name.startswith("haversine"), int(name.split("_C")[1])
        q = golden[name + "_q"]
        out = 0.0
        for tag, quant, nb, case in cases_of(golden, name):
            bclasses, blocs, counts = (golden[tag + k] for k in ("_bclasses", "_blocs", "_counts"))
            want = golden[case + "_prior"]
            clean = K.Rows(q, blocs, hav, nb)
            bound = K.layer3_bound(clean, C, K.scale_bits(int(counts.sum())))
            rows_kw = {k: v for k, v in defect.items() if k in ("radius_eps", "h_factor", "sklearn_order")}
            prior_kw = {k: v for k, v in defect.items() if k not in rows_kw}
            got = K.kde_prior_exact(K.Rows(q, blocs, hav, nb, **rows_kw), bclasses, counts, C, **prior_kw)
            ok = ~clean.nan
            out = max(out, float((np.abs(got - want)[ok] / want[ok] / bound[ok, None]).max()))
        return out

    for name in ("haversine_C33", "euclidean_C5"):
        assert worst_excess(name) <= 1.0                                         # the restatement itself
        assert worst_excess(name, radius_eps=0.0) > 1.0                         # radius without the 1e-9: the k-th bin drops out
        assert worst_excess(name, h_factor=1.0) > 1.0                           # h = d_k
        assert worst_excess(name, use_counts=False) > 1.0                       # counts ignored
        assert worst_excess(name, min_per_class=False) > 1.0                    # the minimum added once
        assert worst_excess(name, min_over_zero=True) > 1.0                     # the minimum over all classes, zero included
    assert worst_excess("haversine_C33", sklearn_order=True) <= 1.0


def test_fixed_point_is_order_free_and_counts_are_duplicates(golden):
    name, tag = "euclidean_C33", "euclidean_C33_q0"
    q = golden[name + "_q"]
    bclasses, blocs, counts = (golden[tag + k] for k in ("_bclasses", "_blocs", "_counts"))
    assert counts.max() > 1
    s = K.scale_bits(int(counts.sum()))
    assert s == 52
    for nb in (1, 7, len(counts)):
        base = K.fixed_sums(K.Rows(q, blocs, False, nb), bclasses, counts, 33, s)
        assert base.max() < 2 ** 62 and base.sum(1).max() < 2 ** 62
        perm = np.random.default_rng(nb).permutation(len(counts))
        assert np.array_equal(K.fixed_sums(K.Rows(q, blocs[perm], False, nb), bclasses[perm], counts[perm], 33, s), base)
        # the prior of the integers is the exact formula to within the rint of every member: layer 3 without a device
        rows = K.Rows(q, blocs, False, nb)
        exact = K.kde_prior_exact(rows, bclasses, counts, 33)
        rel = np.abs(K.prior_from_sums(base) - exact) / exact
        assert (rel <= K.layer3_bound(rows, 33, s)[:, None]).all()
    # a bin of count n is n bins of count 1 - for the scan; the selection counts bins, so thr and two_h2 are held
    rows = K.Rows(q, blocs, False, 7)
    rep = np.repeat(np.arange(len(counts)), counts)
    dup = K.Rows(q, blocs[rep], False, 7)
    dup.thr, dup.two_h2 = rows.thr, rows.two_h2
    with np.errstate(invalid="ignore"):
        dup.members = dup.red <= dup.thr[:, None]
        dup.w = np.exp(-dup.dist / dup.two_h2[:, None])
    assert np.array_equal(K.fixed_sums(dup, bclasses[rep], np.ones(len(rep), dtype=np.int64), 33, s),
                          K.fixed_sums(rows, bclasses, counts, 33, s))
    # the scale bits follow the total
    assert [K.scale_bits(t) for t in (1, 1023, 1024, 436000, 2 ** 31 - 1)] == [52, 52, 51, 43, 31]


def test_sweep_seeds_leave_out_no_query():
    """The GPU sweeps would leave out queries with a pair nearer than 2^-40 (relative) to thr, the k-th's own margin
    included; with these seeds there is none, and no bandwidth is zero."""
    for hav in (True, False):
        for seed, M in K.SWEEP_SEEDS:
            s, _, _, q = K.sweep_points(seed, M, 5)
            for nb in K.SWEEP_NBS + (M,):
                if nb <= M:
                    rows = K.Rows(q, s, hav, nb)
                    gap, own = rows.gaps()
                    assert min(gap.min(), own.min()) >= R.GAP_SWEEP, (hav, seed, nb)
                    assert (rows.h > 0).all() and rows.members.sum(1).min() >= nb


def test_compute_acc_batch_on_a_stand_in_prior(golden):
    name, case = "euclidean_C33", "euclidean_C33_q1_nb7"
    s, q, classes, labels, img = (golden[name + k] for k in ("_s", "_q", "_classes", "_labels", "_img"))
    hp = dict(kde_dist_type="euclidean", kde_quant=1.0, kde_nb=7)
    B, C = len(q), 33
    split = (np.arange(B) % 3 == 0).astype(np.int64)
    log = logging.getLogger("kde-test")
    assert "kde" in csp_eval.BASELINE_PRIORS and csp_eval.UNSUPPORTED_PRIORS == ("kde", "tang_et_al")
    prior = K.NumpyKdePrior(s, classes, C, hp)
    pred, acc = csp_eval.compute_acc_batch(img, labels, split, val_feats=q, prior_type="kde", prior=prior, batch_size=10,
                                           logger=log, return_acc=True)
    ranks = golden[case + "_ranks"]
    want_acc = {sid: {k: round(int((ranks[split == sid] <= k).sum()) * 100 / int((split == sid).sum()), 2) for k in csp_eval.TOP_KS}
                for sid in (0, 1)}
    assert [int(c) for c in pred] == golden[case + "_argmax"].tolist() and acc == want_acc and len(pred) == B and prior.calls == 4
    # location only: the reference's priors give the same predictions as the stand-in's
    pred = csp_eval.compute_acc_batch(None, labels, split, val_feats=q, prior_type="kde", prior=prior, logger=log)
    assert [int(c) for c in pred] == np.argmax(golden[case + "_prior"], axis=1).tolist()
    with pytest.raises(NotImplementedError, match="kde"):
        csp_eval.compute_acc_batch(img, labels, split, val_feats=q, prior_type="kde", prior=None, logger=log)
    with pytest.raises(NotImplementedError, match="tang_et_al"):
        csp_eval.compute_acc_batch(img, labels, split, val_feats=q, prior_type="tang_et_al", prior=prior, logger=log)
    with pytest.raises(ValueError, match="val_feats"):
        csp_eval.compute_acc_batch(img, labels, split, prior_type="kde", prior=prior, logger=log)


def test_bindings_declare_the_kde_entry_points():
    from range_amd import _neighbors_native as nn
    header = open(os.path.join(REPO, "include", "range_neighbors.h")).read()
    assert set(re.findall(r"\b(range_(?:set_)?kde[a-z0-9_]*)\s*\(", header)) == set(nn.KDE_SYMBOLS)
    assert "#define RANGE_KDE_MAX_CLASSES 16384" in header and nn.KDE_MAX_CLASSES == 16384
    assert "#define RANGE_ABI_VERSION 9" in open(os.path.join(REPO, "include", "range_hip.h")).read()
    lib = nn.load_library()
    for name in nn.KDE_SYMBOLS:
        assert hasattr(lib, name)
    p = nn.kde_plan(24000, 436000, 8142, 436000)
    assert p["group"] == 2 and p["groups"] == 12000 and p["chunks"] == 1 and p["ws_bytes"] == 0 and p["scale_bits"] == 43
    assert nn.kde_plan(9, 1000, 33, 1000)["group"] == 8 and nn.kde_plan(9, 1000, 33, 1000, chunks=3)["chunks"] == 3
    assert nn.kde_plan(1, 1, 16384, 1)["lds_bytes"] <= 160 * 1024 and nn.kde_plan(5, 5, 3, 2 ** 31 - 1)["scale_bits"] == 31
    for total in (1, 300, 1024, 436000):
        assert nn.kde_plan(1, 1, 1, total)["scale_bits"] == K.scale_bits(total)
    for bad in ((0, 5, 3, 5), (5, 0, 3, 5), (5, 5, 16385, 5), (5, 5, 3, 4), (5, 5, 3, 2 ** 31)):
        with pytest.raises(nn.RangeNativeError):
            nn.kde_plan(*bad)


def test_kde_prior_refuses_without_a_gpu_or_with_bad_arguments():
    s = R.random_locs(20, 1)
    hp = dict(kde_quant=1.0, kde_nb=3, kde_dist_type="euclidean")
    with pytest.raises(RuntimeError, match="GPU only"):
        gb.KdePrior(s, np.zeros(20, dtype=np.int64), 3, hp, device="cpu")
    with pytest.raises(ValueError, match="train_locs"):
        gb.KdePrior(np.zeros((0, 2)), np.zeros(0, dtype=np.int64), 3, hp, device="cpu")


def test_kde_plan_under_sanitizers(tmp_path):
    """host_plan.h: kde_plan (tests/native/kde_plan.cpp) compiled with g++ under AddressSanitizer and
    UndefinedBehaviorSanitizer and run on the CPU."""
    exe = str(tmp_path / "kde_plan")
    src = os.path.join(REPO, "tests", "native", "kde_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    src, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "kde_plan ok" in p.stdout, p.stdout + p.stderr
