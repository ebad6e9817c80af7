"""The CSP evaluation, CPU side (no GPU): the numpy restatement (tests/csp_rank_refs.py) against the ranks recorded
from the reference's probabilities (tests/golden/csp_rank.npz, written by make_golden_csp_rank.py), the rank rule,
NaN rule and flags on hand-made matrices, range_amd/csp_eval.py (``get_label_rank``, ``compute_acc_batch`` on a
numpy stand-in prior), planted defects, the launch plan under the host sanitizers, the refusals.

The interval: the restatement's probabilities are exact; the reference's float32 ones are within E_ref <= delta / 4
of them (delta = csp_head_refs.gpu_bound 'probs'), so the reference's s_c - s_t is within delta (img_c + img_t) of
the restatement's and its recorded rank lies in [1 + lo, 1 + hi] on EVERY finite row.  Fixture condition: lo == hi
on at least 90 % of a case's finite rows."""
import logging
import os
import subprocess

import numpy as np
import pytest

import csp_head_refs as H
import csp_rank_refs as K
from range_amd import csp_eval

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")


@pytest.fixture(scope="module")
def enc_golden():
    return np.load(os.path.join(GOLDEN, "csp_encoders.npz"))


@pytest.fixture(scope="module")
def head_golden():
    return np.load(os.path.join(GOLDEN, "csp_head.npz"))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "csp_rank.npz"))


@pytest.fixture(scope="module")
def restated(enc_golden, head_golden, golden):
    """Per case: the head, its inputs, the exact probabilities, delta, the interval - computed once."""
    out = {}
    for case in H.CASES:
        head = H.case_head(enc_golden, head_golden, case)
        img, labels = K.case_inputs(golden, case, head)
        p64 = H.probs(head["feats"], head["W"])
        delta = K.case_delta(head_golden, case, head)
        lo, hi = K.rank_interval(p64, img, labels, delta)
        out[case] = dict(head=head, img=img, labels=labels, p64=p64, delta=delta, lo=lo, hi=hi,
                         finite=H.finite_rows(head["feats"]))
    return out


@pytest.mark.parametrize("case", list(H.CASES))
def test_recorded_ranks_inside_the_interval(golden, restated, case):
    r = restated[case]
    fin, lo, hi, ranks = r["finite"], r["lo"], r["hi"], golden[case + "_ranks"]
    assert fin.sum() == 21 and (ranks[~fin] == 0).all() and (golden[case + "_argmax"][~fin] == -1).all()
    assert ((1 + lo[fin] <= ranks[fin]) & (ranks[fin] <= 1 + hi[fin])).all()          # every finite row
    decided = fin & (lo == hi)
    print(f"{case}: delta {r['delta']:.3e}, decided {int(decided.sum())} of {int(fin.sum())} finite rows, "
          f"widest interval {int((hi - lo)[fin].max())}")
    assert decided.sum() >= K.MIN_DECIDED * fin.sum()
    # on decided rows the restatement's own rank (the rule on its exact scores) is the recorded one
    g, e, a = K.rank_rule(r["p64"] * (1.0 if r["img"] is None else r["img"].astype(np.float64)), r["labels"])
    assert np.array_equal(K.ranks_of(g, e)[decided], ranks[decided])
    am = fin & K.argmax_decided(r["p64"], r["img"], r["delta"])
    assert am.sum() >= 0.5 * fin.sum() and np.array_equal(a[am], golden[case + "_argmax"][am])
    assert np.array_equal(golden[case + "_topk"], K.topk_counts(ranks))


HAND = np.array([[0.5, 0.25, 0.5, 0.125, 0.5],         # ties of the maximum
                 [0.0, 0.0, 0.0, 0.0, 0.0],            # all equal
                 [0.1, np.nan, 0.3, np.nan, 0.2],      # NaN entries beside the label
                 [0.1, np.nan, 0.3, 0.2, 0.0],         # the label's score is NaN (label 1)
                 [-np.inf, -np.inf, -np.inf, -np.inf, -np.inf],
                 [0.1, 0.2, 0.3, 0.4, 0.5]])
HAND_LABELS = np.array([2, 3, 0, 1, 4, 7])


def test_rule_on_hand_made_rows():
    for fn in (K.rank_rule, csp_eval.rank_counts):
        g, e, a = (np.asarray(v).astype(np.int64) for v in fn(HAND, HAND_LABELS))
        # row 0: label 2 ties with 0 and 4; only 4 comes after it -> rank 2; np.argmax is the first maximum
        assert (g[0], e[0], a[0]) == (0, 1, 0)
        assert (g[1], e[1], a[1]) == (0, 1, 0)              # label 3 of five equal scores: one after it
        assert (g[2], e[2], a[2]) == (4, 0, 1)              # two NaN and two larger; the first NaN is the arg-max
        assert (g[3], e[3], a[3]) == (-1, -1, -1)           # NaN score of the label
        assert (g[4], e[4], a[4]) == (0, 0, 0)              # all -inf: label 4 is last among ties, arg-max 0
        assert (g[5], e[5], a[5]) == (-2, -2, -2)           # label outside [0, C)
    ok = np.array([0, 1, 2, 4])
    assert np.array_equal(K.ranks_of(*K.rank_rule(HAND, HAND_LABELS)[:2])[ok], [2, 2, 5, 1])
    # the stable double argsort of eval_helper.py, reversed, is the rule (NaN rows included)
    assert np.array_equal(K.stable_argsort_ranks(HAND[ok], HAND_LABELS[ok]), [2, 2, 5, 1])
    assert np.array_equal(np.argmax(HAND[ok], axis=1), [0, 0, 1, 0])


def test_rule_is_the_reference_argsort_on_tie_free_rows():
    rng = np.random.default_rng(11)
    s = rng.random((40, 97))
    labels = rng.integers(0, 97, size=40)
    assert K.tie_free(s).all()
    g, e, a = K.rank_rule(s, labels)
    assert (e == 0).all() and np.array_equal(1 + g, K.argsort_ranks(s, labels))
    assert np.array_equal(a, np.argmax(s, axis=1))
    assert np.array_equal(csp_eval.get_label_rank(s, labels), K.argsort_ranks(s, labels))
    # with ties: the stable form
    s = np.round(s * 8) / 8
    assert not K.tie_free(s).any()
    assert np.array_equal(csp_eval.get_label_rank(s, labels), K.stable_argsort_ranks(s, labels))
    assert np.array_equal(csp_eval.get_label_rank(s.astype(np.float32), labels), K.stable_argsort_ranks(s, labels))


def test_get_label_rank_flags():
    r = csp_eval.get_label_rank(HAND[:5], HAND_LABELS[:5])
    assert r.dtype == np.int64 and np.array_equal(r, [2, 2, 5, 0, 1])
    with pytest.raises(ValueError, match="labels outside"):
        csp_eval.get_label_rank(HAND, HAND_LABELS)
    with pytest.raises(ValueError):
        csp_eval.rank_counts(HAND, HAND_LABELS[:3])


@pytest.mark.parametrize("defect", K.DEFECTS)
def test_planted_defects_fail(defect):
    """Each planted mistake changes an output on rows made for it."""
    if defect == "f32_product":
        # (1 + 2^-23)(1 - 2^-24) = 1 + 2^-24 - 2^-47 > 1 in float64, and rounds to 1 in float32
        p = np.array([[1.0 + 2.0 ** -23, 1.0]], dtype=np.float32)
        img = np.array([[1.0 - 2.0 ** -24, 1.0]], dtype=np.float32)
        assert img[0, 0] < 1.0
        labels = np.array([1])
        good = K.rank_rule(K.scores(p, img), labels)
        bad = K.rank_rule(K.scores(p, img, defect), labels)
        assert (good[0][0], good[1][0], good[2][0]) == (1, 0, 0) and (bad[0][0], bad[1][0]) == (0, 0)
        return
    good, bad = K.rank_rule(HAND[:2], HAND_LABELS[:2]), K.rank_rule(HAND[:2], HAND_LABELS[:2], defect)
    assert any(not np.array_equal(x, y) for x, y in zip(good, bad)), defect
    which = {"ge": 0, "ties_before": 1, "last_argmax": 2}[defect]
    assert not np.array_equal(good[which], bad[which])


class ListLogger:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(str(msg))


def test_compute_acc_batch_on_a_stand_in_prior():
    """Two splits, dropped rows (a NaN location): the reference's denominators - the whole split."""
    rng = np.random.default_rng(5)
    N, C = 50, 12
    prior32 = rng.random((N, C)).astype(np.float32)
    img = rng.random((N, C)).astype(np.float32)
    img[rng.random((N, C)) < 0.1] = 0.0
    labels = rng.integers(0, C, size=N)
    split = (np.arange(N) % 3 == 0).astype(np.int64) + 1          # split ids 1 and 2
    coords = np.stack([np.arange(N, dtype=np.float64), np.zeros(N)], 1)
    dropped = np.array([3, 4, 30])
    coords[dropped, 0] = np.nan
    prior = K.NumpyPrior(prior32)
    log = ListLogger()
    pred, acc = csp_eval.compute_acc_batch(img, labels, split, val_feats=coords, prior_type="geo_net", prior=prior,
                                           batch_size=16, logger=log, eval_flag_str="LocEnc ", return_acc=True)
    assert prior.calls == 4
    kept = np.setdiff1d(np.arange(N), dropped)
    s = prior32[kept].astype(np.float64) * img[kept].astype(np.float64)
    ranks = K.stable_argsort_ranks(s, labels[kept])
    assert [int(c) for c in pred] == np.argmax(s, axis=1).tolist() and len(pred) == N - 3
    for sid in (1, 2):
        members = np.flatnonzero(split == sid)
        in_kept = np.isin(kept, members)
        for k in csp_eval.TOP_KS:
            assert acc[sid][k] == round(int((ranks[in_kept] <= k).sum()) * 100 / len(members), 2)
    # the reference's lines
    assert log.lines[0] == str((N - 3,)) and log.lines[1] == " Split ID: 0" and log.lines[6] == " Split ID: 1"
    assert log.lines[2] == " Top 1\tLocEnc acc (%):   {}".format(acc[1][1]) and len(log.lines) == 11
    # without return_acc: the reference's return value; the model's spa_enc_type as prior_type; no image predictions
    again = csp_eval.compute_acc_batch(img, labels, split, val_feats=coords, prior_type="gridcell", prior=prior,
                                       logger=log)
    assert [int(c) for c in again] == [int(c) for c in pred]
    loc_only = csp_eval.compute_acc_batch(None, labels, split, val_feats=coords, prior_type="geo_net", prior=prior,
                                          logger=log)
    assert [int(c) for c in loc_only] == np.argmax(prior32[kept], axis=1).tolist()
    # 'no_prior': the image predictions alone, no row dropped
    pred0, acc0 = csp_eval.compute_acc_batch(img, labels, split, prior_type="no_prior", logger=log, return_acc=True,
                                             batch_size=7)
    r0 = K.stable_argsort_ranks(img.astype(np.float64), labels)
    assert [int(c) for c in pred0] == np.argmax(img, axis=1).tolist()
    assert acc0[2][3] == round(int((r0[split == 2] <= 3).sum()) * 100 / int((split == 2).sum()), 2)
    # a default logger
    csp_eval.compute_acc_batch(img, labels, split, prior_type="no_prior")


def test_compute_acc_batch_refusals():
    img, labels, split = np.ones((4, 3), dtype=np.float32), np.zeros(4, dtype=np.int64), np.ones(4)
    for name in csp_eval.UNSUPPORTED_PRIORS + ("theory",):
        with pytest.raises(NotImplementedError, match=name):
            csp_eval.compute_acc_batch(img, labels, split, prior_type=name, prior=None, logger=logging.getLogger("t"))
    with pytest.raises(NotImplementedError, match="theory"):
        csp_eval.compute_acc_batch(img, labels, split, val_feats=np.zeros((4, 2)), prior_type="theory",
                                   prior=K.NumpyPrior(img, "gridcell"))
    with pytest.raises(ValueError, match="val_preds"):
        csp_eval.compute_acc_batch(None, labels, split, prior_type="no_prior")
    with pytest.raises(ValueError, match="val_feats"):
        csp_eval.compute_acc_batch(img, labels, split, prior_type="geo_net", prior=K.NumpyPrior(img))
    with pytest.raises(ValueError, match="outside"):
        csp_eval.compute_acc_batch(img, labels + 3, split, prior_type="no_prior")


def test_bindings_declare_the_rank_entry_points():
    from range_amd import _native
    for name in ("range_csp_rank", "range_csp_rank_grid", "range_csp_predict_rank"):
        assert name in _native.SYMBOLS
    header = open(os.path.join(REPO, "include", "range_hip.h")).read()
    for name, value in (("NONE", 0), ("F32", 1), ("F64", 2)):
        assert f"#define RANGE_CSP_IMG_{name} {value}" in header and getattr(_native, "CSP_IMG_" + name) == value
    assert "#define RANGE_ABI_VERSION 9" in header          # entry points added, none changed


def test_csp_rank_plan_under_sanitizers(tmp_path):
    """host_plan.h: csp_rank_plan (tests/native/csp_rank_plan.cpp) compiled with g++ under AddressSanitizer and
    UndefinedBehaviorSanitizer and run on the CPU."""
    exe = str(tmp_path / "csp_rank_plan")
    src = os.path.join(REPO, "tests", "native", "csp_rank_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    src, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "csp_rank_plan ok" in p.stdout, p.stdout + p.stderr
