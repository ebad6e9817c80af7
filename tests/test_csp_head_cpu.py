"""The CSP class head, CPU side (no GPU): the checkpoint reader's ``class_head=True``, the launch plan and the
packing under the host sanitizers, the numpy float64 restatement the GPU tests compare the kernel with
(tests/csp_head_refs.py) against the reference's recorded float32 outputs (tests/golden/csp_head.npz, written
by make_golden_csp_head.py), and range_amd/grid_predictor.py on a numpy stand-in for ``loc_model``.

E_ref per case and output kind is measured HERE from the fixture; the GPU tests' bound is csp_head_refs.gpu_bound
(4 * max(E_ref, 2^-23 max|out|); for the sums C times that of the probabilities plus the float32 additions).
What E_ref itself may be is float32 arithmetic's: a dot product of K terms formed in float32 in any order is
within K 2^-24 sum|x_k w_k| of the exact one (to first order; the factor 1.01 covers the rest), the sigmoid has
slope <= 1/4 and is rounded (2^-24) after an expf of a few ulp (<= 4 2^-24 in all), and a float32 sum of C terms
in [0, 1] adds at most (C - 1) 2^-24 times the sum."""
import os
import subprocess

import numpy as np
import pytest
import torch

import csp_head_refs as H
import csp_refs as R
from range_amd import csp, grid_predictor
from tools import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


@pytest.fixture(scope="module")
def enc_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "csp_encoders.npz"))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "csp_head.npz"))


@pytest.fixture(scope="module")
def heads(enc_golden, golden):
    return {c: H.case_head(enc_golden, golden, c) for c in H.CASES}


def test_fixture(golden, heads):
    want = {"design": (256, 8142), "c_odd": (24, 5), "theory": (256, 33), "d_nohidden": (50, 1), "e_square": (24, 24)}
    assert {c: (h["settings"]["num_filts"], h["C"]) for c, h in heads.items()} == want
    d = heads["design"]["settings"]
    assert (d["spa_enc_type"], d["F"], d["hidden"]) == ("gridcell", 32, 512)
    for c, h in heads.items():
        cols, classes, C = h["cols"], h["classes"], h["C"]
        rows = H.finite_rows(h["feats"])
        assert rows[:21].all() and not rows[21:].any()
        assert golden[c + "_probs"].shape == (24, len(cols)) and golden[c + "_probs"].dtype == np.float32
        assert golden[c + "_single"].shape == golden[c + "_logits"].shape == (24, len(classes))
        assert golden[c + "_sums"].shape == (24,)
        assert 0 in classes and C - 1 in classes and (np.diff(cols) > 0).all() and cols[0] == 0 and cols[-1] == C - 1
        for k in H.KINDS:
            a = golden[f"{c}_{k}"]
            assert np.isfinite(a[rows]).all() and np.isnan(a[~rows]).all(), (c, k)
        # the saturation condition: a quarter of the recorded probabilities away from 0 and 1
        for k in ("probs", "single"):
            p = golden[f"{c}_{k}"][rows]
            assert ((p >= 0.05) & (p <= 0.95)).mean() >= 0.25, (c, k)
    cols = heads["design"]["cols"]
    P = H.DESIGN_COLS_PER_PASS
    assert set(range(40)) | set(range(8142 - 40, 8142)) <= set(cols)
    assert all(m - 1 in cols and m in cols for m in range(P, 8142, P)) and len(cols) < 200
    assert golden["grid_map"].shape == H.GRID_SHAPE == golden["grid_mask"].shape
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "csp_head.npz")) < 1 << 20


def _rewrite(path, edit):
    ck = torch.load(path, weights_only=False)
    edit(ck)
    torch.save(ck, path)
    return path


def test_reader(tmp_path):
    base = dict(spa_enc_type="gridcell", F=4, hidden=16, layers=1, act="relu", use_layn=True, skip=True, num_filts=8,
                num_classes=7, class_scale=0.5)
    path = synth.write_csp_checkpoint(str(tmp_path / "m.pth.tar"), **base)
    sd = torch.load(path, weights_only=False)["state_dict"]
    plain = csp.read_csp_checkpoint(path)
    assert plain.class_emb is None and plain.num_classes == 0
    assert csp.read_csp_checkpoint(path, class_head=False).class_emb is None
    p = csp.read_csp_checkpoint(path, class_head=True)
    assert p.num_classes == 7 and p.class_emb.dtype == np.float32 and p.class_emb.shape == (7, 8)
    assert np.array_equal(p.class_emb, sd["loc_enc.class_emb.weight"].numpy())
    # everything else is what the plain read gives
    assert p.widths == plain.widths and all(np.array_equal(a, b) for a, b in zip(p.weights, plain.weights))
    # class_scale scales class_emb alone
    sd1 = synth.make_csp_checkpoint(**dict(base, class_scale=1.0))["state_dict"]
    assert np.array_equal(sd1["loc_enc.class_emb.weight"].numpy() * np.float32(0.5), p.class_emb)
    assert all(torch.equal(sd1[k], sd[k]) for k in sd if "class_emb" not in k)
    assert sd["class_emb.weight"] is not None and torch.equal(sd["class_emb.weight"], sd["loc_enc.class_emb.weight"])


def test_reader_refusals(tmp_path):
    base = dict(spa_enc_type="gridcell", F=4, hidden=16, layers=1, act="relu", use_layn=True, skip=True, num_filts=8,
                num_classes=7)
    path = str(tmp_path / "m.pth.tar")
    key = "loc_enc.class_emb.weight"
    synth.write_csp_checkpoint(path, **base)
    _rewrite(path, lambda ck: ck["state_dict"].pop(key))
    with pytest.raises(ValueError, match="class_emb.weight: missing"):
        csp.read_csp_checkpoint(path, class_head=True)
    assert csp.read_csp_checkpoint(path).class_emb is None              # the plain read never looks at the head
    synth.write_csp_checkpoint(path, **base)
    _rewrite(path, lambda ck: ck["state_dict"].update({"loc_enc.class_emb.bias": torch.zeros(7)}))
    with pytest.raises(ValueError, match="class_emb.bias"):
        csp.read_csp_checkpoint(path, class_head=True)
    synth.write_csp_checkpoint(path, **base)
    _rewrite(path, lambda ck: ck["params"].update(num_classes=6))
    with pytest.raises(ValueError, match="class_emb.weight: shape"):
        csp.read_csp_checkpoint(path, class_head=True)
    synth.write_csp_checkpoint(path, **base)
    _rewrite(path, lambda ck: ck["state_dict"].update({key: ck["state_dict"][key].t().contiguous()}))
    with pytest.raises(ValueError, match="class_emb.weight: shape"):
        csp.read_csp_checkpoint(path, class_head=True)
    synth.write_csp_checkpoint(path, **base)
    _rewrite(path, lambda ck: ck["state_dict"].update({key: ck["state_dict"][key].double()}))
    with pytest.raises(ValueError, match="float32"):
        csp.read_csp_checkpoint(path, class_head=True)
    for bad in (0, 32769):
        synth.write_csp_checkpoint(path, **dict(base, num_classes=bad))
        with pytest.raises(ValueError, match="num_classes.*supported"):
            csp.read_csp_checkpoint(path, class_head=True)
        assert csp.read_csp_checkpoint(path).num_classes == 0
    synth.write_csp_checkpoint(path, **dict(base, num_classes=32768))
    assert csp.read_csp_checkpoint(path, class_head=True).class_emb.shape == (32768, 8)


def test_class_head_option_is_for_csp(tmp_path):
    from range_amd.load_model import load_model
    with pytest.raises(ValueError, match="class_head"):
        load_model("Wrap", pretrained_path="unused", class_head=True)


def test_csp_head_plan_under_sanitizers(tmp_path):
    """host_plan.h: csp_head_plan / csp_pack_head / csp_predict_chunk (tests/native/csp_head_plan.cpp) compiled with
    g++ under AddressSanitizer and UndefinedBehaviorSanitizer and run on the CPU."""
    exe = str(tmp_path / "csp_head_plan")
    src = os.path.join(REPO, "tests", "native", "csp_head_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    src, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "csp_head_plan ok" in p.stdout, p.stdout + p.stderr
    for width, chunk in ((256, 65536), (257, 65280), (1024, 16384)):
        assert f"csp_predict_chunk({width}) = {chunk}\n" in p.stdout, p.stdout


def float32_limits(head, kind):
    """What float32 arithmetic allows E_ref(kind) to be (the module's docstring)."""
    rows = H.finite_rows(head["feats"])
    x, W = np.abs(head["feats"][rows].astype(np.float64)), np.abs(head["W"].astype(np.float64))
    K = x.shape[1]
    ids = {"probs": head["cols"], "single": head["classes"], "logits": head["classes"], "sums": np.arange(head["C"])}[kind]
    dot = 1.01 * K * U * float((x @ W[ids].T).max())
    if kind == "logits":
        return dot
    per_prob = dot / 4.0 + 4.0 * U
    if kind != "sums":
        return per_prob
    C = head["C"]
    return C * per_prob + 1.01 * (C - 1) * U * C


@pytest.mark.parametrize("kind", H.KINDS)
@pytest.mark.parametrize("case", list(H.CASES))
def test_restatement_against_the_reference(golden, heads, case, kind):
    """The reference's float32 outputs lie within float32 arithmetic's reach of the float64 restatement; NaN
    rows agree.  (DESIGN.md 3.6c records the E_ref values.)"""
    head = heads[case]
    got, ref = H.restated(head, kind), golden[f"{case}_{kind}"]
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref))
    e, lim = H.e_ref(golden, case, head, kind), float32_limits(head, kind)
    print(f"{case} {kind}: E_ref = {e:.3e} (float32 allows {lim:.3e}), max|out| = {float(np.nanmax(np.abs(ref))):.4f}, "
          f"GPU bound {H.gpu_bound(golden, case, head, kind):.3e}")
    assert e <= lim


def test_grid_restatement(enc_golden, golden, heads):
    """The 7 x 12 map, from the coordinates: the encoder's restatement at the grid points, then the head."""
    head = heads[H.GRID_CASE]
    net = R.case_network(enc_golden, head["enc_case"])
    lon, lat = H.grid_coords(*H.GRID_SHAPE)
    assert np.array_equal(lon, golden["grid_lon"]) and np.array_equal(lat, golden["grid_lat"])
    e = H.grid_e_ref(golden, net, head)
    # the embedding's own E_ref (csp_refs) passes through at most sum|w| of the class's row, then slope 1/4
    emb_e = R.e_ref(enc_golden, head["enc_case"], net)
    lim = float32_limits(head, "single") + 0.25 * float(np.abs(head["W"][H.GRID_CLASS]).sum()) * 4.0 * emb_e
    print(f"grid: E_ref = {e:.3e} (allowed {lim:.3e}), bound {H.grid_bound(golden, net, head):.3e}")
    assert e <= lim
    assert np.array_equal(H.mask_lines(golden["grid_mask"]), golden["grid_mask_lines"])


APPLIES = {"bias": ("probs", "single", "logits", "sums"), "no_sigmoid": ("probs", "single", "sums"),
           "sigmoid_in_eval": ("logits",), "row_plus": ("probs", "single", "logits"), "row_minus": ("probs", "single", "logits"),
           "transposed": ("probs", "single", "logits", "sums"), "sum_padded": ("sums",)}


@pytest.mark.parametrize("defect", H.DEFECTS)
def test_a_planted_defect_exceeds_the_gpu_bound(golden, heads, defect):
    """The bounds the GPU tests use discriminate: on the fixture every defect moves every output kind it touches
    further from the restatement than a kernel may be - in every case where it changes anything at all (a head
    of one class has no class c + 1, only a square class_emb can be read transposed)."""
    assert set(APPLIES) == set(H.DEFECTS)
    seen = 0
    for case, head in heads.items():
        rows = H.finite_rows(head["feats"])
        if defect in ("row_plus", "row_minus") and head["C"] == 1:
            continue
        if defect == "transposed" and head["C"] != head["settings"]["num_filts"]:
            continue
        for kind in APPLIES[defect]:
            err = float(np.abs(H.restated(head, kind, defect) - H.restated(head, kind))[rows].max())
            bound = H.gpu_bound(golden, case, head, kind)
            print(f"{defect} {case} {kind}: {err:.3e} / bound {bound:.3e} = {err / bound:.3g}")
            assert err > bound, (defect, case, kind, err, bound)
            seen += 1
    assert seen


def test_grid_defects_exceed_the_bound(enc_golden, golden, heads):
    head = heads[H.GRID_CASE]
    net = R.case_network(enc_golden, head["enc_case"])
    Hh, Ww = H.GRID_SHAPE
    clean, bound = H.grid_map(net, head["W"], H.GRID_CLASS, Hh, Ww), H.grid_bound(golden, net, head)
    for defect in ("bias", "no_sigmoid", "row_plus", "row_minus"):
        assert float(np.abs(H.grid_map(net, head["W"], H.GRID_CLASS, Hh, Ww, defect) - clean).max()) > bound, defect
    # a transposed or flipped grid is caught too
    assert float(np.abs(clean[::-1] - clean).max()) > bound and float(np.abs(clean[:, ::-1] - clean).max()) > bound


class NumpyLocModel:
    """A stand-in for ``model.loc_model`` with a class head: the float64 restatement behind the call forms
    GridPredictor uses."""

    def __init__(self, net, W):
        self.net, self.W, self.num_classes, self.calls = net, W, W.shape[0], []

    def _emb(self, coords):
        assert torch.is_tensor(coords) and coords.dtype == torch.float64 and coords.shape[1] == 2
        self.calls.append(coords.shape[0])
        return R.encode(self.net, coords.numpy()).astype(np.float32)

    def __call__(self, coords, class_of_interest=None, return_feats=True):
        assert return_feats is False and isinstance(class_of_interest, int)
        return torch.from_numpy(H.probs(self._emb(coords), self.W, [class_of_interest])[:, 0].astype(np.float32))

    def class_sum(self, coords):
        return torch.from_numpy(H.sums(self._emb(coords), self.W).astype(np.float32))


def test_grid_predictor_on_the_cpu(enc_golden, golden, heads, monkeypatch):
    head = heads[H.GRID_CASE]
    net = R.case_network(enc_golden, head["enc_case"])
    mask = golden["grid_mask"]
    Hh, Ww = mask.shape
    stand_in = NumpyLocModel(net, head["W"])
    gp = grid_predictor.GridPredictor(mask, stand_in, mask_only_pred=True)
    # the grid: the reference's float32 coordinates widened, rows from 90 down, columns from -180 up
    assert gp.feats.dtype == np.float64 and gp.feats.shape == (Hh, Ww, 2)
    assert np.array_equal(gp.feats[3, :, 0], golden["grid_lon"]) and np.array_equal(gp.feats[:, 5, 1], golden["grid_lat"])
    assert gp.feats[0, 0].tolist() == [-180.0, 90.0] and gp.feats[-1, -1].tolist() == [180.0, -90.0]
    assert np.array_equal(gp.feats, gp.feats.astype(np.float32).astype(np.float64))
    assert np.array_equal(gp.mask_lines, golden["grid_mask_lines"])
    bound = H.grid_bound(golden, net, head)
    raw = gp.dense_prediction(H.GRID_CLASS, mask_op=False)
    assert raw.dtype == np.float32 and raw.shape == (Hh, Ww)
    assert float(np.abs(raw.astype(np.float64) - golden["grid_map"]).max()) <= bound
    masked = gp.dense_prediction(H.GRID_CLASS)
    assert np.array_equal(masked, raw * mask + golden["grid_mask_lines"])
    assert float(np.abs(masked - golden["grid_masked"]).max()) <= bound
    s, mx = gp.dense_prediction_sum(mask_op=False)
    assert float(np.abs(s.astype(np.float64) - golden["grid_sum"]).max()) <= H.grid_sum_bound(golden, net, head) and mx == s.max()
    s2, mx2 = gp.dense_prediction_sum()
    assert np.array_equal(s2, s * mask + gp.mask_lines) and mx2 == mx
    only = gp.dense_prediction_masked(H.GRID_CLASS)
    assert only.shape == (Hh, Ww) and only.dtype == np.float32
    assert np.array_equal(only, np.where(mask == 1, raw, np.float32(0)))
    assert 0 < int((mask == 1).sum()) < mask.size and stand_in.calls[-1] == int((mask == 1).sum())
    with pytest.raises(ValueError, match="mask_only_pred"):
        grid_predictor.GridPredictor(mask, stand_in).dense_prediction_masked(0)
    # chunks: at most CHUNK locations a call, the same map
    assert grid_predictor.CHUNK == 1 << 18
    monkeypatch.setattr(grid_predictor, "CHUNK", 10)
    stand_in.calls.clear()
    assert np.array_equal(gp.dense_prediction(H.GRID_CLASS, mask_op=False), raw)
    assert stand_in.calls == [10] * 8 + [4]
