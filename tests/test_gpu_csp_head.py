"""GPU tests of the CSP class head (csp_head_kernel.h; range_set_csp_head, range_csp_head, range_csp_predict):
the kernel through the C ABI against the numpy float64 restatement (tests/csp_head_refs.py, whose distance to
the reference's recorded float32 outputs tests/test_csp_head_cpu.py measures from tests/golden/csp_head.npz),
the edges of its tiling, bit-for-bit independence of a column from B, the grid, the stream and the other
columns of the call, the fused predict call, the refusals, and the model with ``class_head=True``.

Bound per fixture case and output kind: csp_head_refs.gpu_bound - 4 * max(E_ref, 2^-23 max|out|), for the sums C
times that of the probabilities plus (C - 1) 2^-24 sum|p|.  A head the fixture does not hold (the edge shapes)
takes the same rule with E_ref measured on torch's float32 CPU operators - the operators the reference's head is
made of.  Run with ``pytest -m gpu``."""
import os

import numpy as np
import pytest
import torch

import csp_head_refs as H
import csp_refs as R
from range_amd import _native, csp, posenc
from tools import synth

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
SENTINEL = -12345.678
KIND = {"gridcell": posenc.KIND_GRID, "theory": posenc.KIND_THEORY}
PROBS, LOGITS, SUM = _native.CSP_HEAD_PROBS, _native.CSP_HEAD_LOGITS, _native.CSP_HEAD_SUM
U = 2.0 ** -24


@pytest.fixture(scope="module")
def enc_golden():
    return np.load(os.path.join(GOLDEN, "csp_encoders.npz"))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "csp_head.npz"))


@pytest.fixture(scope="module")
def heads(enc_golden, golden):
    return {c: H.case_head(enc_golden, golden, c) for c in H.CASES}


@pytest.fixture(scope="module")
def nets(enc_golden):
    return {c: R.case_network(enc_golden, c) for c in set(H.CASES.values())}


@pytest.fixture(scope="module")
def engine():
    return _native.HipEngine(DEV)


def install_net(eng, net):
    widths = [w.shape[0] for w in net["weights"]]
    eng.set_csp(KIND[net["spa_enc_type"]], net["freq_list"], widths, net["weights"], net["biases"], net["ln_gamma"],
                net["ln_beta"], csp.ACTIVATIONS[net["act"]], net["skip"], net["use_layn"])
    return widths[-1]


def install_width(eng, K):
    """The smallest network of ``K`` outputs (one layer on 4 features): the head only needs its num_filts."""
    eng.set_csp(posenc.KIND_GRID, np.ones(1), [K], [np.zeros((K, 4), dtype=np.float32)], [np.zeros(K, dtype=np.float32)],
                [None], [None], 1, False, False)


def install_head(eng, W):
    eng.set_csp_head(W)
    assert eng.lib.range_csp_classes(eng._h) == W.shape[0] == eng.csp_classes
    return eng.lib.range_csp_head_cols_per_pass(eng._h)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def head_call(eng, x, mode, ids=None, max_grid=None, lonlat=False, pad=64):
    """range_csp_head (``max_grid``: range_csp_head_grid; ``lonlat``: range_csp_predict on coordinates) through
    ctypes, on torch's current stream, into a buffer with ``pad`` sentinel floats before and after the output,
    which must come back untouched -> the (B, M) - for SUM (B,) - result as a host array."""
    B, C = x.shape[0], eng.lib.range_csp_classes(eng._h)
    M = C if ids is None else ids.shape[0]
    n = B if mode == SUM else B * M
    buf = torch.full((pad + n + pad,), SENTINEL, dtype=torch.float32, device=DEV)
    out = buf[pad:pad + n]
    stream = torch.cuda.current_stream(eng.device).cuda_stream
    ip = None if ids is None else ids.data_ptr()
    if lonlat:
        rc = eng.lib.range_csp_predict(eng._h, x.data_ptr(), B, ip, M, mode, out.data_ptr(), stream)
    elif max_grid is None:
        rc = eng.lib.range_csp_head(eng._h, x.data_ptr(), B, ip, M, mode, out.data_ptr(), stream)
    else:
        rc = eng.lib.range_csp_head_grid(eng._h, x.data_ptr(), B, ip, M, mode, out.data_ptr(), max_grid, stream)
    assert rc == 0, eng.lib.range_last_error().decode()
    host = buf.cpu().numpy()
    assert (host[:pad] == np.float32(SENTINEL)).all() and (host[pad + n:] == np.float32(SENTINEL)).all()
    res = host[pad:pad + n].copy()
    return res if mode == SUM else res.reshape(B, M)


@pytest.mark.parametrize("case", list(H.CASES))
def test_fixture_cases_within_the_bound(golden, heads, nets, engine, case):
    """PROBS, LOGITS and SUM on the reference's recorded embeddings against the restatement; the NaN rows."""
    head = heads[case]
    assert install_net(engine, nets[head["enc_case"]]) == head["W"].shape[1]
    P = install_head(engine, head["W"])
    if case == "design":
        assert P == H.DESIGN_COLS_PER_PASS          # the fixture's stored columns sit around its multiples
    x = dev(head["feats"], np.float32)
    rows = H.finite_rows(head["feats"])
    cols, classes = head["cols"], head["classes"]
    full = {PROBS: head_call(engine, x, PROBS), LOGITS: head_call(engine, x, LOGITS)}
    got = {"probs": full[PROBS][:, cols], "single": full[PROBS][:, classes], "logits": full[LOGITS][:, classes],
           "sums": head_call(engine, x, SUM)}
    for kind in H.KINDS:
        g, ref = got[kind], golden[f"{case}_{kind}"]
        assert g.dtype == np.float32 and g.shape == ref.shape
        # NaN embeddings: NaN where the reference's rows are, the neighbours untouched
        assert np.isnan(g[~rows]).all() and np.isfinite(g[rows]).all() and np.array_equal(np.isnan(g), np.isnan(ref))
        err = float(np.abs(g[rows].astype(np.float64) - H.restated(head, kind)[rows]).max())
        bound = H.gpu_bound(golden, case, head, kind)
        print(f"{case} {kind}: max|gpu - restatement| = {err:.3e}, E_ref = {H.e_ref(golden, case, head, kind):.3e}, "
              f"bound = {bound:.3e}, max|gpu - reference| = {float(np.abs(g[rows] - ref[rows]).max()):.3e}")
        assert err <= bound
    assert np.isnan(full[PROBS][~rows]).all() and np.isfinite(full[PROBS][rows]).all()
    # one class at a time, as class_of_interest asks: the full call's column, bit for bit
    for c in classes:
        one = head_call(engine, x, PROBS, ids=dev([c], np.int32))
        assert np.array_equal(one[:, 0], full[PROBS][:, c], equal_nan=True), c


def synthetic(K, C, B, seed):
    """Embeddings in [-1, 1] and a class_emb that keeps the logits within a few units."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, size=(B, K)).astype(np.float32)
    W = (rng.standard_normal((C, K)) * (2.0 / np.sqrt(K))).astype(np.float32)
    return x, W


def torch_bounds(x, W):
    """The rule of the fixture cases with E_ref from torch's float32 CPU operators -> {mode: (restatement, bound)}."""
    xt, Wt = torch.from_numpy(x), torch.from_numpy(W)
    z32 = torch.nn.functional.linear(xt, Wt)
    p32 = torch.sigmoid(z32)
    z64, p64, s64 = H.logits(x, W), H.probs(x, W), H.sums(x, W)
    C = W.shape[0]
    bz = 4.0 * max(float(np.abs(z32.numpy() - z64).max()), 2.0 ** -23 * float(np.abs(z64).max()))
    bp = 4.0 * max(float(np.abs(p32.numpy() - p64).max()), 2.0 ** -23 * float(np.abs(p64).max()))
    return {LOGITS: (z64, bz), PROBS: (p64, bp), SUM: (s64, C * bp + (C - 1) * U * float(s64.max()))}


@pytest.mark.parametrize("K", [24, 50, 256, 600])
def test_edges_of_the_tiling(engine, K):
    """Rows around the tile height, classes around the column tile and the columns of a pass (read from the
    plan), a num_filts that is no multiple of 8, the 32-row tile of a network wider than 512: within the bound
    at the largest B, and every smaller B the same rows bit for bit."""
    install_width(engine, K)
    T = engine.lib.range_csp_tile_rows(engine._h)
    assert T == (32 if K > 512 else 64)
    install_head(engine, np.zeros((1, K), dtype=np.float32))
    P = engine.lib.range_csp_head_cols_per_pass(engine._h)
    assert P in (256, 512, 1024) and P % 128 == 0
    Bs = sorted({1, 63, 64, 65, 129} | ({31, 32, 33} if K > 512 else set()))
    for C in (1, 31, 32, 33, P - 1, P, P + 1, 2 * P + 1):
        x, W = synthetic(K, C, Bs[-1], seed=1000 + K + C)
        assert install_head(engine, W) == P
        want = torch_bounds(x, W)
        xd = dev(x, np.float32)
        full = {}
        for mode in (PROBS, LOGITS, SUM):
            full[mode] = head_call(engine, xd, mode)
            err = float(np.abs(full[mode].astype(np.float64) - want[mode][0]).max())
            assert err <= want[mode][1], (K, C, mode, err, want[mode][1])
        for B in Bs[:-1]:
            for mode in (PROBS, SUM):
                assert np.array_equal(head_call(engine, xd[:B], mode), full[mode][:B]), (K, C, B, mode)


@pytest.mark.parametrize("K", [256, 600])
def test_bit_for_bit(engine, K):
    """A column's bits do not depend on the other columns of the call (subsets: one id, 33 ids, unsorted, with a
    repeat), on B, on the stream or on the grid."""
    install_width(engine, K)
    P = install_head(engine, np.zeros((1, K), dtype=np.float32))
    C, B = 2 * P + 1, 129
    x, W = synthetic(K, C, B, seed=7 + K)
    install_head(engine, W)
    xd = dev(x, np.float32)
    full = {m: head_call(engine, xd, m) for m in (PROBS, LOGITS, SUM)}
    rng = np.random.default_rng(8)
    unsorted = rng.permutation(C)[:33]
    assert (np.diff(unsorted) < 0).any()
    subsets = [np.array([C - 1]), np.array([P]), unsorted, np.array([5, P + 1, 5, 0, C - 1, P - 1, 5]),
               rng.integers(0, C, size=P + 40)]
    for ids in subsets:
        idd = dev(ids, np.int32)
        for m in (PROBS, LOGITS):
            sub = head_call(engine, xd, m, ids=idd)
            assert sub.shape == (B, len(ids)) and np.array_equal(sub, full[m][:, ids]), (m, ids[:8])
    for i in (0, 64, 128):
        for m in (PROBS, LOGITS):
            assert np.array_equal(head_call(engine, xd[i:i + 1], m), full[m][i:i + 1]), (i, m)
        assert np.array_equal(head_call(engine, xd[i:i + 1], PROBS, ids=dev([P], np.int32))[:, 0], full[PROBS][i:i + 1, P])
        assert np.array_equal(head_call(engine, xd[i:i + 1], SUM), full[SUM][i:i + 1])
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        on_side = {m: head_call(engine, xd, m) for m in (PROBS, LOGITS, SUM)}
    side.synchronize()
    for cap in (1, 3, 0):
        for m in (PROBS, LOGITS, SUM):
            assert np.array_equal(head_call(engine, xd, m, max_grid=cap), full[m]), (cap, m)
            assert np.array_equal(on_side[m], full[m])
        assert np.array_equal(head_call(engine, xd, PROBS, ids=dev(unsorted, np.int32), max_grid=cap), full[PROBS][:, unsorted])


def test_chunk_groups_same_bits(engine):
    """From about 2048 work items on, a work item takes several chunks of columns behind one load of its X tile
    (the plan's chunks_per_item): the same bits as the calls small enough to take one chunk an item."""
    K = 24
    install_width(engine, K)
    P = install_head(engine, np.zeros((1, K), dtype=np.float32))
    C, B = 2 * P + 1, 64 * 1024 + 1            # 1025 row tiles x 2 groups of the 3 chunks >= 2048 items
    x, W = synthetic(K, C, B, seed=11)
    install_head(engine, W)
    xd = dev(x, np.float32)
    want = torch_bounds(x[-256:], W)
    for mode in (PROBS, LOGITS):
        big = engine.csp_head(xd, mode=mode)
        assert big.shape == (B, C)
        for i in range(0, B, 8192):
            assert torch.equal(engine.csp_head(xd[i:i + 8192], mode=mode), big[i:i + 8192]), (mode, i)
        assert float(np.abs(big[-256:].cpu().numpy().astype(np.float64) - want[mode][0]).max()) <= want[mode][1]


def test_predict_is_encode_then_head(heads, nets, engine):
    """range_csp_predict = range_csp_encode into the workspace, then range_csp_head: the same bits, also over
    more locations than one chunk of the workspace (65536) holds; with an identity class_emb its LOGITS are the
    embedding itself."""
    head = heads["theory"]
    install_net(engine, nets[head["enc_case"]])
    install_head(engine, head["W"])
    B = 65536 + 70
    q = synth.make_queries(B, seed=95, lat_max=89.9)
    q[100] = [np.nan, 10.0]
    qd = dev(q, np.float64)
    emb = engine.csp_encode(qd)
    ids = dev([7, 32, 0], np.int32)
    for mode, idd in ((PROBS, ids), (LOGITS, ids), (SUM, None), (PROBS, None)):
        n = B if idd is not None or mode == SUM else 300          # (all 33 columns: a slice is enough)
        got = head_call(engine, qd[:n], mode, ids=idd, lonlat=True)
        assert np.array_equal(got, head_call(engine, emb[:n], mode, ids=idd), equal_nan=True), mode
        assert np.isnan(got[100]).all() and np.isfinite(got[99]).all() and np.isfinite(got[101]).all()
    net = nets["c_odd"]
    K = install_net(engine, net)
    install_head(engine, np.eye(K, dtype=np.float32))
    emb = engine.csp_encode(qd[:200]).cpu().numpy()
    assert np.array_equal(head_call(engine, qd[:200], LOGITS, lonlat=True), emb, equal_nan=True)


def test_refusals(heads, nets, engine):
    lib = engine.lib
    fresh = _native.HipEngine(DEV)
    x = torch.zeros((4, 24), dtype=torch.float32, device=DEV)
    q = torch.zeros((4, 2), dtype=torch.float64, device=DEV)
    out = torch.zeros((4 * 5 + 4,), dtype=torch.float32, device=DEV)
    ids = dev([1, 2], np.int32)
    W = heads["c_odd"]["W"]
    # no network: no head; a network without a head: no classes, every head call refused
    assert lib.range_csp_classes(fresh._h) == 0 and lib.range_csp_classes(None) == 0 and lib.range_csp_head_cols_per_pass(fresh._h) == 0
    assert lib.range_set_csp_head(fresh._h, W.ctypes.data, 5) == -1 and b"range_set_csp" in lib.range_last_error()
    install_net(fresh, nets["c_odd"])
    assert lib.range_csp_classes(fresh._h) == 0
    assert lib.range_csp_head(fresh._h, x.data_ptr(), 4, None, 5, PROBS, out.data_ptr(), None) == -1
    assert b"no CSP class head" in lib.range_last_error()
    assert lib.range_csp_predict(fresh._h, q.data_ptr(), 4, None, 5, PROBS, out.data_ptr(), None) == -1
    with pytest.raises(_native.RangeNativeError, match="no CSP class head"):
        fresh.csp_head(x)
    # the envelope and the shape
    for C in (0, -1, 32769):
        assert lib.range_set_csp_head(fresh._h, W.ctypes.data, C) == -1
    with pytest.raises(ValueError, match="class_emb"):
        fresh.set_csp_head(np.zeros((5, 25), dtype=np.float32))
    assert lib.range_set_csp_head(fresh._h, None, 5) == -1 and lib.range_set_csp_head(None, W.ctypes.data, 5) == -1
    fresh.set_csp_head(W)
    h = fresh._h
    assert lib.range_csp_classes(h) == 5
    ok = [x.data_ptr(), 4, None, 5, PROBS, out.data_ptr()]
    assert lib.range_csp_head(h, *ok, None) == 0
    for i, bad in ((0, None), (0, x.data_ptr() + 2), (1, 0), (1, -3), (3, 0), (3, -1), (3, 4), (4, 3), (4, -1), (5, None),
                   (5, out.data_ptr() + 2)):
        a = list(ok)
        a[i] = bad
        assert lib.range_csp_head(h, *a, None) == -1, (i, bad)
    assert lib.range_csp_head(None, *ok, None) == -1
    assert lib.range_csp_head_grid(h, *ok, -1, None) == -1
    assert lib.range_csp_head(h, x.data_ptr(), 4, ids.data_ptr(), 2, SUM, out.data_ptr(), None) == -1     # SUM with ids
    assert b"SUM" in lib.range_last_error()
    assert lib.range_csp_head(h, x.data_ptr(), 4, ids.data_ptr(), 0, PROBS, out.data_ptr(), None) == -1    # M < 1
    assert lib.range_csp_head(h, x.data_ptr(), 4, ids.data_ptr(), 2, PROBS, out.data_ptr(), None) == 0
    assert lib.range_csp_predict(h, None, 4, None, 5, PROBS, out.data_ptr(), None) == -1
    assert lib.range_csp_predict(h, q.data_ptr(), 4, None, 5, PROBS, None, None) == -1
    assert lib.range_csp_predict(h, q.data_ptr(), 0, None, 5, PROBS, out.data_ptr(), None) == -1
    assert lib.range_csp_predict(h, q.data_ptr(), 4, ids.data_ptr(), 2, SUM, out.data_ptr(), None) == -1
    assert lib.range_csp_predict(h, q.data_ptr(), 4, None, 5, PROBS, out.data_ptr(), None) == 0
    # ids that come from the host are validated against the head
    for bad in ([5], [0, -1], [2, 3, 70000]):
        with pytest.raises(_native.RangeNativeError, match="class id"):
            fresh.csp_head(x, ids=bad)
        with pytest.raises(_native.RangeNativeError, match="class id"):
            fresh.csp_predict(q, ids=torch.tensor(bad))
    with pytest.raises(ValueError, match="class ids"):
        fresh.csp_head(x, ids=[[1, 2]])
    with pytest.raises(ValueError, match="class ids"):
        fresh.csp_head(x, ids=[0.5])
    with pytest.raises(ValueError, match="SUM"):
        fresh.csp_head(x, ids=[1], mode=SUM)
    assert fresh.csp_head(x, ids=[4, 0]).shape == (4, 2) and fresh.csp_head(x, mode=SUM).shape == (4,)
    # range_set_csp drops the head: it belongs to the network it was installed behind
    install_net(fresh, nets["c_odd"])
    assert lib.range_csp_classes(h) == 0 and lib.range_csp_head(h, *ok, None) == -1
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def checkpoints(enc_golden, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("csp_head_ckpt")
    return {c: synth.write_csp_checkpoint(str(tmp / f"{c}.pth.tar"), **H.case_settings(enc_golden, c)) for c in ("theory", "c_odd")}


def test_model_with_the_class_head(enc_golden, golden, heads, nets, checkpoints, engine):
    from range_amd import load_model
    from range_amd.grid_predictor import GridPredictor
    head = heads["theory"]
    net, W, C = nets[head["enc_case"]], head["W"], head["C"]
    model = load_model(head["name"], pretrained_path=checkpoints["theory"], device=DEV, class_head=True)
    lm = model.loc_model
    d = torch.device(DEV)
    assert lm.num_classes == C == 33 and model.location_feature_dim == 256
    sd = lm.state_dict()
    key = "loc_enc.class_emb.weight"
    assert key in sd and sd[key].dtype == torch.float32 and sd[key].device == d and np.array_equal(sd[key].cpu().numpy(), W)
    assert {k for k in sd if "ffn" not in k} == {key} and not lm.loc_enc.class_emb.weight.requires_grad
    q = enc_golden["lonlat"]
    rows = H.finite_rows(head["feats"])
    for coords in (torch.from_numpy(q), torch.from_numpy(q).to(DEV)):
        emb = lm(coords)
        assert emb.shape == (24, 256) and emb.dtype == torch.float32 and emb.device == d
        assert torch.equal(model(coords)[:21], emb[:21]) and torch.equal(lm(coords, return_feats=True)[:21], emb[:21])
        p = lm(coords, return_feats=False)
        assert p.shape == (24, C) and p.dtype == torch.float32 and p.device == d
        assert torch.isnan(p[21:]).all() and torch.isfinite(p[:21]).all()
        for k in (7, torch.tensor(7), np.int64(7)):
            one = lm(coords, class_of_interest=k, return_feats=False)
            assert one.shape == (24,) and one.dtype == torch.float32 and one.device == d
            assert torch.equal(one[:21], p[:21, 7])
        for ids in ([7, 0, 32, 7], torch.tensor([7, 0, 32, 7]), torch.tensor([7, 0, 32, 7], device=DEV), np.array([7, 0, 32, 7])):
            some = lm(coords, class_of_interest=ids, return_feats=False)
            assert some.shape == (24, 4) and some.dtype == torch.float32 and torch.equal(some[:21], p[:21][:, [7, 0, 32, 7]])
        s = lm.class_sum(coords)
        assert s.shape == (24,) and s.dtype == torch.float32 and s.device == d and torch.isnan(s[21:]).all()
        # the head on the engine's own embedding: within the fixture's bound of the restatement ON that embedding
        e32 = emb.cpu().numpy()
        err = float(np.abs(p.cpu().numpy()[rows].astype(np.float64) - H.probs(e32[rows], W)).max())
        assert err <= H.gpu_bound(golden, "theory", head, "probs"), err
        assert float(np.abs(s.cpu().numpy()[rows].astype(np.float64) - H.sums(e32[rows], W)).max()) <= \
            H.gpu_bound(golden, "theory", head, "sums")
        # eval_single_class: raw logits of given embeddings, the C ABI's LOGITS bit for bit
        z = lm.eval_single_class(emb, 7)
        assert z.shape == (24,) and z.dtype == torch.float32 and z.device == d
        want = head_call(model.engine, emb, LOGITS, ids=dev([7], np.int32))[:, 0]
        assert np.array_equal(z.cpu().numpy(), want, equal_nan=True)
        assert float(np.abs(z.cpu().numpy()[rows].astype(np.float64) - H.eval_single_class(e32[rows], W, [7])[:, 0]).max()) <= \
            H.gpu_bound(golden, "theory", head, "logits")
        assert lm.eval_single_class(emb, [7, 3]).shape == (24, 2)
    with pytest.raises(_native.RangeNativeError, match="class id"):
        lm(torch.from_numpy(q), class_of_interest=C, return_feats=False)
    empty = lm(torch.empty((0, 2), dtype=torch.float64), return_feats=False)
    assert empty.shape == (0, C) and empty.dtype == torch.float32
    # the range map of the fixture
    mask = golden["grid_mask"]
    gp = GridPredictor(mask, lm, mask_only_pred=True)
    raw = gp.dense_prediction(H.GRID_CLASS, mask_op=False)
    bound = H.grid_bound(golden, net, head)
    err = float(np.abs(raw.astype(np.float64) - H.grid_map(net, W, H.GRID_CLASS, *H.GRID_SHAPE)).max())
    print(f"grid: max|gpu - restatement| = {err:.3e}, bound = {bound:.3e}, "
          f"max|gpu - reference| = {float(np.abs(raw - golden['grid_map']).max()):.3e}")
    assert raw.shape == H.GRID_SHAPE and raw.dtype == np.float32 and err <= bound
    coords = torch.from_numpy(gp.feats.reshape(-1, 2))
    direct = lm(coords, class_of_interest=H.GRID_CLASS, return_feats=False).cpu().numpy()
    assert np.array_equal(raw, direct.reshape(H.GRID_SHAPE))
    assert np.array_equal(gp.dense_prediction(H.GRID_CLASS), raw * mask + golden["grid_mask_lines"])
    s, mx = gp.dense_prediction_sum(mask_op=False)
    assert np.array_equal(s, lm.class_sum(coords).cpu().numpy().reshape(H.GRID_SHAPE)) and mx == s.max()
    assert float(np.abs(s.astype(np.float64) - H.grid_sums(net, W, *H.GRID_SHAPE)).max()) <= H.grid_sum_bound(golden, net, head)
    s2, _ = gp.dense_prediction_sum()
    assert np.array_equal(s2, s * mask + gp.mask_lines)
    assert np.array_equal(gp.dense_prediction_masked(H.GRID_CLASS), np.where(mask == 1, raw, np.float32(0)))
    # 'CSP_INat' takes the option too
    inat = load_model("CSP_INat", pretrained_path=checkpoints["c_odd"], device=DEV, class_head=True)
    assert inat.loc_model.num_classes == 5 and inat.loc_model(torch.from_numpy(q), return_feats=False).shape == (24, 5)


def test_model_without_the_option(checkpoints):
    from range_amd import load_model
    model = load_model("CSP", pretrained_path=checkpoints["theory"], device=DEV)
    lm = model.loc_model
    q = torch.zeros((3, 2), dtype=torch.float64)
    assert lm.num_classes == 0 and not any("class_emb" in k for k in lm.state_dict())
    assert model.engine.csp_classes == 0
    for call in (lambda: lm(q, return_feats=False), lambda: lm(q, class_of_interest=1, return_feats=False),
                 lambda: lm.class_sum(q), lambda: lm.eval_single_class(lm(q), 1)):
        with pytest.raises(NotImplementedError, match="class_head=True"):
            call()
    assert lm(q).shape == (3, 256) and lm(q, None, True).shape == (3, 256)
