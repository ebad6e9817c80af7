"""GPU tests of the CSP evaluation kernel (csp_rank_kernel.h; range_csp_rank, range_csp_rank_grid,
range_csp_predict_rank) through the C ABI, and of its Python surface.

1. Exact self-consistency: the three outputs equal, bit for bit, the counts formed on the host
   (csp_rank_refs.rank_rule) from the head's own PROBS matrix of the same embeddings, with
   ``p32.astype(f64) * img.astype(f64)`` - every row, at the smallest shapes that reach every edge.
2. The same bits with col_parts 1, 2 and the maximum, a grid cap of 1 and 3, on another stream, and B = 1 taken
   from a larger batch.
3. range_csp_predict_rank equals encode then rank.
4. The fixture (tests/golden/csp_rank.npz): the kernel's ranks lie inside the restatement's interval on every
   finite row, equal the reference's recorded rank on decided rows; the arg-max equals the reference's on rows
   whose two best scores differ by more than the bound (csp_rank_refs: rank_interval, argmax_decided).
5. ``CspLocationModel.label_ranks`` and ``csp_eval.compute_acc_batch``.

Run with ``pytest -m gpu``."""
import os

import numpy as np
import pytest
import torch

import csp_head_refs as H
import csp_rank_refs as K
import csp_refs as R
from range_amd import _native, csp, csp_eval, posenc
from tools import synth

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
SENTINEL = -777
KIND = {"gridcell": posenc.KIND_GRID, "theory": posenc.KIND_THEORY}
IMG_OF = {np.dtype(np.float32): _native.CSP_IMG_F32, np.dtype(np.float64): _native.CSP_IMG_F64}


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
def heads(enc_golden, head_golden):
    return {c: H.case_head(enc_golden, head_golden, c) for c in H.CASES}


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


def install_width(eng, K_):
    eng.set_csp(posenc.KIND_GRID, np.ones(1), [K_], [np.zeros((K_, 4), dtype=np.float32)], [np.zeros(K_, dtype=np.float32)],
                [None], [None], 1, False, False)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def rank_call(eng, x, img, labels, max_grid=None, col_parts=0, lonlat=False, pad=16):
    """range_csp_rank (``max_grid`` / ``col_parts``: range_csp_rank_grid; ``lonlat``: range_csp_predict_rank on
    coordinates) through ctypes on torch's current stream, into one buffer with ``pad`` sentinels around each of the
    three outputs, which must come back untouched -> (greater, tied_after, argmax) as host arrays."""
    B = labels.shape[0]
    buf = torch.full((3, pad + B + pad), SENTINEL, dtype=torch.int32, device=DEV)
    outs = [buf[i, pad:pad + B] for i in range(3)]
    stream = torch.cuda.current_stream(eng.device).cuda_stream
    kind = _native.CSP_IMG_NONE if img is None else IMG_OF[np.dtype(str(img.dtype).replace("torch.", ""))]
    xp, ip = (None if x is None else x.data_ptr()), (None if img is None else img.data_ptr())
    ptrs = [o.data_ptr() for o in outs]
    if lonlat:
        rc = eng.lib.range_csp_predict_rank(eng._h, xp, B, ip, kind, labels.data_ptr(), *ptrs, stream)
    elif max_grid is None and not col_parts:
        rc = eng.lib.range_csp_rank(eng._h, xp, B, ip, kind, labels.data_ptr(), *ptrs, stream)
    else:
        rc = eng.lib.range_csp_rank_grid(eng._h, xp, B, ip, kind, labels.data_ptr(), *ptrs, max_grid or 0, col_parts, stream)
    assert rc == 0, eng.lib.range_last_error().decode()
    host = buf.cpu().numpy()
    assert (host[:, :pad] == SENTINEL).all() and (host[:, pad + B:] == SENTINEL).all()
    return tuple(host[i, pad:pad + B].copy() for i in range(3))


def probs_of(eng, x):
    return eng.csp_head(x, None, _native.CSP_HEAD_PROBS).cpu().numpy()


def synthetic(K_, C, B, seed, P):
    """Embeddings, a class_emb, image predictions and labels with every special row the rule has: labels at 0, at
    C - 1 and on both sides of every chunk edge; planted zeros; the true class at zero (row 2), an all-zero row
    (3), a NaN image entry beside the label (4) and at it (5), a NaN location row between finite ones (6), a label
    of -1 (7) and of C (8)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, size=(B, K_)).astype(np.float32)
    W = (rng.standard_normal((C, K_)) * (2.0 / np.sqrt(K_))).astype(np.float32)
    z = rng.standard_normal((B, C)) * 2.0
    e = np.exp(z - z.max(1, keepdims=True))
    img = (e / e.sum(1, keepdims=True)).astype(np.float32)
    img[rng.random((B, C)) < 0.1] = 0.0
    labels = rng.integers(0, C, size=B).astype(np.int32)
    edges = sorted({0, C - 1} | {c for m in range(P, C, P) for c in (m - 1, m)})
    labels[9:9 + len(edges)] = edges[:max(0, B - 9)]
    if B > 8:
        img[2, labels[2]] = 0.0
        img[3, :] = 0.0
        img[4, (labels[4] + 1) % C] = np.nan
        img[5, labels[5]] = np.nan
        x[6, :] = np.nan
        labels[7], labels[8] = -1, C
    return x, W, img, labels


def expect(p32, img, labels):
    return tuple(v.astype(np.int32) for v in K.rank_rule(K.scores(p32, img), labels))


def same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("K_", [24, 50, 256, 600])
def test_exact_self_consistency(engine, K_):
    install_width(engine, K_)
    engine.set_csp_head(np.zeros((1, K_), dtype=np.float32))
    P = engine.lib.range_csp_head_cols_per_pass(engine._h)
    Bs = [1, 31, 32, 33, 63, 64, 65, 129]
    for C in [1, 5, 31, 32, 33, 255, 256, 257, 513] + ([8142] if K_ == 256 else []):
        x, W, img, labels = synthetic(K_, C, Bs[-1], seed=3000 + K_ + C, P=P)
        engine.set_csp_head(W)
        xd, ld_ = dev(x, np.float32), dev(labels, np.int32)
        p32 = probs_of(engine, xd)
        assert np.isnan(p32[6]).all() and np.isfinite(np.delete(p32, 6, axis=0)).all()
        f32, f64 = dev(img, np.float32), dev(img, np.float64)
        full = {}
        for name, xx, gg, pp, host_img in (("f32", xd, f32, p32, img), ("f64", xd, f64, p32, img.astype(np.float64)),
                                           ("none", xd, None, p32, None), ("no_prior", None, f32, np.ones_like(p32), img)):
            full[name] = rank_call(engine, xx, gg, ld_)
            want = expect(pp, host_img, labels)
            assert same(full[name], want), (K_, C, name, [np.flatnonzero(g != w)[:5] for g, w in zip(full[name], want)])
        # the flags
        g, e, a = full["f32"]
        assert g[5] == e[5] == a[5] == -1 and g[6] == e[6] == a[6] == -1 and (g[[7, 8]] == -2).all() and (a[[7, 8]] == -2).all()
        assert full["no_prior"][0][6] >= 0 and a[4] == (labels[4] + 1) % C or C == 1
        if C > 1:
            assert e[3] == C - 1 - labels[3] and a[3] == 0 and g[3] == 0       # the all-zero row
        # every smaller B: the same rows
        for B in Bs[:-1]:
            assert same(rank_call(engine, xd[:B], f32[:B], ld_[:B]), [v[:B] for v in full["f32"]]), (K_, C, B)
        if C in (5, 513):
            for B in Bs[:-1]:
                assert same(rank_call(engine, None, f64[:B], ld_[:B]), [v[:B] for v in expect(np.ones_like(p32), img, labels)]), (K_, C, B)


@pytest.mark.parametrize("K_,C", [(256, 513), (600, 1025), (256, 8142)])
def test_same_bits_under_variation(engine, K_, C):
    install_width(engine, K_)
    engine.set_csp_head(np.zeros((1, K_), dtype=np.float32))
    P = engine.lib.range_csp_head_cols_per_pass(engine._h)
    chunks = -(-C // P)
    B = 129
    x, W, img, labels = synthetic(K_, C, B, seed=17 + K_ + C, P=P)
    engine.set_csp_head(W)
    xd, ld_, gd = dev(x, np.float32), dev(labels, np.int32), dev(img, np.float32)
    base = rank_call(engine, xd, gd, ld_, col_parts=1)
    assert same(base, expect(probs_of(engine, xd), img, labels))
    for parts in sorted({1, 2, chunks}):
        for cap in (0, 1, 3):
            assert same(rank_call(engine, xd, gd, ld_, max_grid=cap, col_parts=parts), base), (parts, cap)
            assert same(rank_call(engine, None, gd, ld_, max_grid=cap, col_parts=parts),
                        rank_call(engine, None, gd, ld_, col_parts=1)), (parts, cap)
    assert same(rank_call(engine, xd, gd, ld_), base)                       # the plan's own choice
    with torch.cuda.stream(torch.cuda.Stream(DEV)):
        other = rank_call(engine, xd, gd, ld_)
    torch.cuda.synchronize()
    assert same(other, base)
    for b in (0, 5, 64, 128):
        one = rank_call(engine, xd[b:b + 1], gd[b:b + 1], ld_[b:b + 1])
        assert same(one, [v[b:b + 1] for v in base]), b
    # more parts than chunks, both inputs absent, a kind that does not match: refused
    lib, h = engine.lib, engine._h
    out = torch.zeros((3, B), dtype=torch.int32, device=DEV)
    o = [out[i].data_ptr() for i in range(3)]
    F32, NONE = _native.CSP_IMG_F32, _native.CSP_IMG_NONE
    assert lib.range_csp_rank_grid(h, xd.data_ptr(), B, gd.data_ptr(), F32, ld_.data_ptr(), *o, 0, chunks + 1, None) == -1
    assert b"col_parts" in lib.range_last_error()
    assert lib.range_csp_rank(h, None, B, None, NONE, ld_.data_ptr(), *o, None) == -1
    assert lib.range_csp_rank(h, xd.data_ptr(), B, gd.data_ptr(), NONE, ld_.data_ptr(), *o, None) == -1
    assert lib.range_csp_rank(h, xd.data_ptr(), B, None, F32, ld_.data_ptr(), *o, None) == -1
    assert lib.range_csp_rank(h, xd.data_ptr(), B, gd.data_ptr(), 3, ld_.data_ptr(), *o, None) == -1
    assert lib.range_csp_rank(h, xd.data_ptr(), 0, gd.data_ptr(), F32, ld_.data_ptr(), *o, None) == -1
    assert lib.range_csp_rank(h, xd.data_ptr(), B, gd.data_ptr(), F32, ld_.data_ptr(), None, o[1], o[2], None) == -1
    assert lib.range_csp_rank(h, xd.data_ptr(), B, gd.data_ptr(), F32, None, *o, None) == -1
    torch.cuda.synchronize()
    assert (out == 0).all()


def test_no_head_is_refused(engine):
    fresh = _native.HipEngine(DEV)
    install_width(fresh, 24)
    t = torch.zeros(8, dtype=torch.int32, device=DEV)
    x = torch.zeros((1, 24), dtype=torch.float32, device=DEV)
    assert fresh.lib.range_csp_rank(fresh._h, x.data_ptr(), 1, None, 0, t.data_ptr(), t[1:].data_ptr(), t[2:].data_ptr(),
                                    t[3:].data_ptr(), None) == -1
    assert b"head" in fresh.lib.range_last_error()
    with pytest.raises(_native.RangeNativeError, match="head"):
        fresh.csp_rank(x, t[:1])


@pytest.mark.parametrize("case", list(H.CASES))
def test_fixture_and_composed_call(enc_golden, head_golden, golden, heads, nets, engine, case):
    head = heads[case]
    assert install_net(engine, nets[head["enc_case"]]) == head["W"].shape[1]
    engine.set_csp_head(head["W"])
    img, labels = K.case_inputs(golden, case, head)
    fin = H.finite_rows(head["feats"])
    x, ld_ = dev(head["feats"], np.float32), dev(labels, np.int32)
    gd = None if img is None else dev(img, img.dtype)
    g, e, a = rank_call(engine, x, gd, ld_)
    assert (g[~fin] == -1).all() and (e[~fin] == -1).all() and (a[~fin] == -1).all() and (g[fin] >= 0).all()
    ranks = K.ranks_of(g, e)
    delta = K.case_delta(head_golden, case, head)
    p64 = H.probs(head["feats"], head["W"])
    lo, hi = K.rank_interval(p64, img, labels, delta)
    decided = fin & (lo == hi)
    print(f"{case}: ranks {ranks.tolist()}; recorded {golden[case + '_ranks'].tolist()}; decided {int(decided.sum())} of 21")
    assert ((1 + lo[fin] <= ranks[fin]) & (ranks[fin] <= 1 + hi[fin])).all()
    assert np.array_equal(ranks[decided], golden[case + "_ranks"][decided])
    am = fin & K.argmax_decided(p64, img, delta)
    assert np.array_equal(a[am], golden[case + "_argmax"][am])
    # the composed call on the coordinates: encode, then rank - the same bits
    q = dev(enc_golden["lonlat"], np.float64)
    feats = engine.csp_encode(q)
    two = rank_call(engine, feats, gd, ld_)
    assert same(rank_call(engine, q, gd, ld_, lonlat=True), two)
    assert same(tuple(t.cpu().numpy() for t in engine.csp_predict_rank(q, ld_, gd)), two)
    assert same(tuple(t.cpu().numpy() for t in engine.csp_rank(feats, ld_, gd)), two)


@pytest.fixture(scope="module")
def checkpoints(enc_golden, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("csp_rank_ckpt")
    return {c: synth.write_csp_checkpoint(str(tmp / f"{c}.pth.tar"), **H.case_settings(enc_golden, c)) for c in ("theory", "c_odd")}


@pytest.mark.parametrize("case", ["theory", "c_odd"])
def test_python_surface(enc_golden, golden, heads, checkpoints, case):
    from range_amd import load_model
    head = heads[case]
    model = load_model(head["name"], pretrained_path=checkpoints[case], device=DEV, class_head=True)
    lm = model.loc_model
    img, labels = K.case_inputs(golden, case, head)
    q = enc_golden["lonlat"]
    fin = H.finite_rows(head["feats"])
    # the matrix route, on the model's own probabilities: what label_ranks must equal
    p32 = lm(torch.from_numpy(q), return_feats=False).cpu().numpy()
    g, e, a = K.rank_rule(K.scores(p32, img), labels)
    want_r, want_a = K.ranks_of(g, e), np.where(g < 0, -1, a)
    assert (want_r[~fin] == 0).all() and (want_r[fin] > 0).all()
    lm.img_chunk_bytes = 7 * head["C"] * img.itemsize            # several chunks of rows
    for coords, lab, preds in ((q, labels, img), (torch.from_numpy(q).to(DEV), torch.from_numpy(labels), torch.from_numpy(img)),
                               (torch.from_numpy(q), labels.astype(np.int64), torch.from_numpy(img).to(DEV))):
        r, pc = lm.label_ranks(coords, lab, preds)
        assert r.dtype == pc.dtype == np.int64 and np.array_equal(r, want_r) and np.array_equal(pc, want_a)
    r0, _ = lm.label_ranks(q, labels)
    assert np.array_equal(r0, K.ranks_of(*K.rank_rule(K.scores(p32, None), labels)[:2]))
    # compute_acc_batch against the fixture's top-k counts (the recorded ranks, where the rows are decided)
    split = np.ones(24)
    pred, acc = csp_eval.compute_acc_batch(img, labels, split, val_feats=torch.from_numpy(q), prior_type=lm.spa_enc_type,
                                           prior=lm, batch_size=10, return_acc=True)
    assert [int(c) for c in pred] == want_a[fin].tolist()
    assert [acc[1.0][k] for k in K.TOP_KS] == [round(int(n) * 100 / 24, 2) for n in golden[case + "_topk"]]
    assert csp_eval.compute_acc_batch(img, labels, split, val_feats=q, prior_type="geo_net", prior=lm) == pred
    # refusals
    with pytest.raises(ValueError, match="float32 or float64"):
        lm.label_ranks(q, labels, img.astype(np.float16))
    with pytest.raises(ValueError, match="float32 or float64"):
        lm.label_ranks(q, labels, torch.from_numpy(img).to(torch.bfloat16))
    with pytest.raises(ValueError, match="labels outside"):
        lm.label_ranks(q, np.where(np.arange(24) == 3, head["C"], labels), img)
    with pytest.raises(ValueError, match="img_preds must be"):
        lm.label_ranks(q, labels, img[:, :-1] if head["C"] > 1 else img[:-1])
    with pytest.raises(NotImplementedError, match="rbf"):
        csp_eval.compute_acc_batch(img, labels, split, val_feats=q, prior_type="rbf", prior=lm)
    plain = load_model(head["name"], pretrained_path=checkpoints[case], device=DEV).loc_model
    with pytest.raises(NotImplementedError, match="class_head=True"):
        plain.label_ranks(q, labels, img)
    with pytest.raises(NotImplementedError, match="class_head=True"):
        csp_eval.compute_acc_batch(img, labels, split, val_feats=q, prior_type="geo_net", prior=plain)
