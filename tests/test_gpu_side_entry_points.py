"""GPU tests of the host side of the side encoders' entry points (posenc_host.h, csp_host.h, checker_host.h), through
the C ABI:

1. Every refusal keeps its return code and its whole text: one call per fault, each refused before anything is
   launched (a bad pointer never reaches a call that would run), against literals of the messages.  Of the composed
   calls only the faults they refuse in front of their first chunk's encoder launch are in the table; what they
   leave to range_csp_head_grid / range_csp_rank_grid is in that entry point's rows.
2. range_csp_predict_rank over more locations than one chunk of the embedding workspace holds: the bits of
   encode-then-rank in all three outputs, with a NaN location and a label outside the head on either side of the
   chunk edge.

Run with ``pytest -m gpu``."""
import os

import numpy as np
import pytest
import torch

import csp_head_refs as H
import csp_refs as R
from range_amd import _native, csp, posenc
from refusal_table import RefusalTable
from tools import synth

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
KIND = {"gridcell": posenc.KIND_GRID, "theory": posenc.KIND_THEORY}
PROBS, SUM = _native.CSP_HEAD_PROBS, _native.CSP_HEAD_SUM
NONE, F32, F64 = _native.CSP_IMG_NONE, _native.CSP_IMG_F32, _native.CSP_IMG_F64

NULL = "null argument"
B_MSG = "B must be > 0"
NO_NET = "no CSP network set (range_set_csp)"
NO_HEAD = "no CSP class head set (range_set_csp_head)"
ENC_ALIGN = "lonlat_dev must be 8-byte aligned, out_dev 4-byte aligned"
HEAD_ALIGN = "the device pointers must be 4-byte aligned"
RANK_ALIGN = "the device pointers must be aligned to their element"
RANK_CAPS = "max_grid and col_parts must be >= 0"
NEAR_ALIGN = "the device pointers must be 8-byte aligned"


def install_width(eng, K):
    eng.set_csp(posenc.KIND_GRID, np.ones(1), [K], [np.zeros((K, 4), dtype=np.float32)], [np.zeros(K, dtype=np.float32)],
                [None], [None], 1, False, False)


def test_refusals_keep_code_and_text():
    bare, headless, eng = (_native.HipEngine(DEV) for _ in range(3))       # no network; a network; network and head
    install_width(headless, 24)
    install_width(eng, 24)
    eng.set_csp_head(np.zeros((5, 24), dtype=np.float32))
    lib, h = eng.lib, eng._h
    alive = []

    def z(shape, dtype):
        alive.append(torch.zeros(shape, dtype=dtype, device=DEV))
        assert alive[-1].data_ptr() % 16 == 0
        return alive[-1].data_ptr()

    x, q, out = z((4, 24), torch.float32), z((4, 2), torch.float64), z((4, 5), torch.float32)
    ids, labels = z((2,), torch.int32), z((4,), torch.int32)
    g, t, a = (z((4,), torch.int32) for _ in range(3))
    img32, img64 = z((4, 5), torch.float32), z((4, 5), torch.float64)
    feat, sup = z((4, 64), torch.float64), z((4, 2), torch.float64)
    idx, dist = z((4,), torch.int64), z((4,), torch.float64)
    freq = np.ones(2)
    fp = freq.ctypes.data
    table = RefusalTable()                # (every refusal of these entry points is RANGE_ERR_INVALID)
    rows = table.rows

    rows("range_posenc_features", [h, posenc.KIND_THEORY, fp, 2, q, 4, feat, None],
         ("ctx", {0: None}, NULL), ("freq", {2: None}, NULL), ("lonlat", {4: None}, NULL), ("out", {6: None}, NULL),
         ("kind -1", {1: -1}, "positional encoder kind -1"), ("kind 6", {1: 6}, "positional encoder kind 6"),
         ("F 0", {3: 0}, "F = 0 frequencies (1 .. 64)"), ("F 65", {3: 65}, "F = 65 frequencies (1 .. 64)"),
         ("B 0", {5: 0}, B_MSG), ("out + 8", {6: feat + 8}, "out_dev must be 16-byte aligned"))
    rows("range_csp_encode_grid", [h, q, 4, x, 0, None],
         ("ctx", {0: None}, NULL), ("lonlat", {1: None}, NULL), ("out", {3: None}, NULL), ("no network", {0: bare._h}, NO_NET),
         ("B 0", {2: 0}, B_MSG), ("max_grid -1", {4: -1}, "max_grid must be >= 0"),
         ("lonlat + 4", {1: q + 4}, ENC_ALIGN), ("out + 2", {3: x + 2}, ENC_ALIGN))
    rows("range_csp_head_grid", [h, x, 4, None, 5, PROBS, out, 0, None],
         ("ctx", {0: None}, NULL), ("feats", {1: None}, NULL), ("out", {6: None}, NULL),
         ("no head", {0: headless._h}, NO_HEAD), ("no network", {0: bare._h}, NO_HEAD),
         ("B 0", {2: 0}, B_MSG), ("M 0", {4: 0}, "M must be > 0"), ("max_grid -1", {7: -1}, "max_grid must be >= 0"),
         ("mode 3", {5: 3}, "mode 3"), ("mode -1", {5: -1}, "mode -1"),
         ("SUM with ids", {3: ids, 4: 2, 5: SUM}, "SUM runs over all classes: no class ids"),
         ("M 4 of 5", {4: 4}, "M = 4 without class ids: the head has 5 classes"),
         ("feats + 2", {1: x + 2}, HEAD_ALIGN), ("out + 2", {6: out + 2}, HEAD_ALIGN), ("ids + 2", {3: ids + 2, 4: 1}, HEAD_ALIGN))
    rows("range_csp_predict", [h, q, 4, None, 5, PROBS, out, None],
         ("ctx", {0: None}, NULL), ("lonlat", {1: None}, NULL), ("out", {6: None}, NULL),
         ("no head", {0: headless._h}, NO_HEAD), ("no network", {0: bare._h}, NO_HEAD),
         ("B 0", {2: 0}, B_MSG), ("M 0", {4: 0}, "M must be > 0"), ("mode 3", {5: 3}, "mode 3"),
         ("lonlat + 4", {1: q + 4}, ENC_ALIGN))
    rows("range_csp_rank_grid", [h, x, 4, img32, F32, labels, g, t, a, 0, 0, None],
         ("ctx", {0: None}, NULL), ("labels", {5: None}, NULL), ("greater", {6: None}, NULL), ("tied_after", {7: None}, NULL),
         ("argmax", {8: None}, NULL), ("no head", {0: headless._h}, NO_HEAD),
         ("no input", {1: None, 3: None, 4: NONE}, "neither embeddings nor image predictions"),
         ("img_kind 3", {4: 3}, "img_kind 3"), ("img_kind -1", {4: -1}, "img_kind -1"),
         ("img with NONE", {4: NONE}, "img_kind 0 with image predictions"),
         ("F32 without img", {3: None}, "img_kind 1 without image predictions"),
         ("B 0", {2: 0}, B_MSG), ("max_grid -1", {9: -1}, RANK_CAPS), ("col_parts -1", {10: -1}, RANK_CAPS),
         ("col_parts 2 of 1", {10: 2}, "B = 4, col_parts = 2: col_parts above the number of chunks"),
         ("feats + 2", {1: x + 2}, RANK_ALIGN), ("labels + 2", {5: labels + 2}, RANK_ALIGN), ("greater + 2", {6: g + 2}, RANK_ALIGN),
         ("tied_after + 2", {7: t + 2}, RANK_ALIGN), ("argmax + 2", {8: a + 2}, RANK_ALIGN), ("img + 2", {3: img32 + 2}, RANK_ALIGN),
         ("float64 img + 4", {3: img64 + 4, 4: F64}, RANK_ALIGN))
    rows("range_csp_predict_rank", [h, q, 4, img32, F32, labels, g, t, a, None],
         ("ctx", {0: None}, NULL), ("lonlat", {1: None}, NULL), ("labels", {5: None}, NULL), ("greater", {6: None}, NULL),
         ("tied_after", {7: None}, NULL), ("argmax", {8: None}, NULL), ("no head", {0: headless._h}, NO_HEAD),
         ("B 0", {2: 0}, B_MSG), ("img_kind 3", {4: 3}, "img_kind 3"),
         ("img with NONE", {4: NONE}, "img_kind 0 with image predictions"),
         ("F32 without img", {3: None}, "img_kind 1 without image predictions"),
         ("lonlat + 4", {1: q + 4}, ENC_ALIGN))
    rows("range_nearest_support", [h, q, 4, sup, 4, 0, 0, idx, dist, None],
         ("ctx", {0: None}, NULL), ("q", {1: None}, NULL), ("sup", {3: None}, NULL), ("idx", {7: None}, NULL),
         ("Q 0", {2: 0}, "Q and S must be > 0"), ("S 0", {4: 0}, "Q and S must be > 0"),
         ("max_chunks -1", {6: -1}, "max_chunks must be >= 0"),
         ("exclude_self, Q != S", {4: 3, 5: 1},
          "exclude_self needs the same Q = S >= 2 points on both sides (Q = 4, S = 3)"),
         ("q + 4", {1: q + 4}, NEAR_ALIGN), ("sup + 4", {3: sup + 4}, NEAR_ALIGN), ("idx + 4", {7: idx + 4}, NEAR_ALIGN),
         ("dist + 4", {8: dist + 4}, NEAR_ALIGN))
    assert len(table) == 88
    table.check(lib)
    torch.cuda.synchronize()


def test_predict_rank_past_one_chunk():
    enc_golden, head_golden = (np.load(os.path.join(GOLDEN, f)) for f in ("csp_encoders.npz", "csp_head.npz"))
    head = H.case_head(enc_golden, head_golden, "theory")
    net = R.case_network(enc_golden, head["enc_case"])
    eng = _native.HipEngine(DEV)
    widths = [w.shape[0] for w in net["weights"]]
    eng.set_csp(KIND[net["spa_enc_type"]], net["freq_list"], widths, net["weights"], net["biases"], net["ln_gamma"],
                net["ln_beta"], csp.ACTIVATIONS[net["act"]], net["skip"], net["use_layn"])
    eng.set_csp_head(head["W"])
    C, chunk = 33, 65536
    assert eng.csp_classes == C and widths[-1] == 256          # 2^24 / 256 = 65536 rows a chunk
    B = chunk + 70
    nan_rows, bad_row = [100, chunk + 5], chunk + 1
    rng = np.random.default_rng(4242)
    q = synth.make_queries(B, seed=96, lat_max=89.9)
    q[nan_rows] = [np.nan, 10.0]
    labels = rng.integers(0, C, size=B).astype(np.int32)
    labels[bad_row] = C
    img = rng.random((B, C))
    qd = torch.from_numpy(q).to(DEV)
    ld = torch.from_numpy(labels).to(DEV)
    feats = eng.csp_encode(qd)
    plain = np.ones(B, dtype=bool)
    plain[nan_rows + [bad_row]] = False
    for gd in (None, torch.from_numpy(img.astype(np.float32)).to(DEV), torch.from_numpy(img).to(DEV)):
        want = [v.cpu().numpy() for v in eng.csp_rank(feats, ld, gd)]
        # a call that ranked its second chunk with the first chunk's labels or image predictions could not pass
        assert not np.array_equal(want[0][chunk:chunk + 70], want[0][:70])
        got = [v.cpu().numpy() for v in eng.csp_predict_rank(qd, ld, gd)]
        for w, g in zip(want, got):
            assert g.dtype == np.int32 and np.array_equal(g, w)
            assert (g[nan_rows] == -1).all() and g[bad_row] == -2 and (g[plain] >= 0).all()
