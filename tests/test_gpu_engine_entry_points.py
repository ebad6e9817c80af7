"""GPU tests of the host side of the retrieval engine's entry points (encoder_host.h, bank_host.h, scan_host.h,
topk_host.h, forward_host.h), through the C ABI:

1. Every refusal that one bad argument or one missing piece of state reaches before anything is launched with it
   keeps its return code and its whole text: one call per fault, against literals of the messages.  No row passes
   a bad device pointer to a call that would launch; the calls whose refusals reset state of the context (pass 1
   forgets the kept logits, range_forward* / range_encode_raw the workspace's queries) run on contexts whose
   state no other row reads.
2. What a forward call refused BEHIND its encoder launch leaves in the context: range_forward does not claim the
   workspace's e-hat for range_topk_last, range_forward_host does.

The state is tiny: the L = 10, H = 64 synthetic encoder, a 40-row bank, 70 queries (two query tiles, one of them
partial) scanned once with keep_logits.  Run with ``pytest -m gpu``."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import range_oracle as O
from range_amd import _native
from refusal_table import STATE, RefusalTable
from tools import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L, H, N, B = 10, 64, 40, 70
PLUS = _native.MODEL_RANGE_PLUS

NULL = "null argument"
B_MSG = "B must be > 0"
NO_ENC = "encoder not set (range_set_encoder)"
NO_BANK = "bank not set (range_set_bank)"
KEYS_ONLY = "keys-only bank (range_set_keys): only range_topk_stream runs on it"
NO_KEPT = "no kept logits (range_scan_stats with keep_logits)"
BETA = "beta must be in [0,1]"
ROWS_MSG = "n_rows must be > 0"
PARTS_B = "n_parts and B must be > 0"
B_OR_K = "bad B or k"
KEPT_70 = "queries [64, 71) exceed the 70 kept"
KEYS_NORM = ("bank keys are not L2-normalised or not finite (largest row norm 2.0002): the softmax of range_scan_stats / "
             "range_attend needs unit keys, as range/range.py:85-89 prepares them (range_topk_stream accepts any norm)")
XYZ_NORM = ("bank locations are not unit vectors or not finite (largest row norm 2.0000): the geographic softmax needs "
            "them as range/utils/utils.py:11-16 computes them")


def taus(sem, geo):
    return (f"temperatures must be finite, > 0 and at most 1000 (tau_sem {sem}, tau_geo {geo}; tau_geo <= 0: no geographic "
            "head): beyond that the softmax is an argmax to float32 precision")


def make_engine(bank=None, sh_mode=_native.SH_ANALYTIC, keys_only=False):
    eng = _native.HipEngine(DEV)
    w = synth.make_encoder_weights(L, H, 256, 2, 5)
    eng.set_encoder(L, H, 2, 256, sh_mode, [w["layers.0.weight"], w["layers.1.weight"], w["last_layer.weight"]],
                    [w["layers.0.bias"], w["layers.1.bias"], w["last_layer.bias"]])
    if keys_only:
        eng.set_keys(bank.keys)
    elif bank is not None:
        eng.set_bank(bank.keys, bank.values, bank.xyz)
    return eng


@pytest.fixture(scope="module")
def bank():
    return O.prep_bank(*synth.make_bank(N, 5))


@pytest.fixture(scope="module")
def queries():
    return torch.from_numpy(synth.make_queries(B, seed=9, lat_max=90.0)).to(DEV)


def test_refusals_keep_code_and_text(bank, queries, monkeypatch):
    bare = _native.HipEngine(DEV)                                   # nothing set
    bankless = make_engine(sh_mode=_native.SH_CLOSED_FORM)          # an encoder ('closed form'), no bank
    keysonly = make_engine(bank, keys_only=True)
    plain = make_engine(bank)                                       # encoder and bank, nothing kept, no forward yet
    long_key, long_xyz = bank.keys.copy(), bank.xyz.copy()
    long_key[0], long_xyz[0] = 0.0, 0.0
    long_key[0, 0] = long_xyz[0, 0] = 2.0                           # one row of norm 2: exactly, in any arithmetic
    badkeys, badxyz = _native.HipEngine(DEV), _native.HipEngine(DEV)
    badkeys.set_bank(long_key, bank.values, bank.xyz)
    badxyz.set_bank(bank.keys, bank.values, long_xyz)
    monkeypatch.setenv("RANGE_KEEP_LOGITS", "0")
    nokeep = make_engine(bank)                                      # a context that never keeps pass 1's logits
    monkeypatch.delenv("RANGE_KEEP_LOGITS")
    # the 70 queries embedded by a forward call and scanned once with keep_logits; the same with the bf16 planes
    full, planes = make_engine(bank), make_engine(bank)
    planes.set_pv_mode("bf16x3")
    for eng in (full, planes):
        eng.forward(queries, PLUS, 0.5)
        e64, e32t, xqt = eng.encode(queries)
        stt = eng.scan_stats(e32t, xqt, 12.0, 40.0, keep_logits=True)
        assert eng.kept_queries() == B
    lib, h = full.lib, full._h
    alive = [e64, e32t, xqt, stt]

    def z(shape, dtype):
        alive.append(torch.zeros(shape, dtype=dtype, device=DEV))
        return alive[-1].data_ptr()

    def host(a):
        alive.append(a)
        return a.ctypes.data

    q, e64p, e32, xq, st = queries.data_ptr(), e64.data_ptr(), e32t.data_ptr(), xqt.data_ptr(), stt.data_ptr()
    out, part, raw = z((B, 1280), torch.float64), z((B, 1024), torch.float32), z((B, 256), torch.float64)
    tv, ti = z((B, 16), torch.float32), z((B, 16), torch.int64)
    coord = z((B, 4), torch.float64)
    diag, diag_cap = z((1 << 16,), torch.int64), 1 << 16
    out_host = host(np.zeros((B, 1280)))
    table = RefusalTable()
    rows = table.rows

    # ---- encoder_host.h
    desc = lambda *f: C.byref(alive.append(_native.EncoderDesc(*f)) or alive[-1])       # noqa: E731
    w = [np.zeros((H, L * L)), np.zeros((H, H)), np.zeros((256, H))]
    b = [np.zeros(H), np.zeros(H), np.zeros(256)]
    ptrs = lambda arrs: alive.append((C.c_void_p * 3)(*[host(a) if a is not None else None for a in arrs])) or alive[-1]  # noqa: E731
    rows("range_set_encoder", [bare._h, desc(L, H, 2, 256, 0), ptrs(w), ptrs(b)],
         ("ctx", {0: None}, NULL), ("desc", {1: None}, NULL), ("weights", {2: None}, NULL), ("biases", {3: None}, NULL),
         ("L 0", {1: desc(0, H, 2, 256, 0)}, "legendre_polys 0 unsupported (1..64)"),
         ("L 65", {1: desc(65, H, 2, 256, 0)}, "legendre_polys 65 unsupported (1..64)"),
         ("hidden 0", {1: desc(L, 0, 2, 256, 0)}, "hidden 0 unsupported (1..1024)"),
         ("hidden 1025", {1: desc(L, 1025, 2, 256, 0)}, "hidden 1025 unsupported (1..1024)"),
         ("layers 0", {1: desc(L, H, 0, 256, 0)}, "num_hidden_layers 0 unsupported"),
         ("layers 8", {1: desc(L, H, 8, 256, 0)}, "num_hidden_layers 8 unsupported"),
         ("embed 128", {1: desc(L, H, 2, 128, 0)}, "embed_dim 128 unsupported (must be 256)"),
         ("sh_mode 2", {1: desc(L, H, 2, 256, 2)}, "unknown sh_mode 2"),
         ("weights[1]", {2: ptrs([w[0], None, w[2]])}, "weights[1]/biases[1] null"),
         ("biases[2]", {3: ptrs([b[0], b[1], None])}, "weights[2]/biases[2] null"))
    f64s, i32s = (lambda: host(np.zeros(L * L))), (lambda v=0: host(np.full(L * L, v, dtype=np.int32)))
    sh_ok = [h, L, f64s(), f64s(), f64s(), i32s(), i32s(), i32s(), i32s(), 0, None, None]
    rows("range_set_sh_table", sh_ok,
         *[(f"argument {i}", {i: None}, NULL) for i in (0, 2, 3, 4, 5, 6, 7, 8)],
         ("terms without coef", {9: 1, 11: host(np.zeros(1, dtype=np.int32))}, NULL),
         ("terms without pow", {9: 1, 10: host(np.zeros(1))}, NULL),
         ("closed form", {0: bankless._h}, "the coefficient table belongs to the 'analytic' spherical harmonics"),
         ("L 9", {1: 9}, "table for L=9, encoder has L=10"),
         ("cnt -1", {8: i32s(-1)}, "bad table entry (l=0, m=0)"), ("off 1 of 0", {7: i32s(1)}, "bad table entry (l=0, m=0)"),
         ("p2 128", {5: i32s(128)}, "bad table entry (l=0, m=0)"), ("kx 10", {6: i32s(L)}, "bad table entry (l=0, m=0)"),
         ("power 10", {9: 1, 10: host(np.zeros(1)), 11: host(np.full(1, L, dtype=np.int32))}, "power 10 out of range at term 0"))
    rows("range_set_sh_table", sh_ok, ("no encoder", {0: bare._h}, NO_ENC), code=STATE)
    rows("range_encode", [h, q, B, e64p, e32, xq, None],
         *[(f"argument {i}", {i: None}, NULL) for i in (0, 1, 3, 4, 5)], ("B 0", {2: 0}, B_MSG))
    rows("range_encode", [h, q, B, e64p, e32, xq, None], ("no encoder", {0: bare._h}, NO_ENC), code=STATE)
    # (a refused range_encode_raw / range_forward* forgets the workspace's queries: not on `full`)
    rows("range_encode_raw", [plain._h, q, B, raw, None],
         ("ctx", {0: None}, NULL), ("lonlat", {1: None}, NULL), ("out", {3: None}, NULL), ("B 0", {2: 0}, B_MSG))
    rows("range_encode_raw", [plain._h, q, B, raw, None], ("no encoder", {0: bare._h}, NO_ENC), code=STATE)
    rows("range_coord_features", [h, 0, q, B, coord, None],
         ("ctx", {0: None}, NULL), ("lonlat", {2: None}, NULL), ("out", {4: None}, NULL),
         ("mode -1", {1: -1}, "coordinate encoder mode -1"), ("mode 3", {1: 3}, "coordinate encoder mode 3"), ("B 0", {3: 0}, B_MSG))

    # ---- bank_host.h
    keys, values, xyz = host(bank.keys), host(bank.values), host(bank.xyz)
    rows("range_set_bank", [bare._h, keys, values, xyz, N, 0],
         *[(f"argument {i}", {i: None}, NULL) for i in (0, 1, 2, 3)],
         ("n_rows 0", {4: 0}, ROWS_MSG), ("n_rows -1", {4: -1}, ROWS_MSG), ("n_rows 2^31", {4: 1 << 31}, "n_rows too large"))
    rows("range_set_keys", [bare._h, keys, N, 0],
         ("ctx", {0: None}, NULL), ("keys", {1: None}, NULL), ("n_rows 0", {2: 0}, ROWS_MSG), ("n_rows 2^31", {2: 1 << 31}, "n_rows too large"))
    rows("range_set_pv_mode", [bare._h, 0],
         ("ctx", {0: None}, NULL), ("mode 2", {1: 2}, "unknown pv mode 2"), ("mode -1", {1: -1}, "unknown pv mode -1"))
    rows("range_set_temperatures", [bare._h, 0.0, 0.0],
         ("ctx", {0: None}, NULL),
         ("tau_sem -1", {1: -1.0}, "temperatures must be finite, > 0 and at most 1000, or 0 for the model's default (tau_sem -1, tau_geo 0)"),
         ("tau_geo 1001", {2: 1001.0}, "temperatures must be finite, > 0 and at most 1000, or 0 for the model's default (tau_sem 0, tau_geo 1001)"))

    # ---- scan_host.h: what every kernel that forms softmax weights asks of the bank, B and the temperatures
    def softmax_rows(fn, ok, i_ctx, i_b, i_sem, i_geo):
        rows(fn, ok, ("no bank", {i_ctx: bankless._h}, NO_BANK), ("keys-only bank", {i_ctx: keysonly._h}, KEYS_ONLY), code=STATE)
        rows(fn, ok, ("B 0", {i_b: 0}, B_MSG), ("tau_sem 0", {i_sem: 0.0}, taus(0, 40)), ("tau_sem nan", {i_sem: float("nan")}, taus("nan", 40)),
             ("tau_sem 1001", {i_sem: 1001.0}, taus(1001, 40)), ("tau_geo 1001", {i_geo: 1001.0}, taus(12, 1001)),
             ("tau_geo inf", {i_geo: float("inf")}, taus(12, "inf")), ("tau_geo nan", {i_geo: float("nan")}, taus(12, "nan")),
             ("long key", {i_ctx: badkeys._h}, KEYS_NORM), ("long location", {i_ctx: badxyz._h}, XYZ_NORM))

    # (pass 1 forgets the kept logits in front of these checks: on `plain`)
    scan_ok = [plain._h, e32, xq, B, 12.0, 40.0, st, 0, None, None, 0, None]
    rows("range_scan_stats", scan_ok,
         *[(f"argument {i}", {i: None}, NULL) for i in (0, 1, 2, 6)],
         ("topk -1", {7: -1}, "topk must be in [0,16]"), ("topk 17", {7: 17, 8: tv, 9: ti}, "topk must be in [0,16]"),
         ("topk without values", {7: 5, 9: ti}, "topk outputs null"), ("topk without indices", {7: 5, 8: tv}, "topk outputs null"),
         ("sharp in-scan top-k", {0: nokeep._h, 4: 50.0, 7: 5, 8: tv, 9: ti},
          "range_scan_stats(topk > 0) at a temperature above 43 needs to keep its logits (this context cannot: "
          "RANGE_KEEP_LOGITS=0 or not enough free memory): take the top-k from range_topk_stream"))
    softmax_rows("range_scan_stats", scan_ok, 0, 3, 4, 5)
    at_ok = [plain._h, e32, xq, B, 12.0, 40.0, st, 0, B, 0, None]
    first_msg = "first_query must be a non-negative multiple of 64"
    rows("range_scan_stats_at", at_ok,
         *[(f"argument {i}", {i: None}, NULL) for i in (0, 1, 2, 6)],
         ("first 32", {7: 32, 8: 128}, first_msg), ("first -64", {7: -64}, first_msg),
         ("total 69", {8: 69}, "queries [0, 70) exceed the scan's 69"), ("past the total", {3: 6, 7: 64, 8: 69}, "queries [64, 70) exceed the scan's 69"),
         ("n_splits -1", {9: -1}, "n_splits must be >= 0"))
    softmax_rows("range_scan_stats_at", at_ok, 0, 3, 4, 5)
    ts, tg = host(np.array([12.0, 50.0], dtype=np.float32)), host(np.array([40.0, 0.0], dtype=np.float32))
    st2 = z((2, B, 4), torch.float32)
    kept_first = "first kept query must be a non-negative multiple of 64"
    kept_ok = [h, 0, xq, B, 2, ts, tg, 0, st2, None]
    rows("range_stats_kept", kept_ok,
         *[(f"argument {i}", {i: None}, NULL) for i in (0, 2, 5, 6, 8)],
         ("n_taus 0", {4: 0}, "n_taus must be >= 1"), ("n_splits -1", {7: -1}, "n_splits must be >= 0"),
         ("first 32", {1: 32, 3: 6}, kept_first), ("first -64", {1: -64}, kept_first), ("B 0", {3: 0}, B_MSG),
         ("B 71", {3: 71}, "queries [0, 71) exceed the 70 kept"), ("past the kept", {1: 64, 3: 7}, KEPT_70),
         ("second tau_sem 0", {5: host(np.array([12.0, 0.0], dtype=np.float32))}, taus(0, 0)),
         ("first tau_geo 1001", {6: host(np.array([1001.0, 0.0], dtype=np.float32))}, taus(12, 1001)))
    rows("range_stats_kept", kept_ok, ("nothing kept", {0: plain._h}, NO_KEPT), code=STATE)
    attend_ok = [plain._h, e32, xq, B, 12.0, 40.0, 0.5, st, part, None]
    rows("range_attend", attend_ok,
         *[(f"argument {i}", {i: None}, NULL) for i in (0, 1, 2, 7, 8)],
         ("beta 1.5", {6: 1.5}, BETA), ("beta -0.1", {6: -0.1}, BETA), ("beta nan", {6: float("nan")}, BETA))
    softmax_rows("range_attend", attend_ok, 0, 3, 4, 5)
    attend_kept_ok = [h, 0, xq, B, 12.0, 40.0, 0.5, st, part, None]
    rows("range_attend_kept", attend_kept_ok,
         *[(f"argument {i}", {i: None}, NULL) for i in (0, 2, 7, 8)],
         ("first -64", {1: -64}, "first_query must be >= 0"), ("first 32", {1: 32, 3: 6}, "first kept query must be a multiple of 64"),
         ("B 71", {3: 71}, "queries [0, 71) exceed the 70 kept"), ("past the kept", {1: 64, 3: 7}, KEPT_70),
         ("beta 1.5", {6: 1.5}, BETA), ("B 0", {3: 0}, B_MSG), ("tau_sem 0", {4: 0.0}, taus(0, 40)), ("tau_geo 1001", {5: 1001.0}, taus(12, 1001)),
         ("bf16x3 above 43", {0: planes._h, 4: 50.0}, "pv mode bf16x3 is not supported at temperatures above 43"))
    rows("range_attend_kept", attend_kept_ok, ("nothing kept", {0: plain._h}, NO_KEPT), code=STATE)
    diag_ok = [plain._h, e32, xq, B, 12.0, 40.0, 0.5, st, diag, diag_cap, None]
    rows("range_attend_diag", diag_ok,
         *[(f"argument {i}", {i: None}, NULL) for i in (0, 1, 2, 7, 8)],
         ("no geographic head", {5: 0.0}, "diagnostic build exists for the geo variant only"),
         ("capacity 0", {9: 0}, "diag buffer too small"), ("capacity 63", {9: 63}, "diag buffer too small"))
    softmax_rows("range_attend_diag", diag_ok, 0, 3, 4, 5)
    parts, vparts, iparts = z((2, B, 4), torch.float32), z((2, B, 16), torch.float32), z((2, B, 16), torch.int64)
    rows("range_merge_stats", [h, parts, 2, B, st2, None],
         ("ctx", {0: None}, NULL), ("parts", {1: None}, NULL), ("out", {4: None}, NULL), ("n_parts 0", {2: 0}, PARTS_B), ("B 0", {3: 0}, PARTS_B))
    rows("range_merge_topk", [h, vparts, iparts, 2, B, 16, tv, ti, None],
         *[(f"argument {i}", {i: None}, NULL) for i in (0, 1, 2, 6, 7)],
         ("n_parts 0", {3: 0}, "bad n_parts/B/k"), ("B 0", {4: 0}, "bad n_parts/B/k"), ("k 0", {5: 0}, "bad n_parts/B/k"),
         ("k 17", {5: 17}, "bad n_parts/B/k"))
    rows("range_finalize", [h, part, 1, e64p, B, out, None],
         *[(f"argument {i}", {i: None}, NULL) for i in (0, 1, 3, 5)], ("n_parts 0", {2: 0}, PARTS_B), ("B 0", {4: 0}, PARTS_B))
    rows("range_blend", [h, part, part, 0.5, B, z((B, 1024), torch.float32), None],
         *[(f"argument {i}", {i: None}, NULL) for i in (0, 1, 2, 5)], ("B 0", {4: 0}, B_MSG))

    # ---- topk_host.h
    avg, count = C.byref(alive.append(C.c_float()) or alive[-1]), C.byref(alive.append(C.c_int64()) or alive[-1])
    stream_ok = [h, e32, B, 16, tv, ti, None]
    rows("range_topk_stream", stream_ok,
         *[(f"argument {i}", {i: None}, NULL) for i in (0, 1, 4, 5)],
         ("B 0", {2: 0}, B_OR_K), ("k 0", {3: 0}, B_OR_K), ("k 17", {3: 17}, B_OR_K))
    rows("range_topk_stream", stream_ok, ("no bank", {0: bankless._h}, NO_BANK), code=STATE)
    last = ("range_topk_last(B=%d): the workspace holds the e-hat of %d queries (the last range_forward / range_forward_host "
            "call of this context)")
    last_ok = [h, B, 16, tv, ti, None]
    rows("range_topk_last", last_ok,
         ("ctx", {0: None}, NULL), ("values", {3: None}, NULL), ("indices", {4: None}, NULL), ("k 0", {2: 0}, B_OR_K), ("k 17", {2: 17}, B_OR_K))
    rows("range_topk_last", last_ok,
         ("B 69 of 70", {1: 69}, last % (69, B)), ("B 71 of 70", {1: 71}, last % (71, B)), ("B 0", {1: 0}, last % (0, B)),
         ("no forward yet", {0: plain._h}, last % (B, 0)), code=STATE)
    timed = "repeats must be >= 2 and avg_us non-null"
    rows("range_topk_stream_timed", [h, e32, B, 16, tv, ti, 2, avg, None],
         ("repeats 1", {6: 1}, timed), ("repeats 0", {6: 0}, timed), ("avg_us", {7: None}, timed),
         ("ctx", {0: None}, NULL), ("e-hat", {1: None}, NULL), ("k 0", {3: 0}, B_OR_K))
    read = "passes must be >= 1 and repeats >= 2"
    rows("range_stream_read_timed", [h, 0, 1, 2, avg, None],
         ("ctx", {0: None}, NULL), ("avg_us", {4: None}, NULL), ("passes 0", {2: 0}, read), ("repeats 1", {3: 1}, read))
    rows("range_stream_read_timed", [h, 0, 1, 2, avg, None], ("no bank", {0: bankless._h}, NO_BANK), code=STATE)
    rows("range_topk_stream_exact_count", [h, count], ("ctx", {0: None}, NULL), ("count", {1: None}, NULL))

    # ---- forward_host.h (what these refuse behind their encoder launch - no bank, a keys-only bank - is not here)
    for fn, o in (("range_forward", out), ("range_forward_host", out_host)):
        ok = [plain._h, q, B, PLUS, 0.5, o, None]
        rows(fn, ok, ("ctx", {0: None}, NULL), ("lonlat", {1: None}, NULL), ("out", {5: None}, NULL),
             ("model 2", {3: 2}, "unknown model 2"), ("model -1", {3: -1}, "unknown model -1"), ("B 0", {2: 0}, B_MSG), ("B -1", {2: -1}, B_MSG))
        rows(fn, ok, ("no encoder", {0: bare._h}, NO_ENC), code=STATE)
    rows("range_host_copy", [h, out_host, out_host, 8], ("ctx", {0: None}, NULL), ("dst", {1: None}, NULL), ("src", {2: None}, NULL))

    assert len(table) == 248
    table.check(lib)
    torch.cuda.synchronize()
    assert full.kept_queries() == B and planes.kept_queries() == B and plain.kept_queries() == 0
    for eng in (full, plain, bankless, keysonly, badkeys, badxyz, nokeep, planes):
        eng.check_async_error()


def test_a_refused_forward_and_the_workspace_claim(bank, queries):
    """Against a keys-only bank both forward calls run their encoder and are refused by pass 1.  range_forward claims
    the workspace's e-hat for range_topk_last only when it succeeds; range_forward_host claims it as soon as the
    encoder is enqueued - its top-k then runs, and gives what range_topk_stream gives on that e-hat."""
    eng = make_engine(bank, keys_only=True)
    lib, h = eng.lib, eng._h
    out = torch.zeros((B, 1280), dtype=torch.float64, device=DEV)
    out_host = np.zeros((B, 1280))
    tv, ti = torch.zeros((B, 4), dtype=torch.float32, device=DEV), torch.zeros((B, 4), dtype=torch.int64, device=DEV)
    refused = lambda rc: (rc, lib.range_last_error().decode())                               # noqa: E731
    assert refused(lib.range_forward(h, queries.data_ptr(), B, PLUS, 0.5, out.data_ptr(), None)) == (STATE, KEYS_ONLY)
    assert refused(lib.range_topk_last(h, B, 4, tv.data_ptr(), ti.data_ptr(), None)) == (
        STATE, "range_topk_last(B=70): the workspace holds the e-hat of 0 queries (the last range_forward / range_forward_host "
               "call of this context)")
    assert refused(lib.range_forward_host(h, queries.data_ptr(), B, PLUS, 0.5, out_host.ctypes.data, None)) == (STATE, KEYS_ONLY)
    assert lib.range_topk_last(h, B, 4, tv.data_ptr(), ti.data_ptr(), None) == 0
    _, e32, _ = eng.encode(queries)
    val, idx = eng.topk_stream(e32, 4)
    assert torch.equal(val, tv) and torch.equal(idx, ti)
    # ... and a refused range_forward takes the claim back
    assert refused(lib.range_forward(h, queries.data_ptr(), B, PLUS, 0.5, out.data_ptr(), None)) == (STATE, KEYS_ONLY)
    assert lib.range_topk_last(h, B, 4, tv.data_ptr(), ti.data_ptr(), None) == STATE
