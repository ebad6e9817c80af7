"""range_forward in chunks of query tiles, pass 1 of the next chunk on the CUs pass 2 occupies (`-m gpu`;
forward_host.h: forward_chunked, pass1_beside.h: scan_stats_beside_kernel).  The yardstick is always a second
engine created with RANGE_FWD_OVERLAP=0 on the same bank - the forward of one launch per pass - and the check
is ``torch.equal`` on the whole (B, 1280) result: every chunk takes the whole batch's split counts, the new
kernel keeps scan_stats_kernel's MFMA chain and statistics, so nothing may move by a bit.

Shapes (all engines with RANGE_P2_STREAMK=0, so that a small bank takes the split scheme): a bank of 4 100
rows = 257 blocks, 4 valid rows in the last one, with 130 queries in forced chunks of 1 tile (three chunks,
the last with 2 queries), 337 queries in chunks of 2 tiles (the last tile partial) and 64 queries (one tile:
no chunking, the path of the switch off); a bank of 50 016 rows (beyond the stream-K walk with nothing set)
with 1 024 queries in chunks of 8 tiles.  The routes that must not chunk - sharp temperatures, pv_mode
'bf16x3', RANGE_KEEP_LOGITS=0, a 20 000-row bank with the stream-K walk left on - give the same result and
report the same geometry with the switch forced and off."""
import functools
import os

import pytest
import torch

from range_amd import _native
from range_amd.bank import prepare_bank
from range_amd.ckpt import EncoderParams
from tools import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L, H = 10, 64
# (model, beta): RANGE and RANGE+
MODELS = ((_native.MODEL_RANGE, 1.0), (_native.MODEL_RANGE_PLUS, 0.5))
TAUS = {_native.MODEL_RANGE: (15.0, 0.0), _native.MODEL_RANGE_PLUS: (12.0, 40.0)}


@functools.lru_cache(maxsize=None)
def _encoder():
    w = synth.make_encoder_weights(L, H, 256, 2, 5)
    ws = [w[f"layers.{i}.weight"] for i in range(2)] + [w["last_layer.weight"]]
    bs = [w[f"layers.{i}.bias"] for i in range(2)] + [w["last_layer.bias"]]
    return EncoderParams(L, H, 2, 256, "analytic", ws, bs)


@functools.lru_cache(maxsize=2)
def _bank(N):
    return prepare_bank(*synth.make_bank(N, 31))


def _engine(N, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = _native.HipEngine(DEV)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    enc, bank = _encoder(), _bank(N)
    eng.set_encoder(enc.legendre_polys, enc.hidden, enc.num_hidden_layers, 256, _native.SH_ANALYTIC,
                    enc.weights, enc.biases)
    eng.set_bank(bank.keys, bank.values, bank.xyz, 0)
    return eng


def _queries(B, seed):
    return torch.from_numpy(synth.make_queries(B, seed=seed, lat_max=90.0)).to(DEV)


@pytest.mark.parametrize("N,B,tiles", [(4100, 130, 1), (4100, 337, 2), (4100, 64, 1), (50016, 1024, 8)])
def test_chunked_forward_equals_the_forward_of_one_launch_per_pass_bitwise(N, B, tiles):
    split = {"RANGE_P2_STREAMK": "0"}
    yard = _engine(N, dict(split, RANGE_FWD_OVERLAP="0"))
    eng = _engine(N, dict(split, RANGE_FWD_OVERLAP=str(tiles)))
    x, x2 = _queries(B, N + B), _queries(B, N + B + 1)
    for model, beta in MODELS:
        what = f"model {model} N={N} B={B} chunks of {tiles}"
        ref, ref2 = yard.forward(x, model, beta), yard.forward(x2, model, beta)
        geometry = yard.last_geometry()
        # the same call three times
        outs = [eng.forward(x, model, beta) for _ in range(3)]
        for o in outs:
            assert torch.equal(o, ref), what + ": max |chunked - one launch| = %g" % float((o - ref).abs().max())
        # two different batches back to back, nothing between them
        a = eng.forward(x, model, beta)
        b = eng.forward(x2, model, beta)
        assert torch.equal(a, ref) and torch.equal(b, ref2), what + ": back-to-back calls"
        assert eng.last_geometry() == geometry, what
        # the kept logits are complete and in pass 1's layout: pass 2 of all B queries from them, with the
        # statistics of the yardstick's scan, gives the yardstick's bits
        assert eng.kept_queries() == B, what
        tau_sem, tau_geo = TAUS[model]
        _, e32, xq = yard.encode(x2)
        st = yard.scan_stats(e32, xq, tau_sem, tau_geo, keep_logits=True)
        want = yard.attend_kept(0, xq, tau_sem, tau_geo, beta, st)
        got = eng.attend_kept(0, xq, tau_sem, tau_geo, beta, st)
        assert torch.equal(got, want), what + ": attend_kept from the chunked forward's logits"
        eng.check_async_error()


@pytest.mark.parametrize("route", ["sharp", "bf16x3", "no_keep", "streamk"])
def test_routes_that_do_not_chunk_are_the_same_with_the_switch_forced_and_off(route):
    N, B = (20000, 337) if route == "streamk" else (4100, 337)
    env = {} if route == "streamk" else {"RANGE_P2_STREAMK": "0"}
    if route == "no_keep":
        env["RANGE_KEEP_LOGITS"] = "0"
    engines = [_engine(N, dict(env, RANGE_FWD_OVERLAP=v)) for v in ("0", "2")]
    for eng in engines:
        if route == "sharp":
            eng.set_temperatures(100.0, 40.0)
        if route == "bf16x3":
            eng.set_pv_mode("bf16x3")
    x = _queries(B, 77)
    for model, beta in MODELS:
        ref, out = (eng.forward(x, model, beta) for eng in engines)
        assert torch.equal(out, ref), f"{route} model {model}: max |forced - off| = %g" % float((out - ref).abs().max())
        assert engines[1].last_geometry() == engines[0].last_geometry(), route
