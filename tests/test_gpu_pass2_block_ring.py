"""Pass 2 on kept logits with the block-granular V ring (`-m gpu`): ``attend_kept`` (attend_stored_kernel:
two ring slots of a whole 16-row block, one barrier per block, the block loop unrolled by two with an
odd tail) bit for bit against ``attend`` (attend_kernel: the recompute kernel), and against the float64
oracle.  The two kernels share the PV step, the block weights and the write-out (pass2.h: pv_step,
block_weights, store_acc_tile), so the bitwise comparison does not separate those; it separates what each
kernel has of its own: a ring of three half blocks against one of two whole blocks, two barriers and
hand-overs per block against one, pad rows masked in every block against zeroed once in front of the
last, recomputed against kept logits.  What anchors both, shared code included, is the float64 oracle at
2e-5.

Bank sizes are the smallest at which the ring, the tail and the segments can go wrong: 16 / 32 / 48 rows
= 1 / 2 / 3 blocks (the odd tail alone; one unrolled body; body + tail), 53 rows (a last block with 5
valid rows), 1 000 rows (63 blocks, 8 valid rows in the last), 20 011 rows; 17 / 33 / 65 / 200 queries =
a partial wave, a partial tile, two tiles, four tiles.  Each shape runs under the default plan (at these
sizes the stream-K walk: several segments per workgroup, segments of one block, ring re-use across the
segments' barrier) and in a context created with RANGE_P2_STREAMK=0 (the split scheme: small batches
get splits of very few blocks)."""
import os

import numpy as np
import pytest
import torch

from oracle import range_oracle as O
from range_amd import _native
from range_amd.bank import prepare_bank
from range_amd.ckpt import EncoderParams
from tools import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L, H = 10, 64
BATCHES = (17, 33, 65, 200)
# (model name for the oracle, tau_sem, tau_geo, betas): range/range.py's temperatures
MODELS = (("RANGE+", 12.0, 40.0, (0.0, 0.5, 1.0)), ("RANGE", 15.0, 0.0, (1.0,)))


def _encoder():
    w = synth.make_encoder_weights(L, H, 256, 2, 5)
    ws = [w[f"layers.{i}.weight"] for i in range(2)] + [w["last_layer.weight"]]
    bs = [w[f"layers.{i}.bias"] for i in range(2)] + [w["last_layer.bias"]]
    return EncoderParams(L, H, 2, 256, "analytic", ws, bs)


def _engine(enc, bank, env=None):
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        eng = _native.HipEngine(DEV)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    eng.set_encoder(enc.legendre_polys, enc.hidden, enc.num_hidden_layers, 256, _native.SH_ANALYTIC,
                    enc.weights, enc.biases)
    eng.set_bank(bank.keys, bank.values, bank.xyz, 0)
    return eng


@pytest.mark.parametrize("N", [16, 32, 48, 53, 1000, 20_011])
def test_attend_kept_equals_the_recompute_kernel_bitwise_and_the_oracle(N):
    enc = _encoder()
    locs, vals, keys = synth.make_bank(N, 31)
    bank, obank = prepare_bank(locs, vals, keys), O.prep_bank(locs, vals, keys)
    engines = (("stream-K", _engine(enc, bank)), ("splits", _engine(enc, bank, env={"RANGE_P2_STREAMK": "0"})))
    for B in BATCHES:
        qn = synth.make_queries(B, seed=N + B, lat_max=90.0)
        x = torch.from_numpy(qn).to(DEV)
        ref = {}                                                   # the oracle once per (model, beta)
        for plan, eng in engines:
            e64, e32, xq = eng.encode(x)
            for name, tau_sem, tau_geo, betas in MODELS:
                st = eng.scan_stats(e32, xq, tau_sem, tau_geo, keep_logits=True)
                assert eng.kept_queries() == B
                for beta in betas:
                    what = f"{name} beta={beta} N={N} B={B} {plan}"
                    kept = eng.attend_kept(0, xq, tau_sem, tau_geo, beta, st)
                    again = eng.attend_kept(0, xq, tau_sem, tau_geo, beta, st)
                    rec = eng.attend(e32, xq, tau_sem, tau_geo, beta, st)
                    assert torch.equal(kept, again), what + ": two launches differ"
                    assert torch.equal(kept, rec), what + ": max |kept - recompute| = %g" % float((kept - rec).abs().max())
                    if (name, beta) not in ref:
                        ref[name, beta] = O.retrieve64(e64.cpu().numpy(), qn, obank, name, beta)
                    np.testing.assert_allclose(kept.cpu().numpy(), ref[name, beta], rtol=0, atol=2e-5, err_msg=what)
            eng.check_async_error()
