"""The lifecycle of a context that holds a CSP encoder fit (`-m gpu`): a second ``begin`` with a smaller network and
fewer classes behind a larger one whose workspaces were filled, and a fit interleaved with ``range_set_csp`` /
``range_csp_encode`` / a class-head fit on the same context, each give a fresh context's bits; the installed inference
network is unchanged by a fit."""
import os

import numpy as np
import pytest
import torch

import cspfit_cases as K
from range_amd import _cspfit_native as cn
from range_amd import _headfit_native as hn
from range_amd import csp
from tools import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(DEV)


def net(tmp, hidden, layers, nf, C, seed, F=8):
    path = synth.write_csp_checkpoint(os.path.join(str(tmp), f"n{seed}.pth.tar"), device="cpu", spa_enc_type="gridcell", F=F, hidden=hidden,
                                      layers=layers, num_filts=nf, num_classes=C, class_scale=0.3, seed=seed, min_radius=1.0,
                                      max_radius=360.0, dropout=0.0)
    return csp.read_csp_checkpoint(path, class_head=True)


def inputs(B, Bg, C, seed):
    rng = np.random.default_rng(seed)
    ll = lambda n: np.stack([rng.uniform(-180, 180, n), rng.uniform(-90, 90, n)], axis=1)      # noqa: E731
    return dev(ll(B + 4), np.float64), dev(rng.integers(0, B + 4, B), np.int32), dev(rng.integers(0, C, B), np.int32), dev(ll(Bg), np.float64)


def run(fit, p, C, d):
    fit.begin(p, C, p.class_emb)
    out = [*fit.grad(*d, 0.5)]
    out += [fit.step(*d, lr=1e-2, weight=0.5, weight_decay=0.01, dropout=0.25, seed=5) for _ in range(2)]
    return out + [fit.flat_params(), fit.loss(*d, 0.5, want_emb=True)[1]]


def set_csp(eng, p):
    eng.set_csp(p.kind, p.freq_list, p.widths, p.weights, p.biases, p.ln_gamma, p.ln_beta, csp.ACTIVATIONS[p.activation],
                p.skip_connection, p.use_layn)


def test_smaller_fit_behind_a_larger_one_and_interleaved_calls(tmp_path):
    big, small, other = net(tmp_path, 96, 3, 64, 300, 1, F=24), net(tmp_path, 32, 1, 12, 33, 2), net(tmp_path, 48, 1, 20, 7, 3)
    d_big, d_small = inputs(200, 190, 300, 4), inputs(33, 31, 33, 5)
    q = dev(np.random.default_rng(6).uniform(-80, 80, (70, 2)), np.float64)
    fresh = cn.CspFit(DEV)
    want = run(fresh, small, 33, d_small)
    set_csp(fresh.engine, other)
    want_enc = fresh.engine.csp_encode(q)
    fresh.engine.close()

    a = cn.CspFit(DEV)
    run(a, big, 300, d_big)                                  # the workspaces and stores filled by a larger fit
    for x, y in zip(want, run(a, small, 33, d_small)):
        assert torch.equal(x, y)
    # interleaved with the inference network and a class-head fit on the same context
    set_csp(a.engine, other)
    a.engine.set_csp_head(other.class_emb)
    hf = hn.HeadFit(a.engine)
    feats = a.engine.csp_encode(q)
    assert torch.equal(feats, want_enc)
    hf.begin(7, 20, other.class_emb)
    lab = dev(np.arange(70) % 7, np.int32)
    a.begin(small, 33, small.class_emb)
    out = [*a.grad(*d_small, 0.5)]
    h1 = hf.step(feats, None, lab, None, 1e-2)
    out.append(a.step(*d_small, lr=1e-2, weight=0.5, weight_decay=0.01, dropout=0.25, seed=5))
    assert torch.equal(a.engine.csp_encode(q), want_enc)    # the installed network is unchanged by the fit
    set_csp(a.engine, other)
    out.append(a.step(*d_small, lr=1e-2, weight=0.5, weight_decay=0.01, dropout=0.25, seed=5))
    h2 = hf.step(feats, None, lab, None, 1e-2)
    out += [a.flat_params(), a.loss(*d_small, 0.5, want_emb=True)[1]]
    for x, y in zip(want, out):
        assert torch.equal(x, y)
    assert (a.num_classes, a.steps, hf.num_classes, hf.steps) == (33, 2, 7, 2) and not torch.equal(h1, h2)
    assert torch.equal(a.engine.csp_encode(q), want_enc) and a.engine.csp_classes == 0      # (set_csp dropped the head)
    # the head fit alone on a fresh context: the same two losses
    b = hn.HeadFit(DEV)
    set_csp(b.engine, other)
    fb = b.engine.csp_encode(q)
    b.begin(7, 20, other.class_emb)
    assert torch.equal(h1, b.step(fb, None, lab, None, 1e-2)) and torch.equal(h2, b.step(fb, None, lab, None, 1e-2))
    a.engine.close()
    b.engine.close()
