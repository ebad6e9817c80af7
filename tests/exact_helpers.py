"""What the bit-exact GPU tests share (tests/test_gpu_exact.py, tests/test_gpu_exact_dense.py): an
environment override for engines created under a switch, host -> device, and the equality check
that says which rows differ; the constant-e-hat model of the forward-level tests."""
import contextlib
import os

import numpy as np
import torch

from range_amd import load_model
from range_amd.bank import PreparedBank
from range_amd.bankfile import write_bankfile
from tools import exact_bank as X
from tools import synth

DEV = "cuda:0"


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _assert_equal(got, want, what):
    if torch.equal(got, want):
        return
    bad = (got != want).any(dim=1) if got.dim() == 2 else (got != want)
    rows = torch.nonzero(bad).flatten().tolist()
    d = float((got.double() - want.double()).abs().max())
    raise AssertionError(f"{what}: {len(rows)} of {got.shape[0]} rows differ (first {rows[:8]}), max |diff| {d:.3e}")


# -- forward level: a checkpoint whose encoder returns one class direction ------------------------
L_ENC, H_ENC = 10, 64


def _model(tmp_path, bank, c, model, beta, prepared=False, **kw):
    """load_model from a checkpoint whose last layer is weight 0, bias e-hat of class c, and an
    .npz bank at axis locations - or, ``prepared``, the bank's own arrays as a prepared bank file, which
    the engine uploads as they are (no float32 normalisation of the keys, no trigonometry: keys with
    mantissa perturbations and graded locations arrive bit for bit).  ``kw``: further load_model
    arguments (temp=, geo_temp=, pv_mode=)."""
    w = synth.make_encoder_weights(L_ENC, H_ENC, 256, 2, 5)
    w["last_layer.weight"][:] = 0.0
    w["last_layer.bias"][:] = bank.class_vectors([c])[0]
    sd = {}
    for key, v in w.items():
        t = torch.from_numpy(np.ascontiguousarray(v))
        sd[f"model.location.nnet.{key}"] = t
        sd[f"model.nnet.{key}"] = t
    ck = str(tmp_path / "const.ckpt")
    torch.save({"hyper_parameters": synth.default_hparams(L_ENC, H_ENC, 256, 2), "state_dict": sd}, ck)
    if prepared:
        db = write_bankfile(str(tmp_path / "db.rbank"), PreparedBank(bank.keys, bank.values, bank.xyz))
    else:
        db = str(tmp_path / "db.npz")
        np.savez(db, locs=X.lonlat_of(bank.geo), image_embeddings=bank.values, satclip_embeddings=bank.keys)
    return load_model(model, pretrained_path=ck, device=DEV, db_path=db, beta=beta, **kw)


def _fwd_queries(bank, c, B, seed):
    q = X.forward_queries(bank, c, B, seed)
    return q, X.lonlat_of(q.geo)


def _fwd_want(bank, q, beta, geo):
    e = q.e32[:1].astype(np.float64).repeat(len(q.sem), 0)
    return np.concatenate([X.expect(bank, q, beta, geo).astype(np.float64), e], axis=1)


def _assert_rows(got, want, what):
    got = torch.as_tensor(got).cpu()
    _assert_equal(got, torch.from_numpy(want), what)
