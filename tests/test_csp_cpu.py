"""The CSP location encoders ('CSP', 'CSP_INat'), CPU side (no GPU): the checkpoint reader
(range_amd/csp.py), its frequency tables against the reference's, the launch plan and the weight packing
under the host sanitizers, and the numpy float64 restatement the GPU tests compare the kernel with
(tests/csp_refs.py) against the reference's recorded float32 outputs (tests/golden/csp_encoders.npz,
written by make_golden_csp.py).

The bound of the GPU tests is 4 * max(E_ref, 2^-23 max|out|) per case, E_ref = max |reference float32 -
restatement float64| measured HERE from the fixture (csp_refs.gpu_bound); every planted defect must exceed
it on at least one case."""
import os
import subprocess

import numpy as np
import pytest
import torch

import csp_refs as R
from range_amd import csp, posenc
from tools import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "csp_encoders.npz"))


@pytest.fixture(scope="module")
def nets(golden):
    return {c: R.case_network(golden, c) for c in R.CASES}


def test_fixture_rows(golden):
    q = golden["lonlat"]
    assert q.shape == (24, 2) and np.isfinite(q[:21]).all() and not np.isfinite(q[21:]).all(axis=1).any()
    assert [tuple(r) for r in q[16:21]] == [(0, 0), (-180, -90), (180, 90), (-180, 90), (180, -90)]
    assert set(R.CASES) == {k[:-len("_out")] for k in golden.files if k.endswith("_out")}
    assert sorted(str(golden[c + "_name"]) for c in R.CASES).count("CSP_INat") == 1
    for c in R.CASES:
        out = golden[c + "_out"]
        assert str(golden[c + "_type"]) == "Tensor" and str(golden[c + "_dtype"]) == "torch.float32" and out.dtype == np.float32
        assert np.isfinite(out[:21]).all() and np.isnan(out[21:]).all()
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "csp_encoders.npz")) < 1 << 20


@pytest.mark.parametrize("case", R.CASES)
def test_reader_and_frequency_table(golden, nets, case, tmp_path):
    """A checkpoint written with the reference's key names reads back as the fixture's network; the frequency
    table is the reference's bit for bit; params['device'], the heads and the spa_enc.* aliases are ignored."""
    net = nets[case]
    s = net["settings"]
    path = synth.write_csp_checkpoint(str(tmp_path / "m.pth.tar"), **s)
    sd = torch.load(path, weights_only=False)["state_dict"]
    assert {"class_emb.weight", "loc_enc.user_emb.weight", "img_dec.bias", "spa_enc.ffn.layers.0.linear.weight"} <= set(sd)
    p = csp.read_csp_checkpoint(path)
    assert (p.spa_enc_type, p.frequency_num, p.activation, p.use_layn, p.skip_connection, p.num_filts) == \
        (s["spa_enc_type"], s["F"], s["act"], s["use_layn"], s["skip"], s["num_filts"])
    assert p.kind == {"gridcell": posenc.KIND_GRID, "theory": posenc.KIND_THEORY}[s["spa_enc_type"]]
    assert p.widths == [s["hidden"]] * s["layers"] + [s["num_filts"]] and p.input_dim == p.weights[0].shape[1]
    assert np.array_equal(p.freq_list, golden[case + "_freq_list"]) and p.freq_list.dtype == np.float64
    for i in range(len(p.widths)):
        assert np.array_equal(p.weights[i], net["weights"][i]) and np.array_equal(p.biases[i], net["biases"][i])
        if net["ln_gamma"][i] is None:
            assert p.ln_gamma[i] is None and p.ln_beta[i] is None
        else:
            assert np.array_equal(p.ln_gamma[i], net["ln_gamma"][i]) and np.array_equal(p.ln_beta[i], net["ln_beta"][i])


def _rewrite(path, edit):
    ck = torch.load(path, weights_only=False)
    edit(ck)
    torch.save(ck, path)
    return path


def test_reader_refusals(tmp_path):
    base = dict(spa_enc_type="gridcell", F=4, hidden=16, layers=1, act="relu", use_layn=True, skip=True, num_filts=8)
    path = str(tmp_path / "m.pth.tar")
    for spa in csp.UNSUPPORTED_SPA_ENC:
        synth.write_csp_checkpoint(path, **dict(base, spa_enc_type=spa))
        with pytest.raises(NotImplementedError, match=repr(spa)):
            csp.read_csp_checkpoint(path)
    assert set(csp.UNSUPPORTED_SPA_ENC) == {"gridcellnorm", "theorynorm", "theorydiag", "hexagridcell", "naive", "rbf",
                                            "rff", "geo_net", "geo_net_fft"}
    synth.write_csp_checkpoint(path, **dict(base, freq_init="random"))
    with pytest.raises(NotImplementedError, match="'random'"):
        csp.read_csp_checkpoint(path)
    synth.write_csp_checkpoint(path, **dict(base, act="swish"))
    with pytest.raises(NotImplementedError, match="swish"):
        csp.read_csp_checkpoint(path)
    # shapes that are not what params say
    synth.write_csp_checkpoint(path, **base)
    _rewrite(path, lambda ck: ck["params"].update(hidden_dim=17))
    with pytest.raises(ValueError, match="linear.weight"):
        csp.read_csp_checkpoint(path)
    synth.write_csp_checkpoint(path, **base)
    _rewrite(path, lambda ck: ck["params"].update(num_hidden_layer=0))
    with pytest.raises(ValueError):
        csp.read_csp_checkpoint(path)
    synth.write_csp_checkpoint(path, **base)
    _rewrite(path, lambda ck: ck["params"].update(use_layn=False))
    with pytest.raises(ValueError, match="layernorm"):
        csp.read_csp_checkpoint(path)
    synth.write_csp_checkpoint(path, **base)
    _rewrite(path, lambda ck: ck["state_dict"].update(
        {"loc_enc.spa_enc.ffn.layers.0.linear.bias": ck["state_dict"]["loc_enc.spa_enc.ffn.layers.0.linear.bias"].double()}))
    with pytest.raises(ValueError, match="float32"):
        csp.read_csp_checkpoint(path)
    # the envelope
    for bad in (dict(F=65), dict(hidden=1025), dict(num_filts=1025), dict(layers=9)):
        synth.write_csp_checkpoint(path, **dict(base, **bad))
        with pytest.raises(ValueError, match="supported"):
            csp.read_csp_checkpoint(path)
    synth.write_csp_checkpoint(path, **dict(base, layers=8))
    assert len(csp.read_csp_checkpoint(path).widths) == 9


def test_csp_plan_under_sanitizers(tmp_path):
    """host_plan.h: csp_plan / csp_pack_layer (tests/native/csp_plan.cpp) compiled with g++ under
    AddressSanitizer and UndefinedBehaviorSanitizer and run on the CPU."""
    exe = str(tmp_path / "csp_plan")
    src = os.path.join(REPO, "tests", "native", "csp_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    src, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "csp_plan ok" in p.stdout, p.stdout + p.stderr


@pytest.mark.parametrize("case", R.CASES)
def test_restatement_against_the_reference(golden, nets, case):
    """E_ref per case, from the fixture: the reference's float32 result lies within a few float32 roundings of
    the float64 restatement (DESIGN.md 4 records the values), and NaN rows agree."""
    ref, net = golden[case + "_out"], nets[case]
    got = R.encode(net, golden["lonlat"])
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref))
    e, scale = R.e_ref(golden, case, net), float(np.nanmax(np.abs(ref)))
    print(f"{case}: E_ref = {e:.3e}, max|out| = {scale:.4f}, E_ref / max|out| = {e / scale:.2e}, GPU bound {R.gpu_bound(golden, case, net):.3e}")
    # float32 arithmetic: a chain of up to 512 products, LayerNorm, the activation - far below 1e-5 relative
    assert e <= 1e-5 * scale


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_a_planted_defect_exceeds_the_gpu_bound(golden, nets, defect):
    """The bound the GPU tests use discriminates: each defect moves some case further from the restatement
    than a kernel may be."""
    over = {}
    for case in R.CASES:
        net, q = nets[case], golden["lonlat"][:21]
        err = float(np.abs(R.encode(net, q, defect=defect) - R.encode(net, q)).max())
        over[case] = err / R.gpu_bound(golden, case, net)
    print(defect, {c: f"{v:.3g}" for c, v in over.items()})
    assert max(over.values()) > 1.0, over


def test_loader_errors(tmp_path):
    from range_amd.load_model import load_model
    path = synth.write_csp_checkpoint(str(tmp_path / "m.pth.tar"), F=4, hidden=16, num_filts=8)
    for name in ("CSP", "CSP_INat"):
        with pytest.raises(ValueError, match="pretrained"):
            load_model(name)
        with pytest.raises(ValueError, match="RANGE / RANGE\\+"):
            load_model(name, pretrained_path=path, temp=20.0)
        with pytest.raises(ValueError, match="shards"):
            load_model(name, pretrained_path=path, shards=2)
        with pytest.raises(RuntimeError, match="no CPU path"):
            load_model(name, pretrained_path=path, device="cpu")
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError):
                load_model(name, pretrained_path=path, device="cuda")
    for name in ("GeoCLIP", "TaxaBind", "SINR"):
        with pytest.raises(NotImplementedError, match=name):
            load_model(name, pretrained_path=path, device="cuda")
