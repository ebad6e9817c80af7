"""The training-free positional encoders 'Theory' / 's2vec_*', CPU side (no GPU): the numpy restatement
the GPU tests compare the kernel with (tests/posenc_refs.py) against the reference's recorded outputs
(tests/golden/posenc_encoders.npz, written by make_golden_posenc.py), the settings and frequency tables of
range_amd/posenc.py, the launch plan under the host sanitizers, and the loader's errors.

Bounds (derived, not tuned): a single sine / cosine 4e-16 (what the Wrap test grants a libm); a product of
two 2 * 4e-16 + 1.2e-16 -> 1e-15; float32-in results after rounding 6e-8 (one float32 ulp at 1); NaN
positions equal."""
import os
import subprocess

import numpy as np
import pytest

import posenc_refs as R
from range_amd import posenc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = tuple(R.KIND_OF_MODEL)
assert_close = R.assert_close


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "posenc_encoders.npz"))


def test_fixture_rows(golden):
    q = golden["lonlat"]
    assert q.shape == (16, 2) and np.isnan(q[13, 0]) and np.isinf(q[14, 1]) and np.isinf(q[15, 0]) and np.isnan(q[15, 1])
    assert np.isfinite(q[:13]).all()
    for name in NAMES:
        assert str(golden[name + "_type"]) == "Tensor"
        assert golden[name + "_f64"].dtype == np.float64 and golden[name + "_f32"].dtype == np.float32
        # the finite rows are finite, the three bad rows hold NaN
        assert np.isfinite(golden[name + "_f64"][:13]).all()
        assert np.isnan(golden[name + "_f64"][13:]).any(axis=1).all()


@pytest.mark.parametrize("name", NAMES)
def test_restatement_against_the_reference(golden, name):
    kind, q, f = R.KIND_OF_MODEL[name], golden["lonlat"], golden[name + "_freq_list"]
    out = R.encode(kind, q, f)
    assert_close(kind, out, golden[name + "_f64"])
    out32 = R.encode(kind, q.astype(np.float32), f).astype(np.float32)
    assert_close(kind, out32, golden[name + "_f32"])
    # same libm, same expression order: equal bit for bit where this fixture was written
    print(name, "bitwise float64:", np.array_equal(out, golden[name + "_f64"], equal_nan=True))


@pytest.mark.parametrize("name", NAMES)
def test_settings_and_frequency_tables(golden, name):
    s = posenc.spec(name)
    assert s.frequency_num == int(golden[name + "_frequency_num"])
    assert float(s.min_radius) == float(golden[name + "_min_radius"])
    assert float(s.max_radius) == float(golden[name + "_max_radius"])
    assert s.width == int(golden[name + "_embedding_dim"]) == golden[name + "_f64"].shape[1]
    assert s.width == R.width(R.KIND_OF_MODEL[name], s.frequency_num) == posenc.PER_FREQ[s.kind] * s.frequency_num
    assert R.KINDS[s.kind] == R.KIND_OF_MODEL[name]
    f, ref = posenc.freq_list(name), golden[name + "_freq_list"]
    assert f.dtype == np.float64 and f.shape == ref.shape == (s.frequency_num,)
    assert (np.abs(f - ref) <= np.spacing(np.abs(ref))).all()          # within one ulp (bitwise where the fixture was written)
    assert s.frequency_num <= posenc.MAX_FREQ


def test_names():
    assert set(posenc.MODELS) == set(NAMES)
    assert posenc.is_posenc_name("Theory") and posenc.is_posenc_name("s2vec_spherem") and posenc.is_posenc_name("s2vec_nosuch")
    assert not posenc.is_posenc_name("Wrap") and not posenc.is_posenc_name("RANGE+")
    with pytest.raises(NotImplementedError):
        posenc.spec("s2vec_nosuch")


@pytest.mark.parametrize("name,defect", [("s2vec_spherec", "swap"), ("s2vec_spheremplus", "swap"), ("Theory", "swap"),
                                         ("s2vec_grid", "swap"), ("s2vec_spherem", "nodup"), ("s2vec_spherecplus", "nodup"),
                                         ("Theory", "fma")])
def test_a_planted_defect_fails(golden, name, defect):
    """The fixture and the bounds catch a swapped pair of terms, a dropped duplication and Theory's angles
    contracted into an FMA (emulated in long double: 3e-14 in the output)."""
    kind, q, f = R.KIND_OF_MODEL[name], golden["lonlat"], golden[name + "_freq_list"]
    bad = R.encode(kind, q, f, defect=defect)
    with pytest.raises(AssertionError):
        assert_close(kind, bad, golden[name + "_f64"])
    assert_close(kind, R.encode(kind, q, f), golden[name + "_f64"])


def test_posenc_plan_under_sanitizers(tmp_path):
    """host_plan.h: posenc_plan - widths for every kind and F in {1, 16, 33, 64}; for B in {1, 255, 256,
    257, 2^31 + 5} every (location, frequency) covered exactly once and no grid dimension overflows -
    compiled with g++ under AddressSanitizer and UndefinedBehaviorSanitizer and run on the CPU."""
    exe = str(tmp_path / "posenc_plan")
    src = os.path.join(REPO, "tests", "native", "posenc_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    src, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "posenc_plan ok" in p.stdout, p.stdout + p.stderr


def test_loader_errors():
    import torch
    from range_amd.load_model import load_model
    with pytest.raises(NotImplementedError, match="s2vec_nosuch"):
        load_model("s2vec_nosuch", pretrained_path="x", device="cuda")
    with pytest.raises(ValueError, match="pretrained"):
        load_model("Theory")
    with pytest.raises(ValueError, match="RANGE / RANGE\\+"):
        load_model("Theory", pretrained_path="x", temp=20.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        load_model("s2vec_spherec", pretrained_path="x", device="cpu")
    if not torch.cuda.is_available():
        for name in NAMES:
            with pytest.raises(RuntimeError):
                load_model(name, pretrained_path="x", device="cuda")
