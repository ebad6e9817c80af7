"""The generated gfx950 code of pass 2 on kept logits (attend_stored_kernel<true>), compiled as
tests/test_host_cpu.py::test_no_foreign_m0_writes compiles it.  What the block-granular V ring and the
scalar weight arithmetic promise is visible in the inner loop (the innermost loop that holds MFMAs):

  * no packed float32 arithmetic beside the MFMAs (hipcc's SLP vectoriser packed the weights' scalings
    of neighbouring rows into one MFMA gap before they were written as single instructions);
  * one workgroup barrier per block: 256 product MFMAs + the geographic one per s_barrier;
  * no accumulator leaves the AGPR file and nothing is spilled inside the loop;
  * the kernel uses no scratch memory and holds its 64 accumulator tiles in 256 AGPRs.
"""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _innermost_mfma_loop(body):
    """Lines of the shortest backward-branch region of ``body`` that contains an MFMA."""
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"(\.LBB\d+_\d+):", l)] if m}
    best = None
    for i, l in enumerate(body):
        m = re.match(r"\s+s_c?branch\S*\s+(\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), i) < i:
            region = body[labels[m.group(1)]:i + 1]
            if any(re.match(r"\s+v_mfma", r) for r in region) and (best is None or len(region) < len(best)):
                best = region
    return best


def test_inner_loop_of_the_kept_logit_pass2(tmp_path):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    out = tmp_path / "dev.s"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                    "-o", str(out), os.path.join(REPO, "range_amd", "csrc", "range_hip.hip")],
                   check=True, cwd=REPO, capture_output=True)
    kernels = [k for k in re.split(r"\n(?=_ZN9range_hip\w+:)", out.read_text())
               if k.startswith("_ZN9range_hip20attend_stored_kernelILb1E")]
    assert len(kernels) == 1
    k = kernels[0]
    assert re.search(r"; ScratchSize: 0\b", k) and re.search(r"\.amdhsa_private_segment_fixed_size 0\b", k)
    assert re.search(r"; NumAgprs: 256\b", k)
    loop = _innermost_mfma_loop(k.splitlines())
    assert loop is not None
    code = [l.split(";")[0].strip() for l in loop]
    count = lambda pat: sum(1 for l in code if re.match(pat, l))
    n_mfma, n_bar = count(r"v_mfma_f32_16x16x4_f32\b"), count(r"s_barrier\b")
    assert count(r"v_mfma") == n_mfma                        # no other MFMA shape in the loop
    assert n_bar >= 1 and n_mfma == 257 * n_bar, (n_mfma, n_bar)
    packed = [l for l in code if re.match(r"v_pk_(mul|fma|add)_f32\b", l)]
    assert not packed, packed[:4]
    moved = [l for l in code if re.match(r"(v_accvgpr_|scratch_)", l)]
    assert not moved, moved[:4]
