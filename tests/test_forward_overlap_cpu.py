"""The overlapped forward without a GPU: its chunk plan (host_plan.h: plan_forward_chunks) as a stand-alone
program under AddressSanitizer / UndefinedBehaviorSanitizer, and the resources of the pass-1 kernel that has to
fit beside pass 2 (pass1_beside.h), read from the generated gfx950 code."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chunk_plan_under_sanitizers(tmp_path):
    """B = 1 .. 40 000 against four bank sizes on three CU counts: the cuts cover the tiles once and in order,
    every chunk is whole rounds of pass 2 at least 98 % full, no round is added, no plan where the conditions say
    none, and the benchmark's shape gives 39 + 59 + 59 tiles."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "forward_chunks_plan")
    src = os.path.join(REPO, "tests", "native", "forward_chunks_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    src, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "forward_chunks_plan ok" in p.stdout, p.stdout + p.stderr


def test_the_kernel_beside_pass2_fits_what_pass2_leaves():
    """attend_stored_kernel takes 344 of a SIMD's 512 registers per lane: the kernel beside it has 168 (vector
    and accumulator registers together, in the allocation's granules of 8) and no scratch memory."""
    from device_asm import device_asm     # (tests/device_asm.py: one compile for all codegen tests)
    out = device_asm()
    if out is None:
        pytest.skip("hipcc not available")
    text = open(out).read()
    kernels = [k for k in re.split(r"\n(?=_ZN9range_hip\w+:)", text) if "scan_stats_beside_kernel" in k.split(":", 1)[0]]
    assert len(kernels) == 2
    for k in kernels:
        name = k.split(":", 1)[0]
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", k), f"{name} uses scratch memory"
        regs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", k).group(1))     # (unified file: AGPRs included)
        assert (regs + 7) // 8 * 8 <= 168, f"{name}: {regs} registers"
    # the asm MFMAs of the new kernel obey the rule of the others (engine_prims.h: mfma_v)
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_mfma_war", os.path.join(REPO, "tools", "check_mfma_war.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    bad = mod.check(str(out), ["scan_stats_beside_kernel"])
    assert not bad, bad[:5]
