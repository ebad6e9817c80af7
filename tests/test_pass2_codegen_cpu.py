"""The generated gfx950 code of pass 2 on kept logits (attend_stored_kernel<true>), from the compile
that tests/test_host_cpu.py::test_no_foreign_m0_writes reads too (tests/device_asm.py).  What the
block-granular V ring and the scalar weight arithmetic promise is visible in the inner loop (the
innermost loop that holds MFMAs):

  * no packed float32 arithmetic beside the MFMAs (hipcc's SLP vectoriser packed the weights' scalings
    of neighbouring rows into one MFMA gap before they were written as single instructions);
  * one workgroup barrier per block: 256 product MFMAs + the geographic one per s_barrier;
  * no accumulator leaves the AGPR file and nothing is spilled inside the loop;
  * the kernel uses no scratch memory and holds its 64 accumulator tiles in 256 AGPRs.
"""
import re

import pytest

from device_asm import device_asm                      # (one compile for all codegen tests)
from tools import kernel_asm_diff
from tools.kernel_asm_diff import innermost_mfma_loop as _innermost_mfma_loop


def _kernel(prefix):
    """The one kernel of the device assembly whose symbol starts with ``prefix``."""
    out = device_asm()
    if out is None:
        pytest.skip("hipcc not available")
    kernels = [k for k in re.split(r"\n(?=_ZN9range_hip\w+:)", open(out).read())
               if k.startswith(prefix)]
    assert len(kernels) == 1
    return kernels[0]


def test_inner_loop_of_the_kept_logit_pass2():
    k = _kernel("_ZN9range_hip20attend_stored_kernelILb1E")
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


def test_inner_loop_of_the_recompute_pass2():
    """attend_kernel<true, false>: the same register file and one block per loop body - 256 product
    MFMAs, the 64 of the next block's semantic logits and the geographic one, over two barriers (one
    per half block).  (Nothing is asserted on packed arithmetic here: this loop forms its weights in
    C++, and hipcc packs some of them.)"""
    k = _kernel("_ZN9range_hip13attend_kernelILb1ELb0E")
    assert re.search(r"; ScratchSize: 0\b", k) and re.search(r"\.amdhsa_private_segment_fixed_size 0\b", k)
    assert re.search(r"; NumAgprs: 256\b", k)
    loop = _innermost_mfma_loop(k.splitlines())
    assert loop is not None
    code = [l.split(";")[0].strip() for l in loop]
    count = lambda pat: sum(1 for l in code if re.match(pat, l))
    assert count(r"v_mfma") == count(r"v_mfma_f32_16x16x4_f32\b") == 321
    assert count(r"s_barrier\b") == 2
    moved = [l for l in code if re.match(r"(v_accvgpr_|scratch_)", l)]
    assert not moved, moved[:4]


def _cuid_object(cuid):
    """What closes a listing: the object hipcc names after a hash of the translation unit's sources."""
    return (f"\t.text\n\t.p2alignl 6, 3212836864\n\t.type\t__hip_cuid_{cuid},@object\n\t.section\t.bss,\"aw\",@nobits\n"
            f"\t.globl\t__hip_cuid_{cuid}\n__hip_cuid_{cuid}:\n\t.byte\t0\n\t.size\t__hip_cuid_{cuid}, 1\n"
            f"\t.addrsig_sym __hip_cuid_{cuid}\n")


def _listing(cuid):
    """A listing of two kernels in hipcc's layout, closed by the translation unit's ``__hip_cuid`` object."""
    def kernel(name, body):
        return (f"\t.text\n\t.protected\t{name}\n\t.globl\t{name}\n\t.type\t{name},@function\n"
                f"{name}:\n; %bb.0:\n{body}\ts_endpgm\n"
                f"\t.section\t.rodata,\"a\",@progbits\n\t.amdhsa_kernel {name}\n\t\t.amdhsa_next_free_vgpr 8\n"
                f"\t.end_amdhsa_kernel\n\t.text\n.Lfunc_end0:\n\t.size\t{name}, .Lfunc_end0-{name}\n"
                f"\t.set {name}.num_vgpr, 8\n\t.section\t.AMDGPU.csdata,\"\",@progbits\n; Kernel info:\n"
                f"; NumVgprs: 8\n; NumAgprs: 0\n; ScratchSize: 0\n; Occupancy: 8\n")
    return kernel("first_kernel", "\tv_mov_b32_e32 v0, 0\n") + kernel("last_kernel", "\tv_mov_b32_e32 v1, 1\n") + _cuid_object(cuid)


def test_asm_diff_ends_a_kernel_at_its_own_end(tmp_path, capsys):
    """tools/kernel_asm_diff.py: the object hipcc names after a hash of the sources follows the last
    kernel of a listing and is no part of it - two listings that differ in nothing else hold no
    differing kernel, and a kernel's chunk still carries its resource block."""
    a, b = _listing("48af349932bb732f"), _listing("0123456789abcdef")
    ka, kb = kernel_asm_diff.kernels(a), kernel_asm_diff.kernels(b)
    assert sorted(ka) == ["first_kernel", "last_kernel"] and ka == kb
    assert all("; NumAgprs: 0" in k and "; Occupancy: 8" in k and "__hip_cuid" not in k for k in ka.values())
    (tmp_path / "a.s").write_text(a)
    (tmp_path / "b.s").write_text(b)
    assert kernel_asm_diff.main(["kernel_asm_diff", str(tmp_path / "a.s"), str(tmp_path / "b.s")]) == 0
    out = capsys.readouterr().out
    assert "differs" not in out and "2 identical" in out
    # a change inside a kernel is still one
    (tmp_path / "b.s").write_text(b.replace("v_mov_b32_e32 v1, 1", "v_mov_b32_e32 v1, 2"))
    kernel_asm_diff.main(["kernel_asm_diff", str(tmp_path / "a.s"), str(tmp_path / "b.s")])
    assert "differs: last_kernel" in capsys.readouterr().out


def _loop_kernel(name, f, op):
    """A kernel with a loop, in hipcc's layout, emitted as the ``f``-th function of its listing."""
    return (f"\t.text\n\t.protected\t{name}\n\t.globl\t{name}\n\t.type\t{name},@function\n"
            f"{name}:\n.Lfunc_begin{f}:\n; %bb.0:\n\ts_mov_b32 s0, 0\n.LBB{f}_1:\n\t{op}\n\ts_add_i32 s0, s0, 1\n"
            f"\ts_cmp_lt_i32 s0, 8\n\ts_cbranch_scc1 .LBB{f}_1\n; %bb.2:                ; %exit, from BB{f}_1\n\ts_endpgm\n"
            f"\t.section\t.rodata,\"a\",@progbits\n\t.amdhsa_kernel {name}\n\t\t.amdhsa_next_free_vgpr 8\n"
            f"\t.end_amdhsa_kernel\n\t.text\n.Lfunc_end{f}:\n\t.size\t{name}, .Lfunc_end{f}-{name}\n"
            f"\t.set {name}.num_vgpr, 8\n\t.section\t.AMDGPU.csdata,\"\",@progbits\n; Kernel info:\n"
            f"; NumVgprs: 8\n; NumAgprs: 0\n; ScratchSize: 0\n; Occupancy: 8\n")


def test_asm_diff_is_independent_of_emission_order(tmp_path, capsys):
    """The same two kernels emitted in swapped order carry each other's function ordinal in their local labels
    (.LBB<f>_<n>, BB<f>_<n> in comments, .Lfunc_begin<f> / .Lfunc_end<f>) and differ in nothing else: no kernel
    differs.  A changed instruction inside one of them still does, and the block number is still compared."""
    x, y = "v_add_f32_e32 v0, v0, v1", "v_mul_f32_e32 v0, v0, v1"
    a = _loop_kernel("first_kernel", 0, x) + _loop_kernel("last_kernel", 1, y) + _cuid_object("48af349932bb732f")
    b = _loop_kernel("last_kernel", 0, y) + _loop_kernel("first_kernel", 1, x) + _cuid_object("48af349932bb732f")
    assert ".LBB0_1" in a and "BB1_1" in a and ".Lfunc_end1-last_kernel" in a
    (tmp_path / "a.s").write_text(a)
    (tmp_path / "b.s").write_text(b)
    assert kernel_asm_diff.main(["kernel_asm_diff", str(tmp_path / "a.s"), str(tmp_path / "b.s")]) == 0
    out = capsys.readouterr().out
    assert "differs" not in out and "2 / 2 kernel symbols, 2 identical" in out
    (tmp_path / "b.s").write_text(b.replace(x, "v_sub_f32_e32 v0, v0, v1"))
    kernel_asm_diff.main(["kernel_asm_diff", str(tmp_path / "a.s"), str(tmp_path / "b.s")])
    out = capsys.readouterr().out
    assert "differs: first_kernel" in out and "differs: last_kernel" not in out and "1 identical" in out
    (tmp_path / "b.s").write_text(b.replace("s_cbranch_scc1 .LBB0_1", "s_cbranch_scc1 .LBB0_2"))
    kernel_asm_diff.main(["kernel_asm_diff", str(tmp_path / "a.s"), str(tmp_path / "b.s")])
    assert "differs: last_kernel" in capsys.readouterr().out
