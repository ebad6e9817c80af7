"""Compare two device assembly listings of the same translation unit, kernel by kernel (CPU only).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S range_amd/csrc/range_hip.hip -o X.s
    python tools/kernel_asm_diff.py PARENT.s BRANCH.s

For a refactor that must not change the generated code.  Per kernel symbol: identical or not, and for
those that differ NumVgprs / NumAgprs / ScratchSize / Occupancy of both sides and, for the innermost
backward-branch region that holds an MFMA, the instruction counts, whether the register-masked
instruction sequence is equal and whether the opcode multiset is equal.  Exit status 1 if the symbol
sets differ, or if ScratchSize, NumAgprs or Occupancy differ anywhere.  Kernels are compared independent
of the order the compiler emitted them in (the function ordinal of local labels is masked), so moving a
kernel table or an include in the source is no difference.  It compares what is there; it looks for no
particular instruction.
"""
import collections
import re
import sys

FIELDS = ("NumVgprs", "NumAgprs", "ScratchSize", "Occupancy")


def innermost_mfma_loop(body):
    """Lines of the shortest backward-branch region of ``body`` that contains an MFMA."""
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"(\.LBB[\d#]+_\d+):", l)] if m}
    best = None
    for i, l in enumerate(body):
        m = re.match(r"\s+s_c?branch\S*\s+(\.LBB[\d#]+_\d+)", l)
        if m and labels.get(m.group(1), i) < i:
            region = body[labels[m.group(1)]:i + 1]
            if any(re.match(r"\s+v_mfma", r) for r in region) and (best is None or len(region) < len(best)):
                best = region
    return best


def own_end(name, lines):
    """Number of lines of a kernel's chunk that are its own: up to its ``.size`` line (its
    ``.end_amdhsa_kernel`` where there is none) and the resource block that follows it (blank lines,
    comments, the symbol's ``.set`` lines and their section).  What the assembler puts behind the last
    kernel - padding, the translation unit's ``__hip_cuid_<hash>`` object - is not the kernel's."""
    ends = [i for i, l in enumerate(lines) if re.match(rf"\s*\.size\s+{re.escape(name)}\s*,", l)] or \
           [i for i, l in enumerate(lines) if re.match(r"\s*\.end_amdhsa_kernel\b", l)]
    n = ends[-1] + 1
    own = re.compile(rf"\s*($|;|\.set\s+{re.escape(name)}\.|\.section\s+\.AMDGPU\.csdata\b)")
    while n < len(lines) and own.match(lines[n]):
        n += 1
    return n


def without_ordinal(text):
    """Local labels carry the ordinal of their function in the listing (``.LBB<f>_<n>``, ``BB<f>_<n>`` in
    LLVM's comments, ``.Lfunc_begin<f>`` / ``.Lfunc_end<f>``): the order in which the compiler emitted the
    kernels, which follows the order of the source.  A fixed token takes its place; the block number stays."""
    return re.sub(r"(\.LBB|\bBB|\.Lfunc_begin|\.Lfunc_end)\d+(?=_\d|\b)", r"\1#", text)


def kernels(text):
    """{symbol: text from its label to its own end, without function ordinals} for every kernel of a listing."""
    chunks = re.split(r"\n(?=[A-Za-z_][\w$.]*:)", text)
    out = {}
    for c in chunks:
        if re.search(r"^\s*\.amdhsa_kernel\s", c, re.M):
            name, lines = c.split(":", 1)[0], c.split("\n")
            out[name] = without_ordinal("\n".join(lines[:own_end(name, lines)]))
    return out


def instructions(lines):
    """Instructions of a region without comments, labels and directives."""
    code = (l.split(";")[0].strip() for l in lines)
    return [c for c in code if c and not c.endswith(":") and not c.startswith((".", "#"))]


def masked(code):
    """Register numbers and local labels replaced: what is left is opcodes, operand kinds, immediates."""
    return [re.sub(r"\.LBB[\d#]+_\d+", "L", re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1#", c)) for c in code]


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    a, b = (kernels(open(p).read()) for p in argv[1:])
    status = 0
    for name in sorted(set(a) ^ set(b)):
        print(f"only in {'parent' if name in a else 'branch'}: {name}")
        status = 1
    n_same = 0
    for name in sorted(set(a) & set(b)):
        if a[name] == b[name]:
            n_same += 1
            continue
        print(f"differs: {name}")
        for f in FIELDS:
            va, vb = (re.search(rf"; {f}: (\d+)", k) for k in (a[name], b[name]))
            va, vb = (int(v.group(1)) if v else None for v in (va, vb))
            flag = ""
            if va != vb and f != "NumVgprs":
                flag, status = "   <-- must be equal", 1
            print(f"    {f:12s} {va} -> {vb}{flag}")
        la, lb = (innermost_mfma_loop(k.splitlines()) for k in (a[name], b[name]))
        if la is None or lb is None:
            print(f"    inner MFMA loop: {'none' if la is None and lb is None else 'on one side only'}")
            continue
        ca, cb = instructions(la), instructions(lb)
        ops = lambda code: collections.Counter(c.split()[0] for c in code)
        print(f"    inner MFMA loop: {len(ca)} -> {len(cb)} instructions; register-masked sequence "
              f"{'equal' if masked(ca) == masked(cb) else 'DIFFERS'}; opcode multiset "
              f"{'equal' if ops(ca) == ops(cb) else 'DIFFERS'}")
    print(f"{len(a)} / {len(b)} kernel symbols, {n_same} identical; exit status {status}")
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv))
