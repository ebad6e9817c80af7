"""The gfx950 assembly of range_amd/csrc/range_hip.hip for the tests that read the generated code
(test_host_cpu.py::test_no_foreign_m0_writes, test_pass2_codegen_cpu.py): one device-only compile per
test session, about a minute, shared by all of them."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _compile():
    if shutil.which("hipcc") is None:
        return None
    tmp = tempfile.mkdtemp(prefix="range_dev_asm_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    out = os.path.join(tmp, "dev.s")
    done = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                           "-o", out, os.path.join(REPO, "range_amd", "csrc", "range_hip.hip")],
                          cwd=REPO, capture_output=True, text=True)
    return out if done.returncode == 0 else RuntimeError("device compile failed:\n" + done.stderr[-4000:])


def device_asm():
    """Path of the assembly listing, or None where there is no hipcc.  A compile that fails is not tried
    again: every caller gets its error, with the compiler's messages."""
    res = _compile()
    if isinstance(res, Exception):
        raise res
    return res
