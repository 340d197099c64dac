"""Host-side check of the three-slice split of fp32 operands (csrc/bf16_slice.h) behind the sliced weight-gradient tile: no GPU call."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_three_slices_reproduce_every_finite_float(tmp_path, sanitize):
    """hi + mid + lo == x exactly over signed zeros, FLT_MIN, subnormals, FLT_MAX, full significands at every exponent and 10^6 random
    bit patterns; every slice bf16-exact wherever x is a multiple of the bf16 subnormal spacing 2^-133 (all |x| >= 2^-110), the packed
    slices within 2^-133 of x below that; inf and NaN give NaN slices.  The second build runs the same stand-alone program under the
    address and undefined-behaviour sanitizers."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "slice_split_test"
    src = os.path.join(ROOT, "tests", "host", "slice_split_test.hip")
    inc = [f"-I{os.path.join(ROOT, 'benchmarking-lvms_amd', 'csrc')}"]
    san = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", *san, *inc, src, "-o", str(exe)], check=True, timeout=600)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and ": 0 errors" in out.stdout, out.stdout + out.stderr
