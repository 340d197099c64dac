"""Host-side check of the look-ahead arming plan of the static VRNN walks (csrc/vrnn_static.h): no GPU call."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_arming_plan_covers_every_polled_word(tmp_path, sanitize):
    """For the deals of B = 5, 17, 33, 49, 64 on 256 workgroups and T' = 1, 3, 4, 5, 11, 250, forward and backward, in both tile
    orders: the host's fill plus all workgroups' chunks cover every polled 16-byte word, no chunk leaves its buffer or its
    workgroup's row tile, every chunk is 16-byte aligned, and programs outside the rules are refused.  The second build runs the
    same stand-alone program under the address and undefined-behaviour sanitizers."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "arm_plan_test"
    src = os.path.join(ROOT, "tests", "host", "arm_plan_test.hip")
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'benchmarking-lvms_amd', 'csrc')}"]
    san = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", *san, *inc, src, "-o", str(exe)], check=True, timeout=600)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and ": 0 errors" in out.stdout and "7 of 7" in out.stdout, out.stdout + out.stderr
