"""Host-side check of the decoder leader on the VRNN backward walk's spare range (csrc/vrnn_static.h): no GPU call."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_leader_deal_and_its_arming(tmp_path, sanitize):
    """1 .. 4 row tiles on 256, 128 and 64 workgroups, both tile orders: every leader tile owned once and within kMaxTiles, the phi
    part's tile on the workgroup of the same partial-sum tile, one partial-sum tile per armer and a power of two of armers per row
    tile, every polled word of the thirteen-descriptor program covered (T' = 3, 4, 5, 11, 250), and what the rules do not cover
    refused.  The second build runs the same stand-alone program under the address and undefined-behaviour sanitizers."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "bwd_dec_deal_test"
    src = os.path.join(ROOT, "tests", "host", "bwd_dec_deal_test.hip")
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'benchmarking-lvms_amd', 'csrc')}"]
    san = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", *san, *inc, src, "-o", str(exe)], check=True, timeout=600)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and ": 0 errors" in out.stdout and "4 of 4" in out.stdout, out.stdout + out.stderr
