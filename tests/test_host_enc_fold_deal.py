"""Host-side check of the d_enc follower on the VRNN backward walk's posterior half (csrc/vrnn_static.h): no GPU call."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_follower_deal_its_writes_and_its_arming(tmp_path, sanitize):
    """B = 1 .. 64, T' = 3, 4, 5, 6, 11, both tile orders, with and without the decoder leader: one tile of each follower link on every
    workgroup of the posterior half and nowhere else, the same tile of both; every word of EP and d_enc written exactly once over the
    replayed walk; every polled word of the extended program armed exactly once and in front of its producer; arm_applies accepts the
    extended programs and refuses the mutated ones.  The second build runs the same stand-alone program under the address and
    undefined-behaviour sanitizers."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "enc_fold_deal_test"
    src = os.path.join(ROOT, "tests", "host", "enc_fold_deal_test.hip")
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'benchmarking-lvms_amd', 'csrc')}"]
    san = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", *san, *inc, src, "-o", str(exe)], check=True, timeout=600)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and ": 0 errors" in out.stdout and "10 of 10" in out.stdout, out.stdout + out.stderr
