"""Host-side check of the decoder range of the VRNN forward deal (csrc/vrnn_static.h): no GPU call."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decoder_range_of_the_forward_deal(tmp_path):
    """On 256 / 128 / 64 workgroups and 1 .. 4 row tiles the decoder's ranges are disjoint from the chain's, its resident links get one
    tile per workgroup, its last layer at most kMaxTiles, and the range is empty (six descriptors) when fewer than 8 workgroups are
    free."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "dec_deal_test"
    src = os.path.join(ROOT, "tests", "host", "dec_deal_test.hip")
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'benchmarking-lvms_amd', 'csrc')}"]
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", *inc, src, "-o", str(exe)], check=True, timeout=600)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and ": 0 errors" in out.stdout, out.stdout + out.stderr
