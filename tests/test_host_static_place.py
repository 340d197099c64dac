"""Host-side check of the static walk's launch placement (csrc/vrnn_static.h Place, place_wg): no GPU call."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_placement_is_a_range_keeping_bijection(tmp_path):
    """For B = 1 .. 64 on 256 and on 64 CUs and every placement: the block-index map is a bijection of the grid that keeps every
    link's range, every tile has one owner, the resident links still deal at most one tile per workgroup, and with four row tiles on
    256 CUs the prior (posterior) run of row tile r lands on blocks with index % 8 == r (r + 4); elsewhere the local placement falls
    back to the plain one."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "static_place_test"
    src = os.path.join(ROOT, "tests", "host", "static_place_test.hip")
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'benchmarking-lvms_amd', 'csrc')}"]
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", *inc, src, "-o", str(exe)], check=True, timeout=600)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "0 errors" in out.stdout, out.stdout + out.stderr
