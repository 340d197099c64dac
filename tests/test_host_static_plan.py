"""Host-side check of the static walk's resident-weight plan (csrc/vrnn_static.h): no GPU call."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_resident_links_deal_one_tile_per_workgroup(tmp_path):
    """For B = 1 .. 64 on 256 CUs the VRNN deal gives every register-resident link at most one tile per workgroup and every tile
    exactly one owner; on a chip too small for that the converter's condition fails, so the interpreter runs the program."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "static_plan_test"
    src = os.path.join(ROOT, "tests", "host", "static_plan_test.hip")
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'benchmarking-lvms_amd', 'csrc')}"]
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", *inc, src, "-o", str(exe)], check=True, timeout=600)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "0 errors" in out.stdout, out.stdout + out.stderr
