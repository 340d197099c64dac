"""The VRNN and SRNN one-launch roll-outs' step programs (csrc/rollout_plan.h) replayed on the host, as the LSTM's are
(tests/test_lstm_generate_cpu.py, tests/test_generate_any_stack_cpu.py): tests/host/rollout_replay.h walks a program word by word.

Run this file before the GPU tests of the roll-outs: the replay catches a polled word that no link writes, which on a device is a
launch that spins to its poll bound."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,total", [("vrnn_generate_plan_test", "80 cases, 0 errors"), ("srnn_generate_plan_test", "40 cases, 0 errors")])
def test_program_replayed_on_the_host(tmp_path, name, total):
    """S in {1, 5, 8, 16, 24} x B in {1, 17} x {256, 32} CUs x XCD placement off / on, T = 3, (H, Z, R) = (48, 16, 32) and for the VRNN
    also (48, 48, 32) (both arms of its Z == H branch): every polled read inside the sentinel-filled range and prefilled or written
    by exactly one earlier link, no word written twice outside the dummy regions (which nobody reads), every tile owned once, x_out
    complete at width S, u / v / eps / bias reads inside the caller's arrays or the scratch, the regions disjoint and ascending,
    h_out | d_out and z_out written; a program whose phi[3] link (VRNN) or head (SRNN) lost its second T16 output must be caught.
    No GPU call."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / name
    src = os.path.join(ROOT, "tests", "host", name + ".hip")
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'benchmarking-lvms_amd', 'csrc')}"]
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", *inc, src, "-o", str(exe)], check=True, timeout=600)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and total in out.stdout, out.stdout + out.stderr
