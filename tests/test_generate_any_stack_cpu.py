"""One-launch generation at frame stacks that are no multiple of 16, on the CPU: the LSTM cases the GPU tests
(tests/test_gpu_generate_any_stack.py) compare against the float64 restatement of tests/test_lstm_generate_cpu.py, the properties that
make that comparison meaningful, the host replay of the padded LSTM program, and the arithmetic of the scratch bound.

The shapes are the smallest at which each padded place can go wrong (H = 32, T from 3 to 7):
  S = 1   rows of 30 floats (not 16-byte aligned unpadded), one live sample in a 4-sample tile, K padded from 1 to 16, 30 columns over 2 tiles
  S = 5   odd, 150 columns (a ragged last tile), a second draw tile with one live sample
  S = 8   the reference fixture's size, half an operand tile, 240 columns = exactly 15 tiles
  S = 24  two operand tiles, the second half full
with B = 1, 5 (a partial row group) and 17 (two row groups, the second with one row): every S with B = 17, every B with S = 1.

The seeds were picked here, on the CPU, so that every case's smallest float64 gap between the best and the second-best perturbed
logit is >= 2e-3 (asserted at MIN_GAP = 1e-3 below): a component can then not flip within the comparison's 1e-4.

Run this file first: the replay catches a pad word that no link writes, which on a device is a launch that spins to its poll bound.
"""
import functools
import inspect
import os
import shutil
import subprocess

import pytest
import torch

from test_lstm_generate_cpu import MIN_GAP, Case, build_model, inputs, lstm_audio_generate_f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Case: S H L B T start mode seeds (tests/test_lstm_generate_cpu.py)
CASES = {
    "s1b1": Case(1, 32, 1, 1, 7, "x0h0", False, (20, 300)),
    "s1b5": Case(1, 32, 2, 5, 5, "x0", False, (21, 310)),
    "s1b17": Case(1, 32, 1, 17, 7, "x0h0", False, (22, 320)),
    "s5b17": Case(5, 32, 2, 17, 4, "x0h0", False, (23, 330)),
    "s8b17": Case(8, 32, 1, 17, 3, "zeros", False, (24, 340)),
    "s24b17": Case(24, 32, 2, 17, 3, "x0h0", False, (25, 368)),
    "s5b5m": Case(5, 32, 1, 5, 4, "x0h0", True, (28, 360)),  # use_mode=True
}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(model on the CPU, x0, s0, uniforms, float64 samples [B,T,S], float64 (h_n, c_n), smallest gap) of a case — computed once,
    never changed."""
    case = CASES[name]
    m = build_model(case)
    x0, s0, uni = inputs(case)
    sd64 = {k: v.detach().double() for k, v in m.state_dict().items()}
    x64, s64, gap = lstm_audio_generate_f64(sd64, x0, s0, uni, case.T, case.B, case.S, case.H, case.L, case.mode)
    return m, x0, s0, uni, x64, s64, gap


def test_cases_cover_the_shapes():
    assert {c.S for c in CASES.values()} == {1, 5, 8, 24} and {c.L for c in CASES.values()} == {1, 2}
    assert {c.S for c in CASES.values() if c.B == 17} == {1, 5, 8, 24} and {c.B for c in CASES.values() if c.S == 1} == {1, 5, 17}
    assert any(c.mode for c in CASES.values()) and all(c.H == 32 and 3 <= c.T <= 7 for c in CASES.values())


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_have_no_near_ties(name):
    gap = reference(name)[6]
    assert gap >= MIN_GAP, f"case {name}: (perturbed-)logit gap {gap:.2e}: pick another seed"


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_are_not_vacuous(name):
    """At least half of the samples lie strictly inside (-1, 1) — a comparison of clamped values would show nothing — and the rows
    differ from each other and from step to step."""
    case = CASES[name]
    x64 = reference(name)[4]
    assert tuple(x64.shape) == (case.B, case.T, case.S)
    assert float((x64.abs() < 1).double().mean()) >= 0.5
    assert float((x64[:, 1:] - x64[:, :-1]).abs().max()) > 1e-3
    if case.B > 1:
        assert float((x64[1:] - x64[:-1]).abs().max()) > 1e-3


def test_padded_program_replayed_on_the_host(tmp_path):
    """tests/host/lstm_decode_ragged_plan_test.hip (on tests/host/rollout_replay.h): the program of csrc/lstm_decode.h for S in {1, 5, 8, 24} x B in {1, 17} x {1, 2}
    layers x T = 3 on 256 and 32 CUs, with and without XCD-aware placement, replayed word by word — every polled word a link reads
    (the pad columns of the frame-stack operand and of the last decoder layer included) prefilled or written by exactly one earlier
    link, no word written twice, x_out complete at width S, no read past the caller's u, v or bias, the regions disjoint; programs
    that leave the pad columns unwritten or read the unpadded bias must be caught.  No GPU call."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "lstm_decode_ragged_plan_test"
    src = os.path.join(ROOT, "tests", "host", "lstm_decode_ragged_plan_test.hip")
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'benchmarking-lvms_amd', 'csrc')}"]
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", *inc, src, "-o", str(exe)], check=True, timeout=600)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "64 cases, 0 errors" in out.stdout, out.stdout + out.stderr


def test_steps_per_launch_fills_the_bound():
    """The chunking arithmetic of blvm.ops: the most steps whose scratch fits, everything at once when it all fits, an error when
    not even one step fits; the default bound is the named constant, 2**28 floats."""
    from blvm import ops

    assert ops.MAX_SCRATCH_FLOATS == 2**28
    floats = lambda n: 1000 + 96 * n  # noqa: E731  (weight copies + one slab per step)
    for T, bound, want in ((7, 10**9, 7), (7, 1000 + 96 * 3, 3), (7, 1000 + 96 * 4 - 1, 3), (7, 1096, 1), (2, 1000 + 96 * 5, 2)):
        assert ops._steps_per_launch(floats, T, bound, "test") == want
    assert ops._steps_per_launch(floats, 5, None, "test") == 5
    assert ops._steps_per_launch(lambda n: 2**20 * n, 2**12, None, "test") == 2**8
    with pytest.raises(ValueError):
        ops._steps_per_launch(floats, 7, 1095, "test")
    for f in (ops.vrnn_decode, ops.srnn_generate, ops.lstm_generate):
        assert inspect.signature(f).parameters["max_scratch_floats"].default is None
