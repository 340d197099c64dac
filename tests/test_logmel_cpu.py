"""Host side of the log-mel front end (K10): the basis and filterbank builders against their formulas, frame counts, the transform's
defaults, and every refusal that needs no device (CPU tensors, short rows, out-of-range geometry, the library's own checks).
No GPU."""
import ctypes
import math
import os
import subprocess
import sys

import pytest
import torch

from blvm import _hip, ops
from blvm.data.transforms import LogMelSpectrogram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hz_to_mel(f):
    return 2595.0 * math.log10(1.0 + f / 700.0)


def mel_to_hz(m):
    return 700.0 * (10.0 ** (m / 2595.0) - 1.0)


@pytest.mark.parametrize("sample_rate,n_fft,n_mels", [(16000, 512, 80), (16000, 400, 80), (16000, 64, 8), (16000, 128, 40), (8000, 256, 128)])
def test_filterbank_against_the_formula(sample_rate, n_fft, n_mels):
    """Element by element in python floats: fb[k, m] = max(0, min(down, up)) of the two slopes of triangle m at frequency k."""
    fb = ops.logmel_filterbank(sample_rate, n_fft, n_mels)
    n_bins = n_fft // 2 + 1
    assert fb.dtype == torch.float64 and tuple(fb.shape) == (n_bins, n_mels)
    m_max = hz_to_mel(sample_rate / 2)
    pts = [mel_to_hz(m_max * i / (n_mels + 1)) for i in range(n_mels + 2)]
    worst = 0.0
    for k in range(n_bins):
        f = (sample_rate // 2) * k / (n_bins - 1)
        for m in range(n_mels):
            down = (f - pts[m]) / (pts[m + 1] - pts[m])
            up = (pts[m + 2] - f) / (pts[m + 2] - pts[m + 1])
            worst = max(worst, abs(float(fb[k, m]) - max(0.0, min(down, up))))
    assert worst < 1e-9, worst  # float64 on both sides; the slopes divide differences of ~1e1..1e3 Hz
    assert float(fb.min()) >= 0.0 and float(fb.max()) <= 1.0


def test_filter_zero_of_the_128_40_case_is_empty():
    """n_fft 128 at 16 kHz has bins 125 Hz apart, and filter 0 spans less than that between two of them: an all-zero filter, whose
    feature row is -100 dB throughout (the GPU test's constant-row case)."""
    fb = ops.logmel_filterbank(16000, 128, 40)
    assert float(fb[:, 0].abs().max()) == 0.0 and float(fb[:, 1].max()) > 0.0


@pytest.mark.parametrize("n_fft,win", [(512, 128), (400, 400), (64, 32), (128, 128), (30, 17)])
def test_basis_against_the_formula_and_the_fft(n_fft, win):
    basis = ops.logmel_basis(n_fft, win)
    n_bins, left = n_fft // 2 + 1, (n_fft - win) // 2
    assert basis.dtype == torch.float64 and tuple(basis.shape) == (win, 2, n_bins)
    for n, k in [(0, 0), (1, 1), (win - 1, n_bins - 1), (win // 2, 3), (win // 3, n_bins // 2)]:
        w = 0.5 - 0.5 * math.cos(2 * math.pi * n / win)
        ang = 2 * math.pi * k * (left + n) / n_fft
        assert abs(float(basis[n, 0, k]) - w * math.cos(ang)) < 1e-12 and abs(float(basis[n, 1, k]) - w * math.sin(ang)) < 1e-12
    # a frame times the basis is the rfft of the windowed frame zero-padded to n_fft
    frame = torch.randn(win, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    padded = torch.zeros(n_fft, dtype=torch.float64)
    padded[left : left + win] = frame * torch.hann_window(win, periodic=True, dtype=torch.float64)
    ref = torch.fft.rfft(padded)
    assert torch.allclose(frame @ basis[:, 0], ref.real, atol=1e-10) and torch.allclose(frame @ basis[:, 1], -ref.imag, atol=1e-10)


def test_operand_padding():
    """What the kernel reads: basis [WP,2,NBP], fbank [NBP,NMP] in fp32, zero outside the real rows and columns."""
    basis, fbank = ops._logmel_operands("cpu", 16000, 400, 396, 80)
    assert tuple(basis.shape) == (400, 2, 224) and tuple(fbank.shape) == (224, 96) and basis.dtype == fbank.dtype == torch.float32
    assert float(basis[396:].abs().max()) == 0.0 and float(basis[:, :, 201:].abs().max()) == 0.0
    assert float(fbank[201:].abs().max()) == 0.0 and float(fbank[:, 80:].abs().max()) == 0.0
    assert torch.equal(basis[:396, :, :201], ops.logmel_basis(400, 396).float())
    assert ops._logmel_operands("cpu", 16000, 400, 396, 80)[0] is basis  # cached per (device, geometry)


def test_frame_counts_match_torch_stft():
    for L, n_fft, hop in [(1000, 512, 64), (777, 400, 200), (300, 512, 64), (257, 512, 64), (1024, 64, 16), (999, 64, 1000)]:
        spec = torch.stft(torch.zeros(L), n_fft, hop_length=hop, window=torch.ones(n_fft), center=True, pad_mode="reflect", return_complex=True)
        assert ops.logmel_frames(L, hop) == spec.shape[-1] == 1 + L // hop


def test_transform_defaults_are_the_reference_s():
    t = LogMelSpectrogram()
    assert (t.sample_rate, t.n_fft, t.win_length, t.hop_length, t.n_mels, t.normalize_frq_bins) == (16000, 400, 400, 200, 80, True)
    t = LogMelSpectrogram(16000, 512, 128)
    assert (t.win_length, t.hop_length) == (128, 64)
    t = LogMelSpectrogram(n_fft=512, hop_length=100, n_mels=40, normalize_frq_bins=False)
    assert (t.win_length, t.hop_length, t.n_mels, t.normalize_frq_bins) == (512, 100, 40, False)


def test_cpu_tensors_are_refused():
    with pytest.raises(_hip.BlvmHipError):
        ops.log_mel_spectrogram(torch.zeros(2, 1000), [1000, 900], 16000, 512, 128, 64, 80)
    with pytest.raises(_hip.BlvmHipError):
        LogMelSpectrogram()(torch.zeros(1000))
    with pytest.raises(_hip.BlvmHipError):
        LogMelSpectrogram()(torch.zeros(2, 1000), torch.tensor([1000, 900]))


def test_short_rows_are_refused():
    ops.logmel_check_lengths([1000, 257], 512, 1000)
    with pytest.raises(_hip.BlvmHipError, match="row 1 has 256 samples"):
        ops.logmel_check_lengths([1000, 256], 512, 1000)
    with pytest.raises(_hip.BlvmHipError, match="row 0 has 1001 samples"):
        ops.logmel_check_lengths([1001, 300], 512, 1000)


BAD_GEOMETRY = [(511, 128, 64, 80), (2048, 128, 64, 80), (512, 8, 64, 80), (512, 600, 64, 80), (512, 128, 0, 80), (512, 128, 64, 0),
                (512, 128, 64, 129)]  # fmt: skip


@pytest.mark.parametrize("n_fft,win,hop,n_mels", BAD_GEOMETRY)
def test_out_of_range_geometry_is_refused(n_fft, win, hop, n_mels):
    with pytest.raises(_hip.BlvmHipError):
        ops.logmel_check_geometry(n_fft, win, hop, n_mels)
    with pytest.raises(_hip.BlvmHipError):
        LogMelSpectrogram(16000, n_fft, win, hop, n_mels)
    # the library checks before it touches a pointer or the device: -1 and a message
    lib = _hip.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert lib.blvm_logmel(p, p, 2, 1000, n_fft, win, hop, n_mels, p, p, 1, p, p, None) == -1
    assert b"blvm_logmel" in lib.blvm_last_error()


def test_library_refuses_shapes_and_null_pointers():
    lib = _hip.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert lib.blvm_logmel(p, p, 2, 256, 512, 128, 64, 80, p, p, 1, p, p, None) == -1  # no row can hold more than n_fft / 2
    assert lib.blvm_logmel(p, p, 0, 1000, 512, 128, 64, 80, p, p, 1, p, p, None) == -1
    assert lib.blvm_logmel(p, p, 2**20, 2**22, 512, 128, 1, 80, p, p, 1, p, p, None) == -1 and b"2^31" in lib.blvm_last_error()
    assert lib.blvm_logmel(p, p, 2, 1000, 512, 128, 64, 80, p, p, 2, p, p, None) == -1
    assert lib.blvm_logmel(p, None, 2, 1000, 512, 128, 64, 80, p, p, 1, p, p, None) == -1 and b"NULL" in lib.blvm_last_error()
    for n_fft, win, hop, n_mels in [(512, 128, 64, 80), (400, 400, 200, 80), (1024, 1024, 4096, 128), (16, 16, 1, 1)]:
        ops.logmel_check_geometry(n_fft, win, hop, n_mels)  # the two geometries that matter, and the corners of the range


def test_experiment_help_lists_the_front_end_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "experiments", "experiment_asr_ctc.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for flag in ("--n_mels", "--n_fft", "--win_length", "--hop_length"):
        assert flag in r.stdout
