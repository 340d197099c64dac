"""K10, the log-mel front end on the device, against a float64 restatement that shares nothing with the kernel's GEMM form:
per utterance `torch.stft` (centred, reflect-padded about the utterance's OWN ends, periodic Hann of win_length) -> |.|^2 -> the
HTK filterbank from its formula -> 10 log10(max(., 1e-10)) -> (x - mean) / (unbiased std + 1e-10) per mel bin.

Signals: two sines (440 Hz at 0.3, 3100 Hz at 0.1) plus seeded white noise of amplitude 1e-2.  The noise floor is a condition: without
it some mel bins sit 90 dB down, where fp32 cancellation makes stock fp32 `torch.stft` itself differ from float64 by 0.07-0.5 dB;
with it the lowest bin is near -40 dB.

Tolerance: an fp32 CPU restatement of the kernel's GEMM form (frames gathered by index, F @ C, F @ S, filterbank matmul) is compared
with the float64 oracle in the test, per case; the kernel has the same count of fp32 roundings per sum in another order and gets 4x
that measured error, raw (dB) and normalised.  Every figure is printed before it is asserted."""
import functools

import pytest
import torch

from blvm import _hip, ops
from blvm.data.token_map import TokenMap
from blvm.data.transforms import LogMelSpectrogram
from blvm.models import SimpleLSTMASR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR = 16000
# (n_fft, win_length, hop_length, n_mels), lengths
CASES = {
    "probe-512-128-64-80": ((512, 128, 64, 80), (1000, 777, 300)),  # the probe's geometry; 300 is just above n_fft // 2 (with 257 below)
    "torchaudio-400-400-200-80": ((400, 400, 200, 80), (1000, 777, 300)),  # win == n_fft, 201 bins, depth 400
    "small-64-32-16-8": ((64, 32, 16, 8), (1000, 777, 300)),  # everything smaller than one tile
    "empty-filter-128-128-64-40": ((128, 128, 64, 40), (1000, 777)),  # filter 0 is all zero: a constant -100 dB row
    # the kernel's other paths: frames that do not overlap (hop > win_length: staged back to back), an odd hop (no bank skew) with a
    # win_length that is no multiple of the k unroll, and the largest geometry (148 KB of LDS, five chunks of bins, four mel tiles)
    "gaps-64-32-100-8": ((64, 32, 100, 8), (1000, 777, 300)),
    "odd-64-30-7-8": ((64, 30, 7, 8), (1000, 777, 300)),
    "largest-1024-1024-1024-128": ((1024, 1024, 1024, 128), (9000, 7000, 3000)),
}


def signal(length, seed):
    t = torch.arange(length, dtype=torch.float64) / SR
    noise = torch.randn(length, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))
    return (0.3 * torch.sin(2 * torch.pi * 440.0 * t) + 0.1 * torch.sin(2 * torch.pi * 3100.0 * t) + 1e-2 * noise).float()


def filterbank64(n_fft, n_mels):
    freqs = torch.linspace(0, SR // 2, n_fft // 2 + 1, dtype=torch.float64)
    m_max = 2595.0 * torch.log10(torch.tensor(1.0 + (SR / 2) / 700.0, dtype=torch.float64))
    pts = 700.0 * (10.0 ** (torch.linspace(0.0, float(m_max), n_mels + 2, dtype=torch.float64) / 2595.0) - 1.0)
    down = (freqs[:, None] - pts[None, :-2]) / (pts[1:-1] - pts[:-2])[None, :]
    up = (pts[None, 2:] - freqs[:, None]) / (pts[2:] - pts[1:-1])[None, :]
    return torch.minimum(down, up).clamp_min(0.0)


def decibel_and_normalised(mel):
    db = 10.0 * torch.log10(mel.clamp_min(1e-10))
    return db, (db - db.mean(-1, keepdim=True)) / (db.std(-1, keepdim=True) + 1e-10)


def oracle64(x, geometry):
    """float64, per utterance on its own samples: ([n_mels, T] dB, [n_mels, T] normalised)."""
    n_fft, win, hop, n_mels = geometry
    spec = torch.stft(x.double(), n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win, periodic=True, dtype=torch.float64),
                      center=True, pad_mode="reflect", return_complex=True)  # fmt: skip
    return decibel_and_normalised(filterbank64(n_fft, n_mels).T @ spec.abs() ** 2)


def gemm_form32(x, geometry):
    """The kernel's formulation in fp32 on the CPU: the yardstick of what fp32 can give on this input."""
    n_fft, win, hop, n_mels = geometry
    left = (n_fft - win) // 2
    padded = torch.nn.functional.pad(x[None, None], (n_fft // 2, n_fft // 2), mode="reflect")[0, 0]
    frames = 1 + x.numel() // hop
    idx = (torch.arange(frames) * hop + left)[:, None] + torch.arange(win)[None, :]
    F = padded[idx]  # [T, win] fp32
    n = torch.arange(win, dtype=torch.float64)
    k = torch.arange(n_fft // 2 + 1, dtype=torch.float64)
    w = torch.hann_window(win, periodic=True, dtype=torch.float64)
    ang = 2 * torch.pi * (left + n)[:, None] * k[None, :] / n_fft
    C, S = (w[:, None] * torch.cos(ang)).float(), (w[:, None] * torch.sin(ang)).float()
    power = (F @ C) ** 2 + (F @ S) ** 2
    return decibel_and_normalised((power @ filterbank64(n_fft, n_mels).float()).T)


@functools.lru_cache(maxsize=None)
def reference(name):
    """Computed once per case and shared: the signals, the float64 oracle per row, and the fp32 yardstick's own error against it."""
    geometry, lengths = CASES[name]
    rows = [signal(L, seed=100 + i) for i, L in enumerate(lengths)]
    want = [oracle64(x, geometry) for x in rows]
    yard = [gemm_form32(x, geometry) for x in rows]
    err_raw = max(float((y[0].double() - w[0]).abs().max()) for y, w in zip(yard, want))
    err_norm = max(float((y[1].double() - w[1]).abs().max()) for y, w in zip(yard, want))
    return geometry, lengths, rows, want, err_raw, err_norm


def batch_of(rows):
    wave = torch.zeros(len(rows), max(x.numel() for x in rows))
    for i, x in enumerate(rows):
        wave[i, : x.numel()] = x
    return wave.to(DEV)


def run(rows, lengths, geometry, normalize):
    n_fft, win, hop, n_mels = geometry
    feats, lens = ops.log_mel_spectrogram(batch_of(rows), list(lengths), SR, n_fft, win, hop, n_mels, normalize=normalize)
    torch.cuda.synchronize()
    return feats.cpu(), lens.cpu()


@pytest.mark.parametrize("name", list(CASES))
def test_matches_the_float64_oracle(name):
    geometry, lengths, rows, want, err_raw, err_norm = reference(name)
    hop, n_mels = geometry[2], geometry[3]
    assert 0.0 < err_raw < 2e-3 and err_norm < 1e-3, (err_raw, err_norm)  # the yardstick itself is sane (measured: 3.4e-4, 1.0e-4)
    for normalize, which, bound in ((False, 0, 4 * err_raw), (True, 1, 4 * err_norm)):
        feats, lens = run(rows, lengths, geometry, normalize)
        assert tuple(feats.shape) == (len(rows), n_mels, 1 + max(lengths) // hop)
        assert lens.dtype == torch.int32 and lens.tolist() == [1 + L // hop for L in lengths]
        worst = 0.0
        for b, L in enumerate(lengths):
            Tb = 1 + L // hop
            assert tuple(want[b][which].shape) == (n_mels, Tb)
            worst = max(worst, float((feats[b, :, :Tb].double() - want[b][which]).abs().max()))
            assert bool((feats[b, :, Tb:] == 0.0).all()), "columns beyond T_b must be exactly 0"
        print(f"{name} normalize={normalize}: kernel max abs error {worst:.3e}, fp32 GEMM-form yardstick {bound / 4:.3e}, bound {bound:.3e}")
        assert torch.isfinite(feats).all()
        assert worst <= bound, (worst, bound)


def test_an_empty_filter_row_normalises_to_exactly_zero():
    geometry, lengths, rows, want, _, _ = reference("empty-filter-128-128-64-40")
    assert float(filterbank64(geometry[0], geometry[3])[:, 0].abs().max()) == 0.0
    raw, _ = run(rows, lengths, geometry, False)
    norm, _ = run(rows, lengths, geometry, True)
    for b, L in enumerate(lengths):
        Tb = 1 + L // geometry[2]
        assert bool((raw[b, 0, :Tb] == -100.0).all())
        assert bool((norm[b, 0, :Tb] == 0.0).all())  # not NaN, not a rounded mean over 1e-10
        assert float(want[b][1][0].abs().max()) == 0.0  # as in torch


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("normalize", [False, True])
def test_a_row_alone_equals_the_row_in_the_ragged_batch(name, normalize):
    """Bit for bit: nothing leaks across the padding, and reflection is about the row's own end, not the batch's."""
    geometry, lengths, rows, _, _, _ = reference(name)
    feats, _ = run(rows, lengths, geometry, normalize)
    for b, L in enumerate(lengths):
        alone, lens = run(rows[b : b + 1], lengths[b : b + 1], geometry, normalize)
        assert lens.tolist() == [1 + L // geometry[2]]
        assert torch.equal(alone[0], feats[b, :, : alone.shape[2]])


def test_digital_silence():
    """One utterance of pure zeros: -100 dB everywhere raw, exactly 0 after normalisation."""
    for geometry in (CASES["probe-512-128-64-80"][0], CASES["torchaudio-400-400-200-80"][0]):
        rows, lengths = [torch.zeros(1000), signal(600, seed=7)], (1000, 600)
        raw, _ = run(rows, lengths, geometry, False)
        norm, _ = run(rows, lengths, geometry, True)
        assert bool((raw[0] == -100.0).all()) and bool((norm[0] == 0.0).all())
        assert torch.isfinite(norm[1]).all() and float(norm[1].abs().max()) > 0.1


def raw_call(wave, lens_dev, geometry, normalize, fill):
    """blvm_logmel into caller-owned buffers that hold `fill` beforehand."""
    n_fft, win, hop, n_mels = geometry
    basis, fbank = ops._logmel_operands(wave.device, SR, n_fft, win, n_mels)
    out = torch.full((wave.shape[0], n_mels, 1 + wave.shape[1] // hop), fill, device=DEV, dtype=torch.float32)
    out_lens = torch.full((wave.shape[0],), -7, device=DEV, dtype=torch.int32)
    _hip.check(
        _hip.load().blvm_logmel(_hip.ptr(wave), _hip.ptr(lens_dev), wave.shape[0], wave.shape[1], n_fft, win, hop, n_mels, _hip.ptr(basis),
                                _hip.ptr(fbank), int(normalize), _hip.ptr(out), _hip.ptr(out_lens), _hip.stream_ptr()),
        "blvm_logmel",
    )  # fmt: skip
    torch.cuda.synchronize()
    return out.cpu(), out_lens.cpu()


@pytest.mark.parametrize("name", ["probe-512-128-64-80", "torchaudio-400-400-200-80"])
@pytest.mark.parametrize("normalize", [False, True])
def test_results_do_not_depend_on_the_buffers_or_the_call(name, normalize):
    """The caller-owned-buffer contract (a buffer of NaN and one of 1e30 give the same bits) and call-to-call determinism."""
    geometry, lengths, rows, _, _, _ = reference(name)
    wave = batch_of(rows)
    lens_dev = torch.tensor(lengths, dtype=torch.int32).to(DEV)
    a, a_lens = raw_call(wave, lens_dev, geometry, normalize, float("nan"))
    b, b_lens = raw_call(wave, lens_dev, geometry, normalize, 1e30)
    assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(a_lens, b_lens)
    assert a_lens.tolist() == [1 + L // geometry[2] for L in lengths]
    c, _ = run(rows, lengths, geometry, normalize)  # through the op: host lengths, its own buffers
    d, _ = run(rows, lengths, geometry, normalize)
    assert torch.equal(c, d) and torch.equal(a, c)


def test_device_lengths_out_of_range_mark_the_row():
    """An int32 device tensor of lengths is not read back; a row whose length the front end cannot take comes out NaN with length 0
    and does not disturb its neighbours."""
    geometry, lengths, rows, _, _, _ = reference("probe-512-128-64-80")
    wave = batch_of(rows)
    good, _ = raw_call(wave, torch.tensor(lengths, dtype=torch.int32).to(DEV), geometry, True, 0.0)
    for bad in (256, 0, -5, 1001):
        out, out_lens = raw_call(wave, torch.tensor([lengths[0], bad, lengths[2]], dtype=torch.int32).to(DEV), geometry, True, 0.0)
        assert out_lens.tolist() == [1 + lengths[0] // 64, 0, 1 + lengths[2] // 64]
        assert bool(torch.isnan(out[1]).all()) and torch.equal(out[0], good[0]) and torch.equal(out[2], good[2])


def test_transform_forms():
    geometry, lengths, rows, _, _, _ = reference("probe-512-128-64-80")
    t = LogMelSpectrogram(SR, *geometry)
    feats, lens = t(batch_of(rows), torch.tensor(lengths))
    one = t(rows[1].to(DEV))  # [time] -> [n_mels, T]
    assert tuple(one.shape) == (80, 1 + 777 // 64) and torch.equal(one, feats[1, :, : one.shape[1]])
    full = t(batch_of([rows[0], rows[0]]))  # [B, time] of full-length rows -> [B, n_mels, T]
    assert tuple(full.shape) == (2, 80, 16) and torch.equal(full[0], feats[0]) and torch.equal(full[1], feats[0])
    with pytest.raises(_hip.BlvmHipError, match="256 samples"):
        t(batch_of(rows), torch.tensor([1000, 777, 256]))


def test_probe_model_on_front_end_features():
    geometry, lengths, rows, _, _, _ = reference("probe-512-128-64-80")
    feats, feat_lens = LogMelSpectrogram(SR, 512, 128, 64, 80)(batch_of(rows), torch.tensor(lengths))
    torch.manual_seed(0)
    model = SimpleLSTMASR(TokenMap([f"p{i}" for i in range(5)], add_blank=True), input_size=80, hidden_size=32).to(DEV)
    y, y_sl = torch.tensor([[1, 2, 3], [4, 5, 0], [2, 0, 0]]), torch.tensor([3, 2, 1])
    loss, _, out = model(feats, feat_lens.cpu().long(), y.to(DEV), y_sl)
    assert torch.isfinite(loss)
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    assert out.sl.tolist() == feat_lens.tolist() == [1 + L // 64 for L in lengths]
