#!/usr/bin/env python
"""`ops.log_mel_spectrogram` (K10, csrc/logmel.hip) against the same computation in stock torch operators on the same device: per
utterance `torch.stft` on its own samples + filterbank matmul + log10 + mean / std, at one probe batch of about 120 s of audio (32 rows
of up to 60 000 samples, ragged).  If this torch build has no `torch.stft` on the device, the stock path is the unfused GEMM form
(frames gathered by index, two matmuls) and the output says so.  A second stock variant runs ONE batched `torch.stft` over the padded
batch (cheaper, but it reflects about the padded end and normalises over the padding: not the same result for ragged rows; timed to
show what batching alone buys).  One process; every path is warmed up, then timed alternately in rounds of `--calls` calls between two
device events; medians and min..max of the rounds are printed, and the fused result is compared with the stock one first."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "benchmarking-lvms_amd"))
from blvm import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--L", type=int, default=60000)
    ap.add_argument("--sample_rate", type=int, default=16000)
    ap.add_argument("--n_fft", type=int, default=512)
    ap.add_argument("--win_length", type=int, default=128)
    ap.add_argument("--hop_length", type=int, default=64)
    ap.add_argument("--n_mels", type=int, default=80)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "logmel_bench needs a HIP device"
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    lengths = sorted((int(v) for v in torch.randint(a.L * 3 // 4, a.L + 1, (a.B,), generator=gen)), reverse=True)
    lengths[0] = a.L
    t = torch.arange(a.L, dtype=torch.float64) / a.sample_rate
    wave = torch.zeros(a.B, a.L)
    for b, n in enumerate(lengths):
        tone = 0.3 * torch.sin(2 * torch.pi * (200.0 + 37.0 * b) * t[:n]) + 0.1 * torch.sin(2 * torch.pi * 3100.0 * t[:n])
        wave[b, :n] = (tone + 1e-2 * torch.randn(n, dtype=torch.float64, generator=gen)).float()
    wave = wave.to(dev)
    lens_dev = torch.tensor(lengths, dtype=torch.int32).to(dev)
    fb = ops.logmel_filterbank(a.sample_rate, a.n_fft, a.n_mels).float().to(dev)  # [n_bins, n_mels]
    window = torch.hann_window(a.win_length, periodic=True, device=dev)
    left = (a.n_fft - a.win_length) // 2
    basis = ops.logmel_basis(a.n_fft, a.win_length).float().to(dev)
    taps = torch.arange(a.win_length, device=dev)

    def power_stft(x):  # [..., L] -> [..., n_bins, T]
        return torch.stft(x, a.n_fft, hop_length=a.hop_length, win_length=a.win_length, window=window, center=True, pad_mode="reflect",
                          return_complex=True).abs() ** 2  # fmt: skip

    def power_gather(x):  # the unfused GEMM form of one utterance
        padded = torch.nn.functional.pad(x[None, None], (a.n_fft // 2, a.n_fft // 2), mode="reflect")[0, 0]
        idx = (torch.arange(1 + x.numel() // a.hop_length, device=dev) * a.hop_length + left)[:, None] + taps[None, :]
        F = padded[idx]
        return ((F @ basis[:, 0]) ** 2 + (F @ basis[:, 1]) ** 2).T

    try:
        power_stft(wave[0, : lengths[0]])
        torch.cuda.synchronize()
        power, stock_form = power_stft, "torch.stft"
    except Exception as e:  # noqa: BLE001  (reported in the output, not hidden)
        power, stock_form = power_gather, f"gather + matmul (torch.stft unavailable: {type(e).__name__}: {e})"

    def finish(p):  # [..., n_bins, T] power -> normalised log-mel [..., n_mels, T]
        db = 10.0 * torch.log10(torch.clamp_min(fb.T @ p, 1e-10))
        return (db - db.mean(-1, keepdim=True)) / (db.std(-1, keepdim=True) + 1e-10)

    def fused():
        return ops.log_mel_spectrogram(wave, lens_dev, a.sample_rate, a.n_fft, a.win_length, a.hop_length, a.n_mels)[0]

    def stock():
        out = torch.zeros(a.B, a.n_mels, 1 + a.L // a.hop_length, device=dev)
        for b, n in enumerate(lengths):
            f = finish(power(wave[b, :n]))
            out[b, :, : f.shape[1]] = f
        return out

    paths = dict(fused=fused, stock=stock)
    if power is power_stft:
        paths["stock_batched_padded"] = lambda: finish(power_stft(wave))
    got, want = fused(), stock()
    torch.cuda.synchronize()
    diff = float((got - want).abs().max())

    for f in paths.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(a.rounds):
        for name, f in paths.items():  # alternated: a drift of the box hits every path alike
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.calls * 1e3)
    frames = sum(1 + n // a.hop_length for n in lengths)
    out = dict(shape=dict(B=a.B, L=a.L, seconds_of_audio=round(sum(lengths) / a.sample_rate, 1), frames=frames, n_fft=a.n_fft,
                          win_length=a.win_length, hop_length=a.hop_length, n_mels=a.n_mels),
               rounds=a.rounds, calls_per_round=a.calls, stock_form=stock_form, max_abs_diff_fused_vs_stock=diff)  # fmt: skip
    for name, ts in times.items():
        out[name + "_us"] = dict(median=round(statistics.median(ts), 1), min=round(min(ts), 1), max=round(max(ts), 1))
    out["stock_over_fused"] = round(out["stock_us"]["median"] / out["fused_us"]["median"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
