"""Two timings for the Gaussian heads of WaveNet (DESIGN K7b / K10c), on the GPU:

  generate   `WaveNet.generate(cached=True)` in one launch (K10c) at res_channels = 64, 4 stacks x 10 layers (40 blocks), B = 16,
             16000 frames: the GMM-10 head against the DMoL head of the same network.  One warm-up call per head, then ROUNDS calls per
             head, the heads alternating; host clock around the call and a synchronise (the call draws its noise on the device, two
             or three launches in front of the kernel).
  k7b        the K7b forward + backward (`ops.gmm_log_prob`, W = NULL, time-major, S = 1: WaveNet's call) on [16, 16000] frames at
             n = 3 (the general arm) against n = 10 (the arm of the audio models), device events around REPS forward + backward pairs,
             ROUNDS windows per count, alternating; ns per frame.

Prints median and min .. max per row and writes them as JSON (--out).  TEST / MEASUREMENT INFRASTRUCTURE: not imported by the product.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "benchmarking-lvms_amd"))

from blvm import ops  # noqa: E402
from blvm.models import WaveNet  # noqa: E402
from blvm.modules.distributions import DiagonalGaussianMixtureDense, DiscretizedLogisticMixtureDense  # noqa: E402

DEV = "cuda:0"


def row(name, vals, unit):
    r = dict(name=name, unit=unit, median=statistics.median(vals), min=min(vals), max=max(vals), runs=vals)
    print(f"{name}: median {r['median']:.5g} {unit} (min {r['min']:.5g}, max {r['max']:.5g}, {len(vals)} runs)", flush=True)
    return r


def bench_generate(B, n_frames, rounds):
    C = 64
    models = {}
    for name in ("dmol", "gmm10"):
        torch.manual_seed(0)
        lik = DiscretizedLogisticMixtureDense(C, 1, num_mix=10, num_bins=2**16) if name == "dmol" else DiagonalGaussianMixtureDense(C, 1, num_mix=10, initial_sd=1, epsilon=1e-4)
        m = WaveNet(likelihood=lik, n_layers=10, n_stacks=4, res_channels=C).to(DEV).eval()
        assert m._decode_kernel_applies() if name == "dmol" else m._gauss_decode_kernel_applies()
        models[name] = m
    times = {k: [] for k in models}
    for r in range(rounds + 1):  # round 0: the warm-up
        for name, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x = m.generate(n_samples=B, n_frames=n_frames, cached=True)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert bool(torch.isfinite(x).all())
            if r:
                times[name].append(1e3 * dt / n_frames)
    return [row(f"generate {k} B={B} frames={n_frames}", v, "ms/frame") for k, v in times.items()]


def bench_k7b(B, T, rounds, reps):
    cases = {}
    for n in (3, 10):
        g = torch.Generator(device=DEV).manual_seed(n)
        par = torch.randn(T * B, 3 * n, device=DEV, generator=g).requires_grad_(True)
        y = torch.rand(B, T, device=DEV, generator=g) * 2 - 1
        cases[n] = (par, y, torch.full((B,), T, device=DEV, dtype=torch.int32))

    def pair(n):
        par, y, sl = cases[n]
        par.grad = None
        ops.gmm_log_prob(par, None, None, y, sl, ops.LAYOUT_TIME_MAJOR, B, T, T, 1, n, 0.6931, 1e-4).sum().backward()

    times = {n: [] for n in cases}
    for r in range(rounds + 1):
        for n in cases:
            pair(n)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                pair(n)
            b.record()
            torch.cuda.synchronize()
            if r:
                times[n].append(1e6 * a.elapsed_time(b) / reps / (B * T))
    return [row(f"k7b fwd+bwd n={n} frames={B * T}", v, "ns/frame") for n, v in times.items()]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16000)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    rows = bench_k7b(a.batch, 16000, a.rounds, a.reps) + bench_generate(a.batch, a.frames, a.rounds)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
