#!/usr/bin/env python
"""What `model.represent(x, x_sl)` costs beside the only other way to the latents, `model(x, x_sl)[2].z` under `torch.no_grad()`, for
the four latent-variable models at their BASELINE configurations (bench.py's models and shapes: [64, 16000], CW-VAE [8, 49152]).

The two routes are alternated in one process after a warm-up; a sample is a host clock around `--calls` calls between two device
synchronisations, and `--rounds` samples are taken of each.  Per model one JSON line: median and min..max of both routes, their
ratio, `spread_ms` = the larger max - min of the two routes' own samples (what repeats of the SAME code differ by in this run) and
`within_spread` = represent's median is not above forward's by more than that.  Also `represent(level=1)` for CW-VAE and
`represent(level=top)` for STCN, `--num_samples K` > 1 (the K-particle mean beside K forward calls), and for VRNN the training
throughput of the resampling probe in latent frames/s: `LatentRepresentation` + one forward / backward / Adam step of
`SimpleLSTMASR(hidden 128)` through the step function of experiments/_asr.py.  DESIGN "K8r"."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "benchmarking-lvms_amd"))
sys.path.insert(0, os.path.join(ROOT, "experiments"))
DEV = "cuda:0"


def build(name):
    from blvm.models import STCN, CWVAEAudio, SRNNAudio, VRNNAudio

    torch.manual_seed(0)
    if name == "vrnn":
        return VRNNAudio(likelihood="DMoL", input_size=64, hidden_size=256, latent_size=256, residual_posterior=True), 64, 16000
    if name == "srnn":
        return SRNNAudio(likelihood="DMoL", input_size=64, hidden_size=256, latent_size=256, residual_posterior=True, smoothing=True), 64, 16000
    if name == "stcn":
        return STCN(likelihood="DMoL", n_layers=5, latent_size=[256, 128, 64, 32, 16], res_channels=256, n_stack_frames=64, dense=True), 64, 16000
    return CWVAEAudio(z_size=[128, 64, 32], h_size=192, strides=[64, 16, 16], num_level_layers=8, stride_per_layer=2,
                      precision_posterior=True, likelihood="DMoL", num_bins=2**16), 8, 49152  # fmt: skip


def stats(ts):
    return dict(median=round(statistics.median(ts), 3), min=round(min(ts), 3), max=round(max(ts), 3))


def alternate(fns, warmup, rounds, calls):
    """{name: [ms per call]} of the routes in `fns`, one sample of each per round in turn."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) * 1e3 / calls)
    return out


def probe_training(model, x, x_sl, a):
    """Latent frames/s of the resampling probe's training step on the frozen VRNN."""
    import _asr
    from blvm.data.token_map import TokenMap
    from blvm.data.transforms import LatentRepresentation
    from blvm.evaluation import Tracker
    from blvm.models import SimpleLSTMASR

    fe = LatentRepresentation(model, level=0, num_samples=1)
    tm = TokenMap([f"t{i:02d}" for i in range(61)], add_blank=True)
    B = x.shape[0]
    gen = torch.Generator().manual_seed(0)
    y, y_sl = torch.randint(1, 62, (B, 40), generator=gen), torch.randint(32, 41, (B,), generator=gen)
    probe = SimpleLSTMASR(tm, model.latent_size, 128).to(DEV).train()
    opt = torch.optim.Adam(probe.parameters(), lr=0.0)  # the optimiser works, the weights stay: every step meets the same transcripts
    tracker, frames = Tracker(), 0
    x_host = x.cpu()

    def step():
        nonlocal frames
        loss, metrics, _, z_sl = _asr.probe_step(probe, fe, x_host, x_sl, y, y_sl, DEV)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        tracker.update(metrics)
        frames = int(z_sl.sum())

    ts = alternate(dict(step=step), a.warmup, a.rounds, a.calls)["step"]
    return dict(step_ms=stats(ts), latent_frames_per_step=frames, frames_per_s=round(frames / statistics.median(ts) * 1e3, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="vrnn,srnn,stcn,cwvae")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--num_samples", type=int, default=4, help="K of the extra K-particle row (0: leave it out)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "probe_represent needs a HIP device"
    for name in a.models.split(","):
        model, B, T = build(name)
        model = model.to(DEV).eval()
        gen = torch.Generator().manual_seed(1)
        x = ((torch.rand(B, T, generator=gen) * 2 - 1) * 0.5).to(DEV)
        x_sl = (torch.rand(B, generator=gen) * 0.5 + 0.5).mul(T).long().sort(descending=True).values
        x_sl[0] = T  # ragged, longest first, the first row full
        levels = len(getattr(model, "latent_size", [0])) if name == "stcn" else (3 if name == "cwvae" else 1)

        def forward():
            with torch.no_grad():
                return model(x, x_sl)[2].z

        fns = dict(forward=forward, represent=lambda: model.represent(x, x_sl))
        if name == "cwvae":
            fns["represent_level1"] = lambda: model.represent(x, x_sl, level=1)
        if name == "stcn":
            fns["represent_top"] = lambda: model.represent(x, x_sl, level=levels - 1)
        if a.num_samples > 1:
            fns[f"forward_x{a.num_samples}"] = lambda: [forward() for _ in range(a.num_samples)]
            fns[f"represent_k{a.num_samples}"] = lambda: model.represent(x, x_sl, num_samples=a.num_samples)
        ts = alternate(fns, a.warmup, a.rounds, a.calls)
        fwd, rep = statistics.median(ts["forward"]), statistics.median(ts["represent"])
        spread = max(max(ts[k]) - min(ts[k]) for k in ("forward", "represent"))
        res = dict(model=name, shape=[B, T], rounds=a.rounds, calls=a.calls, ms={k: stats(v) for k, v in ts.items()},
                   forward_over_represent=round(fwd / rep, 3), spread_ms=round(spread, 3), within_spread=bool(rep - fwd <= spread))  # fmt: skip
        if name == "vrnn":
            res["probe_training"] = probe_training(model, x, x_sl, a)
        print(json.dumps(res), flush=True)
        del model, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
