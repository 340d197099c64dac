"""ms per generated 64-sample stack of the LSTMAudio roll-out (`blvm_lstm_generate`) at the BASELINE widths S = 64, H = 256:
one layer at B = 2, 16, 64, 128, two layers at B = 16, the step-by-step path at B = 16, and `blvm_srnn_generate` at the same B in
the same session.  Every figure: warm-up call, then `--reps` timed calls of `--steps` steps each (device events around the whole
call: weight packing, sentinel fill, launch and the copies of the final state); median and min..max of the calls, per step.
python tools/probe_lstm_decode.py [--steps 250] [--reps 7]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "benchmarking-lvms_amd"))
from blvm import _hip  # noqa: E402
from blvm.models import LSTMAudio, SRNNAudio  # noqa: E402


def per_step_ms(fn, steps, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / steps)
    _hip.check_async()
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=250)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    T = a.steps
    torch.manual_seed(0)
    lstm = {L: LSTMAudio(stack_size=64, hidden_size=256, num_layers=L).cuda() for L in (1, 2)}
    srnn = SRNNAudio(likelihood="DMoL", input_size=64, hidden_size=256, latent_size=256, residual_posterior=True, smoothing=True).cuda()

    def report(what, fn, steps=T):
        med, lo, hi = per_step_ms(fn, steps, a.reps)
        print(f"{what}: {med:.4f} ms per stack (median of {a.reps}; {lo:.4f} .. {hi:.4f})", flush=True)

    for B in (2, 16, 64, 128):
        report(f"LSTM one launch, 1 layer, B={B}", lambda: lstm[1].generate(n_samples=B, max_timesteps=T, fused=True))
        report(f"SRNN one launch, B={B}", lambda: srnn.srnn.generate(x=torch.zeros(B, 1, 64, device="cuda"), n_samples=B, max_timesteps=T, fused=True))
    report("LSTM one launch, 2 layers, B=16", lambda: lstm[2].generate(n_samples=16, max_timesteps=T, fused=True))
    n = max(T // 5, 1)  # the step-by-step path is host-bound: fewer steps time the same thing
    report("LSTM step by step, 1 layer, B=16", lambda: lstm[1].generate(n_samples=16, max_timesteps=n, fused=False), n)


if __name__ == "__main__":
    main()
