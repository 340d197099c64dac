"""ms per model step of `STCN.generate` at the default widths (res_channels 256, latents 256/128/64/32/16, 5 layers x 5 stacks, S = 64
samples per step): the one-launch kernel (`blvm_stcn_generate`) and the step-by-step path at the same shape, and the weight
ingest per workgroup the one-launch figure stands for (the matrices a step streams: a block's skip half only where a level or the
output sum reads it, no residual half in a stack's last block).  Every figure: warm-up call, then `--reps` timed calls (device events
around the whole call: weight packing and the launch); median and min..max of the calls, per step.  `--slow-reps 0` leaves the
step-by-step path out.  `--resume` adds the calls from a state: a resumed one-launch call of the same length (each call continues the
state the call before it returned), and the one-off cost of a prompt of receptive_field stacks — the latent pass over the prompt
(`STCN._prime`) and the priming of the kernel's rings from the state's windows (`STCN._prime_rings`), in ms per call.
python tools/probe_stcn_generate.py [--samples 16000] [--batch 16] [--reps 5] [--slow-reps 1] [--resume]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "benchmarking-lvms_amd"))
from blvm import _hip  # noqa: E402
from blvm.models.stcn.stcn import STCN  # noqa: E402


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


def streamed_floats(m):
    """Matrix elements one step of the one-launch kernel reads."""
    C, S = m.res_channels, m.n_stack_frames
    groups = m._skip_groups()
    n = 2 * S * C + C * C  # causal conv, in_transform
    for i, g in enumerate(groups):
        n += 4 * C * C + (C * C if i + 1 < len(groups) else 0) + (C * C if g >= 0 else 0)
    for p in m.prior:
        n += 2 * sum(l.weight.numel() for l in (p.transform_mu[0], p.transform_mu[2], p.transform_mu[4]))
    ot = m.out_transform
    n += ot.in_transform.weight.numel() + len(ot.res_blocks) * 6 * C * C - C * C
    return n + m.out_upsample[0].weight.numel() + 32 * 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=16000)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slow-reps", type=int, default=1)
    ap.add_argument("--resume", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(0)
    m = STCN(likelihood="DMoL", n_stack_frames=64).cuda()
    steps = (a.samples + 63) // 64
    mb = 4 * streamed_floats(m) / 1e6
    med, lo, hi = per_step_ms(lambda: m.generate(n_samples=a.batch, max_timesteps=a.samples, fused=True), steps, a.reps)
    print(f"one launch, B={a.batch}, {steps} steps: {med:.4f} ms per step (median of {a.reps}; {lo:.4f} .. {hi:.4f}); {mb:.1f} MB of weights per "
          f"step -> {mb / med:.1f} GB/s per workgroup", flush=True)  # fmt: skip
    if a.resume:
        S, rf = m.n_stack_frames, m.receptive_field
        box = [m.generate(n_samples=a.batch, max_timesteps=rf * S, fused=True, return_state=True)[1].state]

        def resumed():
            box[0] = m.generate(n_samples=a.batch, max_timesteps=steps * S, fused=True, state=box[0], return_state=True)[1].state

        med, lo, hi = per_step_ms(resumed, steps, a.reps)
        print(f"one launch from a state, B={a.batch}, {steps} steps: {med:.4f} ms per step (median of {a.reps}; {lo:.4f} .. {hi:.4f})", flush=True)
        prompt = 0.8 * torch.tanh(torch.randn(a.batch, rf * S, device="cuda"))
        num_mix = m.likelihood_module.num_mix
        for mode in ("posterior", "prior"):
            med, lo, hi = per_step_ms(lambda: m._prime_rings(m._prime(prompt, None, mode)[0], num_mix), 1, a.reps)
            print(f"priming from a prompt of {rf} stacks ({mode} latents), B={a.batch}: {med:.3f} ms (median of {a.reps}; {lo:.3f} .. {hi:.3f})",
                  flush=True)  # fmt: skip
    if a.slow_reps > 0:
        med, lo, hi = per_step_ms(lambda: m.generate(n_samples=a.batch, max_timesteps=a.samples, fused=False), steps, a.slow_reps)
        print(f"step by step, B={a.batch}, {steps} steps: {med:.4f} ms per step (median of {a.slow_reps}; {lo:.4f} .. {hi:.4f})", flush=True)


if __name__ == "__main__":
    main()
