"""Train-step time of every model in the three operand modes (f32, bf16, f16), alternated in one process on one GPU, at bench.py's
default shapes (WaveNet also at [4, 1, 16000], its BASELINE shape).  Times come from bench.measure (the same step, optimizer and
clipping bench.py times); one JSON line per model and mode.  Then the GradScaler's own kernels on the VRNN's gradients
(unscale_ with its inf check, step, update) are timed with HIP events and reported against the VRNN f16 step.

usage: python tools/amp_bench.py [--steps 10] [--warmup 3] [--rounds 2] [--models vrnn,srnn,...]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "benchmarking-lvms_amd"))

import torch  # noqa: E402

import bench  # noqa: E402

SHAPES = {"vrnn": [(64, 16000)], "srnn": [(64, 16000)], "lstm": [(64, 16000)], "stcn": [(64, 16000)], "wavenet": [(4, 16000), (64, 16000)],
          "cwvae": [(8, 49152)]}  # fmt: skip
MODES = ("f32", "bf16", "f16")


def scaler_cost(dev, steps=20):
    """HIP-event time of unscale_ + step + update of a GradScaler over the VRNN's parameters with finite gradients (the optimizer's
    own update excluded: timed separately and subtracted)."""
    model = bench.build_model("vrnn", dev)
    params = list(model.parameters())
    for p in params:
        p.grad = torch.randn_like(p) * 1e-3
    opt = torch.optim.Adam(params, lr=3e-4, fused=True)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0**16, growth_interval=2000)
    scaler.scale(torch.ones((), device=dev))  # (creates the scale tensor, as the step's scaler.scale(loss) does)
    nbytes = sum(p.numel() for p in params) * 4

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / steps

    def with_scaler():
        scaler.unscale_(opt)
        scaler.step(opt)
        scaler.update()

    t_opt = timed(opt.step)
    t_scaled = timed(with_scaler)
    return dict(grad_mbytes=nbytes / 1e6, ms_opt=t_opt, ms_opt_with_scaler=t_scaled, ms_scaler=t_scaled - t_opt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2, help="f32 / bf16 / f16 alternations per model and shape")
    ap.add_argument("--models", default=",".join(SHAPES))
    args = ap.parse_args()
    from blvm import _hip
    from blvm.training.ddp import FlatGradAllReduce

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    vrnn_f16 = None
    for name in args.models.split(","):
        for B, T in SHAPES[name]:
            model = bench.build_model(name, dev)
            init = [p.detach().clone() for p in model.parameters()]
            best = {}
            for r in range(args.rounds):
                for mode in MODES:
                    with torch.no_grad():
                        for p, v in zip(model.parameters(), init):
                            p.copy_(v)
                    _hip.set_operand_dtype(mode)
                    res = bench.measure(name, model, B, T, args.steps, args.warmup, 0, dev, False, FlatGradAllReduce)
                    if res["async_errors"]:
                        raise SystemExit(f"{name} {mode}: persistent launch aborted; no number")
                    best.setdefault(mode, []).append(res["ms_median"])
            _hip.set_operand_dtype("f32")
            for mode in MODES:
                ms = sorted(best[mode])
                line = dict(model=name, shape=[B, T], dtype=mode, ms_median=ms[len(ms) // 2], ms_runs=ms,
                            vs_bf16=ms[len(ms) // 2] / sorted(best["bf16"])[len(best["bf16"]) // 2] - 1)
                print(json.dumps(line), flush=True)
                if name == "vrnn" and mode == "f16":
                    vrnn_f16 = line["ms_median"]
            del model
            torch.cuda.empty_cache()
    sc = scaler_cost(dev)
    if vrnn_f16:
        sc["share_of_vrnn_f16_step"] = sc["ms_scaler"] / vrnn_f16
    print(json.dumps(dict(model="vrnn", what="GradScaler unscale_+step+update minus Adam step", **sc)), flush=True)


if __name__ == "__main__":
    main()
