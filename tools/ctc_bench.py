#!/usr/bin/env python
"""Forward + backward of `ops.ctc_loss` (K9, csrc/ctc.hip) against `logits.log_softmax(2)` + `torch.nn.functional.ctc_loss` on the same
device, at the probe's own shape (T = 750, B = 40, C = 62, L ~ 40).  One process; both paths are warmed up, then timed alternately in
rounds of `--calls` calls between two device events; the medians and the min..max of the rounds are printed, and the two paths'
results are compared first (faster and different is not faster).  Also times the loss-only call and the greedy decode."""
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
    ap.add_argument("--T", type=int, default=750)
    ap.add_argument("--B", type=int, default=40)
    ap.add_argument("--C", type=int, default=62)
    ap.add_argument("--L", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ctc_bench needs a HIP device"
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    logits = torch.randn(a.T, a.B, a.C, generator=gen).to(dev).requires_grad_(True)
    y_sl = torch.randint(max(a.L - 8, 1), a.L + 1, (a.B,), generator=gen)
    x_sl = torch.randint(max(a.T - 100, 2 * a.L + 1), a.T + 1, (a.B,), generator=gen)
    y = torch.randint(1, a.C, (a.B, a.L), generator=gen)
    y_dev, x_dev, yl_dev = y.to(dev).int(), x_sl.to(dev).int(), y_sl.to(dev).int()
    y_long = y.to(dev)
    n = float(y_sl.sum())

    def fused():
        logits.grad = None
        (ops.ctc_loss(logits, y_dev, x_dev, yl_dev, blank=0).sum() / n).backward()

    def stock():
        logits.grad = None
        nll = torch.nn.functional.ctc_loss(logits.log_softmax(2), y_long, x_sl, y_sl, blank=0, reduction="none", zero_infinity=False)
        (nll.sum() / n).backward()

    def loss_only():
        with torch.no_grad():
            ops.ctc_loss(logits, y_dev, x_dev, yl_dev, blank=0)

    def greedy():
        ops.ctc_greedy(logits, x_dev, blank=0)

    fused()
    g_fused = logits.grad.clone()
    stock()
    g_stock = logits.grad.clone()
    diff = float((g_fused - g_stock).norm() / g_stock.norm())

    paths = dict(fused=fused, stock=stock, loss_only=loss_only, greedy=greedy)
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
    out = dict(shape=dict(T=a.T, B=a.B, C=a.C, L=a.L), rounds=a.rounds, calls_per_round=a.calls, grad_rel_diff_fused_vs_stock=diff)
    for name, ts in times.items():
        out[name + "_us"] = dict(median=round(statistics.median(ts), 1), min=round(min(ts), 1), max=round(max(ts), 1))
    out["stock_over_fused"] = round(out["stock_us"]["median"] / out["fused_us"]["median"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
