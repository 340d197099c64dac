#!/usr/bin/env python
"""One training step of the CTC probe at its own shape (T = 750, B = 40, 80 features, hidden 128, one layer, 62 classes, 32-40 labels):
`SimpleLSTMASR` forward + backward + `tracker.update(metrics)`, as synchronised wall time per step.  The step is what the error rates
cost the training loop: on the host path the greedy decode's copy, the string building and the Python Levenshtein sit inside
forward; on the device path (`ops.ctc_error_totals`) nothing leaves the device until the tracker is read, which is timed apart.

One process times ONE source tree (`--package`: the directory that holds `blvm/`), so that two commits can be compared by running
the tool alternately on each (A B A B: a drift of the box hits both alike) with the same library.  Warm-up steps first, then
`--rounds` rounds of `--steps` steps, every step between two device synchronisations; the median and min..max over all steps are
printed as one JSON line, with the hypothesis lengths the step met (the host path's cost grows with them).  Where the tree has
`ops.ctc_error_totals`, that call alone, and the distance launch inside it, are also timed between device events, in rounds of
`--calls` calls.

`--num_layers` and `--bidirectional True|False` build the deeper probes of the reference's `experiments/phoneme.txt`
(`--hidden_size 256 --num_layers 3 --bidirectional True`); their defaults are the one-layer unidirectional step above."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def spread(ts, digits=3):
    return dict(median=round(statistics.median(ts), digits), min=round(min(ts), digits), max=round(max(ts), digits))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package", default=os.path.join(HERE, "..", "benchmarking-lvms_amd"))
    ap.add_argument("--T", type=int, default=750)
    ap.add_argument("--B", type=int, default=40)
    ap.add_argument("--input_size", type=int, default=80)
    ap.add_argument("--hidden_size", type=int, default=128)
    ap.add_argument("--num_layers", type=int, default=1)
    ap.add_argument("--bidirectional", type=lambda v: v.lower() in ("1", "true", "yes"), default=False, metavar="True|False")
    ap.add_argument("--classes", type=int, default=62)
    ap.add_argument("--L", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package))
    from blvm import ops
    from blvm.data.token_map import TokenMap
    from blvm.evaluation.tracker import Tracker
    from blvm.models import SimpleLSTMASR

    assert torch.cuda.is_available(), "asr_step_bench needs a HIP device"
    dev = "cuda:0"
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(0)
    tm = TokenMap([chr(97 + i % 26) + chr(97 + i // 26) for i in range(a.classes - 1)], add_blank=True)  # two-letter "phonemes"
    model = SimpleLSTMASR(tm, a.input_size, a.hidden_size, num_layers=a.num_layers, bidirectional=a.bidirectional).to(dev).train()
    # lr = 0: the optimiser does its work and the weights stay, so that every timed step meets the same transcripts (a few real
    # steps on one batch collapse the untrained model to blanks, and an empty hypothesis costs the host path nothing)
    opt = torch.optim.Adam(model.parameters(), lr=0.0)
    x_sl = torch.randint(max(a.T - 100, 2 * a.L + 1), a.T + 1, (a.B,), generator=gen).sort(descending=True).values
    y_sl = torch.randint(max(a.L - 8, 1), a.L + 1, (a.B,), generator=gen)
    y = torch.randint(1, a.classes, (a.B, a.L), generator=gen)
    # every label holds its own feature vector for an equal share of the row's frames, plus a little noise: the greedy transcripts
    # then have about as many tokens as the targets (white noise would give hundreds, a constant input none)
    proto = torch.randn(a.classes, a.input_size, generator=gen)
    seg = (torch.arange(a.T)[None, :] * y_sl[:, None] // x_sl[:, None]).clamp(max=a.L - 1)  # [B,T] label position of frame t
    x = (proto[y.gather(1, seg)].permute(0, 2, 1) + 0.1 * torch.randn(a.B, a.input_size, a.T, generator=gen)).contiguous().to(dev)
    tracker = Tracker()

    def step():
        opt.zero_grad(set_to_none=True)
        loss, metrics, out = model(x, x_sl, y, y_sl)
        loss.backward()
        opt.step()
        tracker.update(metrics)
        return out

    for _ in range(a.warmup):
        out = step()
    hyp_tokens = [len(h.split(" ")) if h else 0 for h in out.hyps]
    torch.cuda.synchronize()
    times = []
    for _ in range(a.rounds):
        for _ in range(a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = step()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    values = tracker.values()
    read_ms = (time.perf_counter() - t0) * 1e3

    res = dict(package=os.path.relpath(os.path.abspath(a.package), os.path.join(HERE, "..")),
               shape=dict(T=a.T, B=a.B, input=a.input_size, hidden=a.hidden_size, layers=a.num_layers, bidirectional=a.bidirectional,
                          classes=a.classes, L=a.L), steps=len(times),
               step_ms=spread(times), tracker_read_ms=round(read_ms, 3), wer=round(values["wer"], 4), cer=round(values["cer"], 4),
               hyp_tokens=dict(mean=round(statistics.mean(hyp_tokens), 1), max=max(hyp_tokens)))  # fmt: skip
    if hasattr(ops, "ctc_error_totals"):
        logits = out.logits.detach().transpose(0, 1).contiguous()
        il, tl, yd = x_sl.to(dev).int(), y_sl.to(dev).int(), y.to(dev).int()
        tables = tm.unit_tables()
        for _ in range(5):
            ops.ctc_error_totals(logits, il, yd, tl, tables, blank=model.blank_index)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                ops.ctc_error_totals(logits, il, yd, tl, tables, blank=model.blank_index)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / a.calls * 1e3)
        res["error_counts_us"] = spread(ts, 1)  # the decode, the distances under both tables and the batch sums
        hyp, hyp_lens = ops.ctc_greedy_device(logits, il, blank=model.blank_index)
        ts = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                ops.edit_distance(yd, tl, hyp, hyp_lens, table=tables)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / a.calls * 1e3)
        res["edit_distance_us"] = spread(ts, 1)  # the distances alone: one launch for both tables
    print(json.dumps(res))


if __name__ == "__main__":
    main()
