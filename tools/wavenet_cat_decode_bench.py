"""Cached WaveNet generation with the categorical head: milliseconds per generated sample of the one-launch path
(`blvm_wavenet_cat_decode`), of the block-by-block path (`WaveNet._generate_cached`) and of the DMoL one-launch kernel as the
yardstick, on the benchmark's WaveNet (5 x 10 blocks, 96 channels) with an 8-bit softmax, at B = 1, 16 and 64.

Device events around whole calls; 5 windows in which the paths alternate; median and range over the windows.  With
`--parent-tree PATH` (a built checkout of the parent commit: its `benchmarking-lvms_amd` and `include`) the block-by-block path and
the DMoL kernel are measured once more on that tree's package and library, in a fresh process, which is the "before" of the table in
DESIGN K10c.

python tools/wavenet_cat_decode_bench.py [--parent-tree PATH] [--out profiles/wavenet_cat_decode_bench.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

BATCHES = (1, 16, 64)
CHANNELS = 96  # --channels 64: the register-resident path <8,64,64> of the kernel instead of the any-width one
WINDOWS = 5
FRAMES = {"cat_one_launch": 400, "dmol_one_launch": 400, "cat_block_by_block": 12}  # per window; the slow path gets fewer frames


def build(head):
    from blvm.models import WaveNet
    from blvm.modules.distributions import CategoricalDense, DiscretizedLogisticMixtureDense

    torch.manual_seed(0)
    C = CHANNELS
    lik = CategoricalDense(C, 256) if head == "cat" else DiscretizedLogisticMixtureDense(C, 1, num_mix=10, num_bins=2**16)
    return WaveNet(likelihood=lik, n_layers=10, n_stacks=5, res_channels=C).cuda()


def paths(which):
    """{name: (B, n) -> None} of the paths asked for."""
    out = {}
    if "cat_one_launch" in which or "cat_block_by_block" in which:
        cat = build("cat")
    if "cat_one_launch" in which:
        assert cat._cat_decode_kernel_applies()
        out["cat_one_launch"] = lambda B, n: cat.generate(B, n, cached=True)
    if "dmol_one_launch" in which:
        dmol = build("dmol")
        assert dmol._decode_kernel_applies()
        out["dmol_one_launch"] = lambda B, n: dmol.generate(B, n, cached=True)
    if "cat_block_by_block" in which:
        out["cat_block_by_block"] = lambda B, n: cat._generate_cached(B, n)
    return out


def measure(which):
    """-> {path: {B: [ms per sample of each window]}}; within a window the paths run one after the other."""
    fns = paths(which)
    res = {name: {B: [] for B in BATCHES} for name in fns}
    for B in BATCHES:
        for name, fn in fns.items():  # warm-up: allocator, code objects, weights into the caches
            fn(B, max(FRAMES[name] // 4, 2))
        torch.cuda.synchronize()
        for _ in range(WINDOWS):
            for name, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(B, FRAMES[name])
                e1.record()
                torch.cuda.synchronize()
                res[name][B].append(e0.elapsed_time(e1) / FRAMES[name])
    return res


def summary(windows):
    return {"median_ms": statistics.median(windows), "min_ms": min(windows), "max_ms": max(windows), "windows_ms": windows}


def main():
    global CHANNELS
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: block by block and DMoL measured on it too")
    ap.add_argument("--tree", default=ROOT, help="(internal) the tree whose package is imported")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wavenet_cat_decode_bench.json"))
    ap.add_argument("--only", default=None, help="(internal) comma-separated paths; prints their windows as one JSON line")
    ap.add_argument("--channels", type=int, default=CHANNELS, help="residual / skip channels (default: the benchmark's 96)")
    a = ap.parse_args()
    CHANNELS = a.channels
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "benchmarking-lvms_amd"))
    if a.only:
        print("RESULT " + json.dumps(measure(a.only.split(","))))
        return
    res = {name: {str(B): summary(w) for B, w in per.items()} for name, per in measure(list(FRAMES)).items()}
    if a.parent_tree:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "cat_block_by_block,dmol_one_launch", "--tree", a.parent_tree,
                              "--channels", str(CHANNELS)],
                             check=True, capture_output=True, text=True, timeout=900).stdout  # fmt: skip
        line = [l for l in out.splitlines() if l.startswith("RESULT ")][-1]
        for name, per in json.loads(line[len("RESULT "):]).items():
            res["parent_" + name] = {str(B): summary(w) for B, w in per.items()}
    doc = {"model": f"WaveNet 5 x 10 blocks, {CHANNELS} channels; heads: CategoricalDense({CHANNELS}, 256), DMoL(num_mix=10)", "device": torch.cuda.get_device_name(0),
           "method": f"device events around whole generate calls, {WINDOWS} alternating windows, frames per window {FRAMES}", "unit": "ms per sample",
           "parent_measured": bool(a.parent_tree), "paths": res}  # fmt: skip
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("| path | " + " | ".join(f"B = {B}" for B in BATCHES) + " |")
    print("|---|" + "---|" * len(BATCHES))
    for name, per in res.items():
        print(f"| {name} | " + " | ".join(f"{per[str(B)]['median_ms']:.4f} ({per[str(B)]['min_ms']:.4f} .. {per[str(B)]['max_ms']:.4f})" for B in BATCHES) + " |")


if __name__ == "__main__":
    main()
