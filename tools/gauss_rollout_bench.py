"""VRNNAudio / SRNNAudio `generate()` at the benchmark widths (S = 64, H = 256, Z = 256, B = 16, T = 250) with the GMM head and with
the DMoL head: seconds per call on this tree and, with `--parent-tree PATH` (a built checkout of the parent commit: its
`benchmarking-lvms_amd` and `include`), on that tree's package and library.  On a tree without the one-launch GMM roll-out the GMM call
runs step by step, so the pair is the gain of the one-launch path; the DMoL pair shows what the new head arms cost the DMoL roll-out.

Host clock around a whole call that ends in a device synchronise; 2 warm-up calls, then REPS calls per model; each tree is measured in
fresh processes, ROUNDS times, the trees alternating; median and interquartile range over all calls of a tree.

python tools/gauss_rollout_bench.py [--parent-tree PATH] [--out profiles/gauss_rollout_bench.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
S, H, Z, B, T = 64, 256, 256, 16, 250
REPS, ROUNDS = 10, 2
MODELS = ("vrnn_gmm", "srnn_gmm", "vrnn_dmol", "srnn_dmol")


def measure():
    import torch

    from blvm.models import SRNNAudio, VRNNAudio

    res = {}
    for name in MODELS:
        torch.manual_seed(0)
        cls = VRNNAudio if name.startswith("vrnn") else SRNNAudio
        m = cls(likelihood="GMM" if name.endswith("gmm") else "DMoL", input_size=S, hidden_size=H, latent_size=Z).cuda()
        for _ in range(2):
            m.generate(n_samples=B, max_timesteps=T)
        torch.cuda.synchronize()
        times = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            (x, _), _ = m.generate(n_samples=B, max_timesteps=T)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        assert torch.isfinite(x).all()
        res[name] = times
    return res


def summary(times):
    q = statistics.quantiles(times, n=4)
    return {"median_s": statistics.median(times), "iqr_s": q[2] - q[0], "min_s": min(times), "max_s": max(times), "calls": len(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit, measured in alternation with this tree")
    ap.add_argument("--tree", default=None, help="(internal) measure the package of this tree and print one JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gauss_rollout_bench.json"))
    a = ap.parse_args()
    if a.tree:
        sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "benchmarking-lvms_amd"))
        print("RESULT " + json.dumps(measure()))
        return
    trees = {"this": ROOT, **({"parent": a.parent_tree} if a.parent_tree else {})}
    calls = {tag: {name: [] for name in MODELS} for tag in trees}
    for _ in range(ROUNDS):
        for tag, tree in trees.items():
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", tree], check=True, capture_output=True, text=True, timeout=1500).stdout
            line = [l for l in out.splitlines() if l.startswith("RESULT ")][-1]
            for name, times in json.loads(line[len("RESULT "):]).items():
                calls[tag][name] += times
    res = {tag: {name: summary(t) for name, t in per.items()} for tag, per in calls.items()}
    doc = {"shape": dict(S=S, H=H, Z=Z, B=B, T=T), "method": f"host clock around generate() + synchronise, 2 warm-ups, {REPS} calls x {ROUNDS} alternating rounds per tree",
           "unit": "seconds per call", "trees": res}  # fmt: skip
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("| model | " + " | ".join(f"{tag}: median (IQR) s" for tag in res) + " |")
    print("|---|" + "---|" * len(res))
    for name in MODELS:
        print(f"| {name} | " + " | ".join(f"{res[tag][name]['median_s']:.5f} ({res[tag][name]['iqr_s']:.5f})" for tag in res) + " |")


if __name__ == "__main__":
    main()
