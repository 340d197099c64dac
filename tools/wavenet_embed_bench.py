"""WaveNet with embedded class input (K10e): the numbers of DESIGN "K10e".

  front     forward and backward of `ops.wavenet_embed_front` at [64, 16000] classes, C = E = 64, for V = 256 and V = 65536, beside
            `F.embedding` + torch's grouped `conv1d` on the same device (the yardstick); ms and achieved GB/s of the bytes the
            algorithm needs: forward = the [T-1, B, C] output once (262 MB) + the classes; backward = d_out read twice (once per tap)
            + the classes, their sort keys and permutation + the dense [V, E] gradient.
  train     one training step (forward, backward, Adam) of the embedded categorical WaveNet and of the float-input categorical
            WaveNet (5 x 10 blocks, 64 channels, V = 256) at [4, 16000].
  generate  frames per second of one-launch generation, embedded against float-input, same network at B = 16.

Device events around whole calls; WINDOWS windows in which the candidates alternate; median (min .. max).  With `--tree PATH` (a built
checkout, e.g. of the parent commit) the package of that tree is imported instead and the embedded rows are left out where it cannot
build them: the "parent" column of the table.

python tools/wavenet_embed_bench.py [--tree PATH] [--only front,train,generate] [--out profiles/wavenet_embed_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
WINDOWS = 5


def timed(fns, reps):
    """{name: () -> None} -> {name: [ms per call of each window]}; the candidates alternate within a window."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    res = {name: [] for name in fns}
    for _ in range(WINDOWS):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) / reps)
    return res


def summary(windows, nbytes=None):
    s = {"median_ms": statistics.median(windows), "min_ms": min(windows), "max_ms": max(windows)}
    if nbytes is not None:
        s["bytes"] = nbytes
        s["GB_per_s"] = nbytes / (s["median_ms"] * 1e-3) / 1e9
    return s


def front(embedded):
    from blvm import ops

    B, T, C = 64, 16000, 64
    out = {}
    for V in (256, 65536):
        torch.manual_seed(0)
        k = torch.randint(0, V, (T, B), device="cuda")
        kb = k.t().contiguous()
        emb = torch.randn(V, C, device="cuda", requires_grad=True)
        cw = (torch.randn(C, 1, 2, device="cuda") * 0.5).requires_grad_(True)
        bias = torch.zeros(C, device="cuda", requires_grad=True)
        d_tm = torch.randn(T - 1, B, C, device="cuda")
        d_bc = d_tm.permute(1, 2, 0).contiguous()  # torch's layout [B,C,T-1]

        def torch_fwd():
            return F.conv1d(F.embedding(kb, emb).transpose(1, 2), cw, bias, groups=C)

        def grads(y, d):
            torch.autograd.grad(y, (emb, cw, bias), d)

        fns = {"torch_fwd": lambda: torch_fwd().detach(), "torch_fwd_bwd": lambda: grads(torch_fwd(), d_bc)}
        if embedded:
            fns["fused_fwd"] = lambda: ops.wavenet_embed_front(k, emb, cw, bias, False).detach()
            fns["fused_fwd_bwd"] = lambda: grads(ops.wavenet_embed_front(k, emb, cw, bias, False), d_tm)
        res = timed(fns, 3)
        n_out = (T - 1) * B * C * 4
        fwd_bytes, bwd_bytes = n_out + T * B * 4, 2 * n_out + 3 * T * B * 4 + V * C * 4
        per = {}
        for side in ("torch", "fused") if embedded else ("torch",):
            fwd, both = res[f"{side}_fwd"], res[f"{side}_fwd_bwd"]
            per[f"{side}_fwd"] = summary(fwd, fwd_bytes)
            per[f"{side}_bwd"] = summary([b - f for b, f in zip(both, fwd)], bwd_bytes)  # the step minus its forward, window by window
        out[f"V={V}"] = per
    return out


def wavenet(embedded_model):
    from blvm.models import WaveNet
    from blvm.modules.distributions import CategoricalDense

    torch.manual_seed(0)
    kw = dict(embedding_dim=64, num_bins=256) if embedded_model else {}
    return WaveNet(likelihood=CategoricalDense(64, 256), n_layers=10, n_stacks=5, res_channels=64, **kw).cuda()


def train(embedded):
    B, T = 4, 16000
    x_sl = torch.full((B,), T)
    torch.manual_seed(1)
    k = torch.randint(0, 256, (B, T), device="cuda")
    fns = {}
    for name in ("float_input", "embedded") if embedded else ("float_input",):
        m = wavenet(name == "embedded")
        opt = torch.optim.Adam(m.parameters(), lr=3e-4)
        x = k if name == "embedded" else m.likelihood.levels[k]

        def step(m=m, opt=opt, x=x):
            loss = m(x, x_sl)[0]
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()

        fns[name] = step
    return {name: summary(w) for name, w in timed(fns, 2).items()}


def generate(embedded):
    B, n = 16, 400
    fns = {}
    for name in ("float_input", "embedded") if embedded else ("float_input",):
        m = wavenet(name == "embedded")
        assert m._cat_decode_kernel_applies()
        fns[name] = lambda m=m: m.generate(B, n, cached=True)
    out = {}
    for name, w in timed(fns, 1).items():
        out[name] = summary(w)
        out[name]["frames_per_s"] = B * n / (out[name]["median_ms"] * 1e-3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT, help="the tree whose package is imported (a built checkout)")
    ap.add_argument("--only", default="front,train,generate")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wavenet_embed_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "benchmarking-lvms_amd"))
    from blvm import ops

    embedded = hasattr(ops, "wavenet_embed_front")
    parts = {"front": front, "train": train, "generate": generate}
    doc = {"device": torch.cuda.get_device_name(0), "tree": os.path.relpath(os.path.abspath(a.tree), os.path.abspath(ROOT)), "embedded_built": embedded,
           "method": f"device events around whole calls, {WINDOWS} alternating windows, median (min .. max)"}  # fmt: skip
    for name in a.only.split(","):
        doc[name] = parts[name](embedded)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
