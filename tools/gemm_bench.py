"""Diagnostic: TF/s of blvm_gemm_f32 on the shapes the models use (run on the GPU box)."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "benchmarking-lvms_amd"))
from blvm import ops  # noqa: E402

dev = "cuda:0"
shapes = [  # (name, op_a, op_b, M, N, K, split_k)
    ("enc L1   fwd", 0, 0, 16000, 256, 64, 1),
    ("mlp      fwd", 0, 0, 16000, 256, 256, 1),
    ("dec L1   fwd", 0, 0, 16000, 256, 768, 1),
    ("dec L3   fwd", 0, 0, 16000, 1920, 256, 1),
    ("dec L3 dgrad", 0, 1, 16000, 256, 1920, 1),
    ("dec L3 wgrad", 1, 1, 1920, 256, 16000, 8),
    ("whh    wgrad", 1, 1, 1536, 512, 16000, 4),
    ("mlp    wgrad", 1, 1, 256, 256, 16000, 48),
    ("XG       fwd", 0, 0, 16000, 1536, 256, 1),
    ("wavenet conv", 0, 0, 84468, 192, 96, 1),
    ("wavenet 1x1 ", 0, 0, 84468, 192, 96, 1),
    ("big square  ", 0, 0, 4096, 4096, 4096, 1),
]

# `gemm_bench.py ws [name filter ...]`: the forward / data-gradient shapes with K <= 256 on BOTH paths of one library — the staged
# tiles (row threshold raised past every M) and the weight-stationary path (threshold 1) — with the epilogues the models use.  10
# warm-up launches per path; the timed launches rotate through operand sets that together exceed the Infinity Cache, so no launch
# finds its operands warm (warm repeated operands misled the weight-gradient work).
ws_shapes = [  # (name, op_b, M, N, K, epilogue) — VRNN [64, 16000]: rows = 16 000; CW-VAE C4: rows = 398 848
    ("enc L1    fwd", 0, 16000, 256, 64, "leaky"),
    ("enc L2/L3 fwd", 0, 16000, 256, 256, "leaky"),
    ("XQ        fwd", 0, 16000, 256, 256, "none"),
    ("XG        fwd", 0, 16000, 1536, 256, "none"),
    ("dec L3    fwd", 0, 16000, 1920, 256, "none"),
    ("mlp     dgrad", 1, 16000, 256, 256, "gate"),
    ("d_enc DQ0 dgr", 1, 16000, 256, 256, "acc"),
    ("dec L1  dgrad", 1, 16000, 768, 256, "none"),
    ("cw C->4C  fwd", 0, 398848, 768, 192, "leaky"),
    ("cw 4C->C dgrd", 1, 398848, 768, 192, "gate"),
    ("rows  256 fwd", 0, 256, 256, 256, "leaky"),
    ("rows 1024 fwd", 0, 1024, 256, 256, "leaky"),
    ("rows 4096 fwd", 0, 4096, 256, 256, "leaky"),
    ("rows 1024 wide", 0, 1024, 1536, 256, "none"),
    ("rows 1024 K64", 0, 1024, 256, 64, "leaky"),
]


def bench_ws(only):
    from blvm import _hip

    lib = _hip.load()
    builtin = lib.blvm_gemm_ws_min_rows(-1)
    print(f"built-in row threshold {lib.blvm_gemm_ws_min_rows(-1)}; us per launch, staged tiles -> weight-stationary")
    for name, ob, M, N, K, epi in ws_shapes:
        if only and not any(o in name for o in only):
            continue
        per_set = 4 * (M * K + M * N * (2 if epi in ("gate", "acc") else 1))
        nset = max(2, min(24, (640 << 20) // per_set + 1)) if per_set < (640 << 20) else 1
        sets = []
        for _ in range(nset):
            A = torch.randn(M, K, device=dev)
            C = torch.randn(M, N, device=dev)
            G = torch.randn(M, N, device=dev) if epi == "gate" else None
            sets.append((A, C, G))
        B = torch.randn((K, N) if ob else (N, K), device=dev)
        bias = torch.randn(N, device=dev) if epi == "leaky" else None

        def f(i):
            A, C, G = sets[i % nset]
            ops.gemm(0, ob, M, N, K, A, K, B, B.shape[1], C, N, bias=bias, act=ops.ACT_LEAKY if epi == "leaky" else ops.ACT_NONE,
                     slope=0.01, gate=G, ldg=N if G is not None else 0, accumulate=epi == "acc")  # fmt: skip

        us = []
        for min_rows in (2**31 - 1, 1):
            lib.blvm_gemm_ws_min_rows(min_rows)
            for i in range(10):
                f(i)
            n = max(2 * nset, 10)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(n):
                f(i)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) / n * 1e3)
        lib.blvm_gemm_ws_min_rows(-1)
        tf = [2 * M * N * K / u / 1e6 for u in us]
        print(f"{name}  op_b={ob} M={M:6d} N={N:5d} K={K:4d} {epi:5s} sets={nset:2d}  {us[0]:8.1f} -> {us[1]:8.1f} us   {tf[0]:6.1f} -> {tf[1]:6.1f} TF/s", flush=True)
        del sets
    assert lib.blvm_gemm_ws_min_rows(-1) == builtin


if sys.argv[1:2] == ["ws"]:
    bench_ws(sys.argv[2:])
    sys.exit(0)

for name, oa, ob, M, N, K, sk in shapes:
    A = torch.randn((K, M) if oa else (M, K), device=dev)
    B = torch.randn((K, N) if ob else (N, K), device=dev)
    C = torch.zeros(M, N, device=dev)
    f = lambda: ops.gemm(oa, ob, M, N, K, A, A.shape[1], B, B.shape[1], C, N, accumulate=sk > 1, split_k=sk)  # noqa: E731
    for _ in range(3):
        f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        f()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 20
    print(f"{name}  M={M:6d} N={N:5d} K={K:6d} split={sk:3d}  {ms * 1e3:8.1f} us  {2 * M * N * K / ms / 1e9:7.1f} TF/s")
