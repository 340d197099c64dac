"""Diagnostic (GPU box): price the weight-gradient GEMMs dW[M,N] += D^T Act (D [rows, M], Act [rows, N], both row-major) of the
tree this file sits in, on the shapes the models run.

  * the VRNN chain's weight gradients (vrnn.hip, the grouped launch of the batched part; X = H = Z = 256, R = 512 at the headline
    configuration, rows = 16 000) one by one and as ONE grouped launch (blvm_wgrad_group_f32), with their bias gradients;
  * the VRNN decoder's three weight gradients (768 -> 256 -> 256 -> 1920) as the grouped launch the MLP's backward hands over;
  * MLP-like groups (three layers, as ops.py's _MLPFunction backward hands them over);
  * single weight-gradient GEMMs through blvm_gemm_f32 (op_a = op_b = 1) at the CW-VAE / STCN / VRNN shapes.

Run it in the old and in the new tree on one box to compare (BLVM_HIP_LIB=<other library> times another build of the library under
this tree's Python, as long as both export the same entry points).  Prints one line per case: microseconds and TF/s.

  (no argument)   every case once
  chain           the chain group alone, full and ragged row counts interleaved (for counters / A-B)
  groups          chain group, decoder group and the single shapes 1536 x 512 x 16000 and 256 x 256 x 64000, three rounds (A-B of two
                  libraries: one process each, alternated by the caller)"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "benchmarking-lvms_amd"))
from blvm import _hip, ops  # noqa: E402

dev = "cuda:0"
ROWS = int(os.environ.get("ROWS", 16000))
REPS = int(os.environ.get("REPS", 20))
X = H = Z = 256
R = 512  # the recurrent state of the headline model (hidden 256, r_dim = 2 hidden)


def chain_jobs():
    """(M, N, bias) of every weight gradient of the VRNN chain's grouped launch, in vrnn.hip's order."""
    j = [(3 * R, X, True), (3 * R, H, False), (3 * R, R, True), (H, Z, True)]
    j += [(H, H, True)] * 3
    j += [(2 * Z, H, True), (2 * Z, H, True)]
    j += [(H, H, True)] * 4
    j += [(H, R, True), (H, R, False), (H, X, True)]
    return j


def decoder_jobs():
    """(M, N, bias) of the headline decoder's weight gradients: Linear(H + R, H), Linear(H, H), Linear(H, 1920) (the DMoL head of a
    64-sample frame stack with 10 mixture components)."""
    return [(H, H + R, True), (H, H, True), (1920, H, True)]


def timed(f):
    for _ in range(10):  # (with 3 the first case of a process read ~13 % slow: 813 against 707 us for the chain group)
        f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3  # us


def group_case(name, shapes, rows):
    g = torch.Generator(device=dev).manual_seed(0)
    jobs = []
    for M, N, bias in shapes:
        D = torch.randn(rows, M, device=dev, generator=g)
        A = torch.randn(rows, N, device=dev, generator=g)
        jobs.append((D, A, torch.zeros(M, N, device=dev), torch.zeros(M, device=dev) if bias else None))
    flop = sum(2 * M * N * rows for M, N, _ in shapes)
    us = timed(lambda: ops.wgrad_group(jobs, rows))
    print(f"{name:34s} jobs={len(shapes):2d} rows={rows:6d}  {us:8.1f} us  {flop / us / 1e6:6.1f} TF/s", flush=True)
    return us


def single_case(M, N, K):
    g = torch.Generator(device=dev).manual_seed(1)
    D = torch.randn(K, M, device=dev, generator=g)
    A = torch.randn(K, N, device=dev, generator=g)
    C = torch.zeros(M, N, device=dev)
    tiles = ((M + 63) // 64) * ((N + 63) // 64)
    sk = max(1, min((768 + tiles - 1) // tiles, (K + 255) // 256))  # the callers' request (common.h gemm_pick_split)
    us = timed(lambda: ops.gemm(1, 1, M, N, K, D, M, A, N, C, N, accumulate=True, split_k=sk))
    print(f"gemm_f32 (1,1) M={M:5d} N={N:4d} K={K:6d}       {us:8.1f} us  {2 * M * N * K / us / 1e6:6.1f} TF/s", flush=True)
    return us


def main():
    if sys.argv[1:] == ["chain"]:  # the grouped chain launch alone, full and ragged row counts interleaved (for counters / A-B)
        for _ in range(3):
            group_case("chain group (one launch)", chain_jobs(), ROWS)
            group_case("chain group, ragged rows", chain_jobs(), ROWS - 5)
        return
    if sys.argv[1:] == ["groups"]:
        print(f"library: {os.path.basename(_hip.lib_path())}")
        for _ in range(3):
            group_case("chain group (one launch)", chain_jobs(), ROWS)
            group_case("decoder group (one launch)", decoder_jobs(), ROWS)
            single_case(1536, 512, 16000)
            single_case(256, 256, 64000)
        return
    print(f"tree: {os.path.dirname(os.path.abspath(__file__))}/..  device: {torch.cuda.get_device_name(0)}")
    total = 0.0
    for i, (M, N, bias) in enumerate(chain_jobs()):
        total += group_case(f"chain job {i:2d} {M}x{N}{' +db' if bias else ''}", [(M, N, bias)], ROWS)
    print(f"chain jobs one by one: {total:.1f} us in all")
    group_case("chain group (one launch)", chain_jobs(), ROWS)
    group_case("chain group, ragged rows", chain_jobs(), ROWS - 5)
    group_case("decoder group (one launch)", decoder_jobs(), ROWS)
    group_case("encoder-like MLP group", [(256, 64, True), (256, 256, True), (256, 256, True)], ROWS)
    group_case("decoder-like MLP group", [(256, 512, True), (256, 256, True), (256, 256, True)], ROWS)
    for M, N, K in [(256, 256, 16000), (768, 256, 16000), (1536, 512, 16000), (768, 192, 393216), (192, 192, 98304),
                    (384, 192, 49152), (256, 256, 64000), (60, 60, 8000)]:
        single_case(M, N, K)


if __name__ == "__main__":
    main()
