"""Gate of the static-walk kernel (csrc/vrnn_static.hip): the dependent [B,N]x[N,N] relu chain of probe_engine_chain.py, per link,
walked by the interpreter (one descriptor visit per link; BLVM_PCHAIN_PROBE_RUN=4: runs of four links per visit) and by the static
kernel, alternately in one process.  Both outputs must match bit for bit.  The bare tile loop is tools/pchain_probe.hip."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "benchmarking-lvms_amd"))
import torch
from blvm import _hip
from blvm._hip import ptr, stream_ptr, check
lib = _hip.load(); dev = "cuda:0"


def chain(fn, B, N, L, reps=3):
    torch.manual_seed(0)
    W = (torch.rand(N, N, device=dev) * 2 - 1) * 2.45 / N ** 0.5
    b = (torch.rand(N, device=dev) * 2 - 1) * 0.1
    x0 = torch.rand(B, N, device=dev) * 2 - 1
    rows = (B + 15) // 16 * 16
    W16 = torch.empty(N * N, device=dev); x16 = torch.empty((L + 1) * rows * N, device=dev); xs = torch.empty(L, B, N, device=dev)
    check(lib.blvm_pchain_rows_to_t16(ptr(W), N, N, N, ptr(W16), stream_ptr()), "t16 W")
    check(lib.blvm_pchain_rows_to_t16(ptr(x0), N, B, N, ptr(x16), stream_ptr()), "t16 x")
    best = 1e9
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(fn(ptr(W16), ptr(b), ptr(x16), ptr(xs), B, N, L, 0, stream_ptr()), "probe")
        e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    _hip.check_async()
    return best * 1e3 / L, xs.clone()


if __name__ == "__main__":
    L = 2000
    for B, N in ((64, 256), (8, 256), (64, 512)):
        for rep in range(2):  # alternate, twice
            te, xe = chain(lib.blvm_pchain_chain_probe, B, N, L)
            ts, xs = chain(lib.blvm_pchain_static_chain_probe, B, N, L)
            same = bool(torch.equal(xe, xs))
            print(f"B={B} N=K={N} L={L}: engine {te:.3f} us/link, static {ts:.3f} us/link, outputs bit-identical: {same}", flush=True)
            if not same:
                sys.exit(1)
