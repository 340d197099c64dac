"""Anatomy of the resident operand poll (csrc/pchain.h product_regs) in a -DPCHAIN_TPROF build of the library
(tools/probe_build_variant.sh tprof -DPCHAIN_TPROF, then BLVM_HIP_LIB=scratch/variants/tprof/libblvm_hip.so): per visit kind and wave
class — the epilogue waves 0 .. 3 and the waves 4 .. 15 that leave a tile at its barrier — polls per tile, us from the first issue of a
tile's operand poll to the successful one, and us from there to the tile's last T16 store (waves that store nothing: to the end of
the tile).  Means over the waves of a class, over all tiles of the first workgroup of each role.

Rows: the resident chain probe (K = 256 / 512, B = 8 / 64; --paced E:P adds the same chain under that first-poll delay) and the
VRNN forward and backward programs of bench.py's shape ([64, T' = 250], H = Z = 256).  A default build prints zeros.
With the decoder leader on the backward walk's spare range (blvm_vrnn_dec_bwd_fold, the default) the spare role also prints its
resident leader link and, per walk step, the time it spends in the leader's three links and in the arming stores against the
whole step; --no-leader runs the same steps with the switch off.  The decoder's gradient dZ3 is the DMoL head's on random
audio: what the leader costs does not depend on its values.
With the d_enc follower on the backward walk's posterior half (blvm_vrnn_enc_bwd_fold, the default) that role also prints the
follower's resident link and, per walk step, the time it spends in the follower's two links against the whole step and the wait
that is left in front of its next critical poll (link 0 of its run); --no-enc-fold runs the same steps with the switch off."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "benchmarking-lvms_amd"))
import torch
from blvm import _hip
from blvm._hip import ptr, stream_ptr, check
from blvm.models import VRNNAudio
lib = _hip.load(); dev = torch.device("cuda:0")
BASE, ROLE = 128, 512  # csrc/vrnn_static.hip kAnatBase, kAnatRole
TICK = 0.01            # us per wall-clock tick
FWD = {4: "prior run, link 0 (K=512, after the GRU)", 5: "prior run, link 1", 6: "prior run, link 2", 8: "posterior run, link 0 (K=512, after the GRU)",
       9: "posterior run, link 1", 10: "posterior run, link 2", 12: "heads", 16: "phi_z run, link 0 (after the heads)", 17: "phi_z run, link 1",
       18: "phi_z run, link 2", 19: "phi_z run, link 3", 20: "GRU"}
BWD = {0: "GRU backward", 4: "partial sum, prior half (K=512)", 8: "partial sum, posterior half (K=512)", 12: "partial sum, spare range (K=512)",
       20: "summing link", 24: "phi_z run, link 0", 25: "phi_z run, link 1", 28: "dz", 32: "prior run, link 0 (K=512, after dz)",
       33: "prior run, link 1", 34: "prior run, link 2", 36: "posterior run, link 0 (K=512, after dz)", 37: "posterior run, link 1", 38: "posterior run, link 2",
       44: "decoder leader, dY1 (K=256, resident)", 56: "d_enc follower, d_enc (K=256, resident)"}


def rows(h, role, names):
    for slot, name in names.items():
        out = []
        for cls in (0, 1):
            q = h[BASE + role * ROLE + (slot * 2 + cls) * 4:][:4]
            n = max(q[0], 1)
            out.append(f"{q[1] / n:5.2f} polls {q[2] * TICK / n:6.3f} us issue->ok {q[3] * TICK / n:6.3f} us ok->store" if q[0] else "-" * 52)
        if out[0][0] != "-" or out[1][0] != "-":
            print(f"   {name:44s} | waves 0-3: {out[0]} | waves 4-15: {out[1]}", flush=True)


def profiled(fn):
    buf = torch.zeros(4096, dtype=torch.int64, device=dev)
    lib.blvm_pchain_profile(buf.data_ptr())
    fn()
    torch.cuda.synchronize(); lib.blvm_pchain_profile(None)
    _hip.check_async()
    return buf.cpu().tolist()


def chain(B, N, L, early, epi):
    torch.manual_seed(0)
    W = (torch.rand(N, N, device=dev) * 2 - 1) * 2.45 / N ** 0.5
    b = (torch.rand(N, device=dev) * 2 - 1) * 0.1
    x0 = torch.rand(B, N, device=dev) * 2 - 1
    rws = (B + 15) // 16 * 16
    W16 = torch.empty(N * N, device=dev); x16 = torch.empty((L + 1) * rws * N, device=dev); xs = torch.empty(L, B, N, device=dev)
    check(lib.blvm_pchain_rows_to_t16(ptr(W), N, N, N, ptr(W16), stream_ptr()), "t16 W")
    check(lib.blvm_pchain_rows_to_t16(ptr(x0), N, B, N, ptr(x16), stream_ptr()), "t16 x")
    h = profiled(lambda: check(lib.blvm_pchain_static_chain_probe_paced(ptr(W16), ptr(b), ptr(x16), ptr(xs), B, N, L, 0, early, epi, stream_ptr()), "probe"))
    print(f"chain probe B={B} K={N} L={L}, first-poll delay early={early} epi={epi}:", flush=True)
    rows(h, 0, {0: "link"})


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--links", type=int, default=2000)
    ap.add_argument("--paced", default="", help="first-poll delays EARLY:EPI for a second pass over the chain probe, comma separated")
    ap.add_argument("--steps", type=int, default=3, help="profiled VRNN train steps")
    ap.add_argument("--no-leader", action="store_true", help="blvm_vrnn_dec_bwd_fold(0): the decoder's data gradients as K6 launches")
    ap.add_argument("--no-enc-fold", action="store_true", help="blvm_vrnn_enc_bwd_fold(0): d_enc as two K6 launches behind the walk")
    ap.add_argument("--no-chain", action="store_true", help="skip the chain probe rows")
    args = ap.parse_args()
    settings = [(0, 0)] + [tuple(int(v) for v in item.split(":")) for item in args.paced.split(",") if item]
    if args.no_leader:
        lib.blvm_vrnn_dec_bwd_fold(0)
    enc_fold = getattr(lib, "blvm_vrnn_enc_bwd_fold", None)  # (a library from before the follower: none)
    if args.no_enc_fold and enc_fold:
        enc_fold(0)
    for B, N in () if args.no_chain else ((64, 256), (8, 256), (64, 512), (8, 512)):
        for st in settings:
            chain(B, N, args.links, *st)
    B, T = 64, 16000
    torch.manual_seed(0)
    model = VRNNAudio(likelihood="DMoL", input_size=64, hidden_size=256, latent_size=256, residual_posterior=True).to(dev)
    x = (torch.rand(B, T) - 0.5).to(dev); x_sl = torch.full((B,), T, dtype=torch.int64)

    def step():
        model.zero_grad(); loss, _, _ = model(x, x_sl, beta=1.0, free_nats=2.0); loss.backward()

    for _ in range(2):
        step()
    n0, f0, e0 = lib.blvm_pchain_static(-2), lib.blvm_vrnn_dec_bwd_fold(-2), enc_fold(-2) if enc_fold else 0
    h = profiled(lambda: [step() for _ in range(args.steps)])
    print(f"VRNN [64, T'=250], {args.steps} train steps, static launches {lib.blvm_pchain_static(-2) - n0}, "
          f"backward launches with the decoder leader {lib.blvm_vrnn_dec_bwd_fold(-2) - f0}, with the d_enc follower "
          f"{(enc_fold(-2) if enc_fold else 0) - e0}:", flush=True)
    for title, role, names in (("forward, prior half (workgroup 0)", 0, FWD), ("forward, posterior half", 1, FWD), ("backward, prior half (workgroup 0)", 2, BWD),
                               ("backward, posterior half", 3, BWD), ("backward, spare range", 4, BWD)):
        print(f" {title}:", flush=True)
        rows(h, role, names)
        if role == 3:  # (the last profiled launch: csrc/vrnn_static.hip bwd_post_follower)
            q, w, nxt = h[BASE + 3 * ROLE + 13 * 8:][:4], h[BASE + 3 * ROLE + 14 * 8:][:4], h[BASE + 3 * ROLE + 36 * 8:][:4]
            if q[0] and w[0] == 1:
                print(f"   per walk step ({q[0]} steps): follower links {q[2] * TICK / q[0]:6.2f} us, whole step {w[2] * TICK / q[0]:6.2f} us; "
                      f"wait left in front of the run's link 0 (waves 0-3, issue->ok): {nxt[2] * TICK / max(nxt[0], 1):6.3f} us", flush=True)
    q, w = h[BASE + 4 * ROLE + 13 * 8:][:4], h[BASE + 4 * ROLE + 14 * 8:][:4]  # (the last profiled launch: csrc/vrnn_static.hip bwd_spare_leader)
    if q[0]:
        print(f"   per walk step ({q[0]} steps): leader links {q[2] * TICK / q[0]:6.2f} us, arming stores {q[3] * TICK / q[0]:6.2f} us, "
              f"whole step {w[2] * TICK / q[0]:6.2f} us", flush=True)
