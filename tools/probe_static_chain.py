"""Gate of the static-walk kernel (csrc/vrnn_static.hip): the dependent [B,N]x[N,N] relu chain of probe_engine_chain.py, per link,
walked by the interpreter (one descriptor visit per link; BLVM_PCHAIN_PROBE_RUN=4: runs of four links per visit) and by the static
kernel in its two forms — `fetch`: the weight fragments are re-read every link, `resident`: they are loaded once per launch and stay
in registers — alternately in one process.  All outputs must match bit for bit.  Per shape: `--repeats` rounds (each figure the best
of three launches), the spread of the fetch form over the rounds and the median gain of the resident form over it.

--bare PATH: also run the bare tile loop (tools/pchain_probe.hip built to PATH) and print its output beside the rows.

--paced E:P[,E:P...]: also run the resident form under each poll pacing setting (csrc/pchain.h "poll pacing"; first-poll delay of E
s_sleep units on the waves that leave a tile at its barrier and P on the epilogue waves, blvm_pchain_static_chain_probe_paced),
alternated with the others in every round, checked bit for bit, and print per shape each setting's median, spread and gain over the
plain resident form.

--places P[,P...]: run the resident and paced forms under each placement of the static launch (csrc/vrnn_static.h Place: 0 the
program's TileIter mode, 1 plain TileIter, 2 plain behind the block-index permutation; bits 32 / 64 of blvm_pchain_tune), alternated
in every round."""
import argparse, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "benchmarking-lvms_amd"))
import torch
from blvm import _hip
from blvm._hip import ptr, stream_ptr, check
lib = _hip.load(); dev = "cuda:0"


def paced(early, epi):
    return lambda W16, b, x16, xs, B, N, L, nwg, stream: lib.blvm_pchain_static_chain_probe_paced(W16, b, x16, xs, B, N, L, nwg, early, epi, stream)


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
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--links", type=int, default=2000)
    ap.add_argument("--bare", default=None, help="the built tools/pchain_probe binary")
    ap.add_argument("--paced", default="", help="pacing settings EARLY:EPI, comma separated")
    ap.add_argument("--places", default="", help="placements of the static launch (0, 1, 2), comma separated; empty: the tune bits as they are")
    ap.add_argument("--shapes", default="64:256,8:256,64:512,8:512", help="B:N, comma separated")
    args = ap.parse_args()
    L = args.links
    settings = [tuple(int(v) for v in item.split(":")) for item in args.paced.split(",") if item]
    places = [int(v) for v in args.places.split(",") if v] or [None]
    base = int(os.environ.get("BLVM_PCHAIN_TUNE", "84")) & ~96  # the program's own bits; 32 / 64 select the placement
    tag = lambda pl: "" if pl is None else f" place={pl}"
    for B, N in (tuple(int(v) for v in item.split(":")) for item in args.shapes.split(",")):
        fetch, res, pc = [], {pl: [] for pl in places}, {(pl, st): [] for pl in places for st in settings}
        for rep in range(args.repeats):  # alternate
            te, xe = chain(lib.blvm_pchain_chain_probe, B, N, L)
            tf, xf = chain(lib.blvm_pchain_static_chain_probe_fetch, B, N, L)
            same = bool(torch.equal(xe, xf))
            print(f"B={B} N=K={N} L={L}: engine {te:.3f} us/link, static fetch {tf:.3f}, outputs bit-identical: {same}", flush=True)
            if not same:
                sys.exit(1)
            fetch.append(tf)
            for pl in places:
                if pl is not None:
                    lib.blvm_pchain_tune(base | (0, 32, 96)[pl])
                tr, xr = chain(lib.blvm_pchain_static_chain_probe, B, N, L)
                same = bool(torch.equal(xe, xr))
                print(f"  {tag(pl)} static resident {tr:.3f} us/link, bit-identical to the engine: {same}", flush=True)
                if not same:
                    sys.exit(1)
                res[pl].append(tr)
                for st in settings:
                    tp, xp = chain(paced(*st), B, N, L)
                    ok = bool(torch.equal(xp, xe))
                    print(f"  {tag(pl)} paced early={st[0]} epi={st[1]}: {tp:.3f} us/link, bit-identical to the engine: {ok}", flush=True)
                    if not ok:
                        sys.exit(1)
                    pc[pl, st].append(tp)
                if pl is not None:
                    lib.blvm_pchain_tune(-1)  # (the engine and the fetch form run with the bits of the environment)
        med = statistics.median
        print(f"B={B} N=K={N}: fetch median {med(fetch):.3f} spread {max(fetch) - min(fetch):.3f}", flush=True)
        for pl in places:
            print(f"B={B} N=K={N}{tag(pl)}: resident median {med(res[pl]):.3f} spread {max(res[pl]) - min(res[pl]):.3f}, "
                  f"gain over fetch {med(fetch) - med(res[pl]):.3f} us/link", flush=True)
            for st in settings:
                v = pc[pl, st]
                print(f"B={B} N=K={N}{tag(pl)}: paced early={st[0]} epi={st[1]} median {med(v):.3f} spread {max(v) - min(v):.3f}, "
                      f"gain over resident {med(res[pl]) - med(v):+.3f} us/link", flush=True)
    if args.bare:
        print(f"bare tile loop ({args.bare} {L} 1):", flush=True)
        out = subprocess.run([args.bare, str(L), "1"], capture_output=True, text=True, timeout=300)
        print(out.stdout + out.stderr, flush=True)
        sys.exit(out.returncode)
