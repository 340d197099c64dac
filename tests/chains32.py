"""Shared by tests/test_gpu_chains32.py (the kernels) and tests/test_chains32_cpu.py (the float32 stand-in): the cases of the fp32 VRNN
step program (K1, `ops.vrnn_sequence`) and SRNN latent chain (K3, `ops.srnn_latent_chain`) on every dispatch arm, their inputs, the
free-running float64 oracle, the bars and the one function (`judge`) that holds a result against them.

Inputs and oracles are tests/links16.py's (`vrnn_inputs`, `srnn_inputs`, `vrnn_oracle`, `srnn_oracle` with mode "f32": nothing is
rounded and nothing teacher forced), at widths of this file's choosing (X != H != Z != R wherever the arm allows it, so a swapped
leading dimension cannot cancel).  Lengths are ragged through `x_sl` with stride 3 (`t * 3 < x_sl`): row 0 is full, row 1 is an
exact multiple of the stride that ends early, the last row ends after two steps.  Loss of a backward case:
(out * w).sum() + (c_raw * kld + c_fn * kld_fn).sum(), c_raw != c_fn, free nats on.

Free nats.  The floor is the midpoint of the widest gap between neighbouring values of the float64 oracle's live element-wise KL
inside its inter-quartile range, so between 1/4 and 3/4 of the live elements lie above it; which elements sit on the floor is then
decided from the statistics the kernel (or the stand-in) stored (`links16._kl_terms`, `forced_stats`).

Kinks.  A batch row in which the float64 oracle has a hidden pre-activation within KINK32 of zero carries no loss in a backward
case (w = 0, length 0; `links16.bwd_inputs`' mechanism): a float32 evaluation may put that unit on the other branch of its
(Leaky)ReLU, and then no reference exists for the row's gradient at fp32 precision.  KINK32 of a case is 4 x the stand-in's largest
|pre(float32) - pre(float64)| over STANDIN_SEEDS seeds.  The case's seed is the first for which at most 1/4 of the rows are left out,
never all rows of a 16-row tile, never row 0, row 1 (the exact multiple of the stride), the last row or the first row of the last
tile.  The forward of a left-out row is compared like any other.

Bars.  Values: every (t, b) row of every stored tensor and every element of kld / kld_fn at `links16.BAR_VALUE` (1e-5).  Gradients:
per tensor, and per batch row for the inputs' gradients, the larger of `links16.FP32_GRAD_BAR` (2e-5) and 4 x the stand-in's worst
distance over STANDIN_SEEDS seeds, never above 1e-4; recorded in tests/golden/chains32_bars.json by tools/record_chains32_bars.py and
re-asserted entry by entry in tests/test_chains32_cpu.py."""
import collections
import contextlib
import functools
import json
import os

import torch

import blvm_oracle as O
import links16 as L

STRIDE = 3
SRNN_R = 32
FWD_T, BWD_T = 6, 3
MAX_BAR = 1e-4
STANDIN_FACTOR = 4.0  # the GPU's other summation order and the split-bf16 weight-gradient products (their own bar: 3e-6)
OLD_GRAD_BAR = 1e-3  # what the model-level tests hold a gradient tensor to
COEF = (L.SRNN_C_RAW, L.SRNN_C_FN)

# the arms
STATIC, INTERPRETER, ROW_GROUPS, PER_LINK = "static", "interpreter", "rowgroups", "perlink"

Case = collections.namedtuple("Case", "family arm B X H Z R given residual engine")


def _v(arm, B, X, H, Z, R, given, residual, engine=True):
    return Case("vrnn", arm, B, X, H, Z, R, given, residual, engine)


def _s(arm, B, H, Z, given, residual, engine=True):
    return Case("srnn", arm, B, 0, H, Z, SRNN_R, given, residual, engine)


SW = (64, 256, 256, 512)  # X, H, Z, R of the static walk
IW = (48, 64, 32, 96)  # the interpreter's: Z != H, so the phi run opens with its own first link
VRNN_CASES = (
    [_v(STATIC, B, *SW, given, res) for B in (5, 17, 64) for res in (True, False) for given in (True, False)]
    + [_v(INTERPRETER, 21, *IW, True, True), _v(INTERPRETER, 64, *IW, False, False)]
    + [_v(ROW_GROUPS, 65, *IW, True, True), _v(ROW_GROUPS, 150, *IW, False, False)]  # 65: the last group is one tile holding one row
    + [_v(PER_LINK, 21, *IW, True, True, engine=False),  # 16-row tiles
       _v(PER_LINK, 257, 48, 48, 32, 96, True, False),  # H = 48: no link fits 32x32 tiles
       _v(PER_LINK, 257, *IW, True, True),  # every link on 32x32 tiles; the last tile holds one row
       _v(PER_LINK, 257, 48, 64, 48, 96, False, True),  # Z = 48: three column tiles in the head and dz kernels; the links stay on 32x32
       _v(PER_LINK, 257, 48, 64, 32, 80, True, False)]  # R = 80: the 3R- and R-wide links fall back to 16-row tiles inside the sequence
)
SRNN_CASES = (
    [_s(INTERPRETER, B, H, Z, given, res) for B in (5, 37, 128) for H, Z in ((64, 32), (128, 48)) for res in (True, False) for given in (True, False)]
    + [_s(PER_LINK, 129, 64, 32, True, True),  # 32x32 tiles, the last tile holds one row
       _s(PER_LINK, 129, 48, 16, False, False),  # 16-row tiles
       _s(PER_LINK, 5, 64, 32, True, True, engine=False)]
)
# T' = 1: no recurrent gradient product (dz.has_gemm is false; the d_z0 / d_h0 tail reads step 0 directly): one case per arm
T1_CASES = [VRNN_CASES[4], VRNN_CASES[12], VRNN_CASES[14], VRNN_CASES[16], VRNN_CASES[18], SRNN_CASES[8], SRNN_CASES[24], SRNN_CASES[26]]
FWD_CASES = [(c, FWD_T) for c in VRNN_CASES + SRNN_CASES] + [(c, 1) for c in T1_CASES]
BWD_CASES = [(c, BWD_T) for c in VRNN_CASES + SRNN_CASES] + [(c, 1) for c in T1_CASES]


def case_id(ct):
    c, Tp = ct
    widths = f"X{c.X}-H{c.H}-Z{c.Z}-R{c.R}" if c.family == "vrnn" else f"H{c.H}-Z{c.Z}"
    return (f"{c.family}-{c.arm}{'' if c.engine else '-engine_off'}-B{c.B}-{widths}-{'state0' if c.given else 'nostate0'}-"
            f"{'residual' if c.residual else 'plain'}-T{Tp}")  # fmt: skip


# ----------------------------------------------------------------------------------------------------------------------
# which arm a case must take: the increments of blvm_vrnn_path_counts (7 words) / blvm_srnn_path_counts (6 words)
# ----------------------------------------------------------------------------------------------------------------------

VRNN_COUNTERS = ("forward on a program", "forward on launch-per-link", "backward on a program", "backward on launch-per-link",
                 "programs on row groups", "16x16-tile link launches", "32x32-tile link launches")  # fmt: skip
SRNN_COUNTERS = VRNN_COUNTERS[:4] + VRNN_COUNTERS[5:]


def _tiles(B, links):
    """(16-row, 32x32) launches of `links`, each a tuple of its segments' output widths (stages.h `launch_lin_n`: 32x32 tiles from
    128 rows on where every segment's width is a multiple of 32)."""
    wide = [B >= 128 and all(n % 32 == 0 for n in seg) for seg in links]
    return [len(wide) - sum(wide), sum(wide)]


def expected_counts(c, Tp, backward):
    """-> (counter increments, static-walk launches) of one forward (backward: one backward) of the case."""
    H, Z, R = c.H, c.Z, c.R
    if c.family == "vrnn":
        if c.arm != PER_LINK:
            return [0, 0, 1, 0, int(c.arm == ROW_GROUPS), 0, 0] if backward else [1, 0, 0, 0, int(c.arm == ROW_GROUPS), 0, 0], int(c.arm == STATIC)
        # a step: first layers + hidden projection | two more layers | four phi layers;  backward: dphi + G | three phi layers | heads | two layers
        links = [(H, R)] + [(H,)] * 3 + [(H, H)] * 3 if backward else [(H, H, 3 * R)] + [(H, H)] * 2 + [(H,)] * 4
        t = _tiles(c.B, links)
        return ([0, 0, 0, 1, 0] if backward else [0, 1, 0, 0, 0]) + [Tp * t[0], Tp * t[1]], 0
    if c.arm != PER_LINK:
        return [0, 0, 1, 0, 0, 0] if backward else [1, 0, 0, 0, 0, 0], 0
    t = _tiles(c.B, [(H, H)] * 3)  # three two-chain links a step, each way
    tail = _tiles(c.B, [(Z,)] * 2) if backward and c.given else [0, 0]  # d_z0: both first layers of step 0
    return ([0, 0, 0, 1] if backward else [0, 1, 0, 0]) + [Tp * t[0] + tail[0], Tp * t[1] + tail[1]], 0


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------


def ragged_lengths(Tp, B):
    """x_sl for `t * STRIDE < x_sl`: row 0 full, row 1 an exact multiple of the stride that ends early (T' >= 3), the last row ends
    after two steps, the others spread over 1 .. T' * STRIDE."""
    n = Tp * STRIDE
    sl = [(7 * b + 3) % n + 1 for b in range(B)]
    sl[0] = n
    if Tp >= 3:
        sl[1], sl[-1] = 2 * STRIDE, STRIDE + 1
    return torch.tensor(sl, dtype=torch.int64)


def _links16_case(c, Tp):
    return (Tp, c.B, c.H, c.Z, c.given) if c.family == "vrnn" else (Tp, c.B, c.H, c.Z, c.given, c.residual, False)


@functools.lru_cache(maxsize=None)
def raw_inputs(c, Tp, seed=0):
    """links16's inputs of the case at this file's widths, with `lens` = x_sl in samples (read-only: shared)."""
    base = L.vrnn_inputs(_links16_case(c, Tp), seed, Tp, X=c.X, R=c.R) if c.family == "vrnn" else L.srnn_inputs(_links16_case(c, Tp), seed, Tp, R=c.R)
    inp = dict(base)
    inp["lens"] = ragged_lengths(Tp, c.B)
    return inp


def oracle(c, inp, dtype=torch.float64, backward=False, forced_stats=None, free_nats=L.SRNN_FREE_NATS, pre_out=None, residual=None, coef=COEF):
    """The free-running oracle of the case in `dtype` (float32: the stand-in).  -> dict of stored tensors, kld, kld_fn and, with
    `backward`, d_<input>, d_<parameter>."""
    residual = c.residual if residual is None else residual
    if c.family == "vrnn":
        return L.vrnn_oracle(inp, "f32", None, dtype, None, backward, residual=residual, stride=STRIDE, free_nats=free_nats, forced_stats=forced_stats,
                             kl=True, pre_out=pre_out, coef=coef)  # fmt: skip
    case = (0, c.B, c.H, c.Z, c.given, residual, False)
    return L.srnn_oracle(inp, "f32", case, dtype, None, backward, forced_stats, STRIDE, free_nats, pre_out, coef)


def live_mask(inp, Tp):
    return torch.arange(Tp).unsqueeze(1) * STRIDE < inp["lens"].unsqueeze(0)  # [T', B]


def floor_from_reference(ref, live):
    """-> (free nats, share of live elements above the floor): the midpoint of the widest gap of the sorted live KL inside its
    inter-quartile range (module docstring)."""
    kl = O.kl_gaussian(ref["mu_q"], ref["sd_q"], ref["mu_p"], ref["sd_p"])
    v = kl[live].flatten().sort().values
    n = v.numel()
    if n < 8:  # (a seed that leaves every row out: `kink_conditions` turns it down)
        return L.SRNN_FREE_NATS, 0.0
    lo, hi = n // 4, (3 * n) // 4
    gaps = v[lo + 1 : hi + 1] - v[lo:hi]
    i = int(gaps.argmax())
    floor = float((v[lo + i] + v[lo + i + 1]) / 2)
    return floor * kl.shape[-1], float((v > floor).double().mean())


def _pre(c, inp, dtype):
    pre = []
    with torch.no_grad():
        out = oracle(c, inp, dtype, pre_out=pre)
    return torch.stack(pre).double(), out  # [links, B, H]


def kink_measure(c, Tp, seed):
    """The stand-in's largest |pre(float32) - pre(float64)| on one seed."""
    inp = raw_inputs(c, Tp, seed)
    return float((_pre(c, inp, torch.float32)[0] - _pre(c, inp, torch.float64)[0]).abs().max())


def kink_conditions(near):
    """-> the conditions (module docstring) a case's left-out rows miss, [] if none."""
    B = near.numel()
    miss = []
    if int(near.sum()) * 4 > B:
        miss.append(f"{int(near.sum())} of {B} rows left out (cap 1/4)")
    for r0 in range(0, B, 16):
        if bool(near[r0 : r0 + 16].all()):
            miss.append(f"all rows of the tile at row {r0} left out")
    for b in sorted({0, min(1, B - 1), B - 1, (B - 1) // 16 * 16}):
        if bool(near[b]):
            miss.append(f"row {b} left out")
    return miss


@functools.lru_cache(maxsize=None)
def inputs(c, Tp, seed=0, kink=None):
    """-> (inp, free nats, share above the floor).  kink None: a forward case, every row carries loss.  Else the backward case: the rows
    with a hidden pre-activation of the float64 oracle within `kink` of zero carry none (`near_kink`)."""
    base = raw_inputs(c, Tp, seed)
    inp = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in base.items()}
    pre, ref = _pre(c, inp, torch.float64)
    if kink is not None:
        near = pre.abs().amin((0, 2)) < kink
        inp["w"][:, near] = 0
        inp["lens"][near] = 0
        inp["near_kink"] = near
    free_nats, share = floor_from_reference(ref, live_mask(inp, Tp).unsqueeze(-1).expand_as(ref["mu_q"]))
    return inp, free_nats, share


# ----------------------------------------------------------------------------------------------------------------------
# the recorded table
# ----------------------------------------------------------------------------------------------------------------------

BARS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chains32_bars.json")
ROW_GRADS = {"srnn": (("d", 1), ("a", 1), ("z0", 0)), "vrnn": (("enc", 1), ("h0", 0))}  # (input, its batch-row axis)


def grad_names(c):
    if c.family == "srnn":
        return ("d", "a") + (("z0",) if c.given else ()) + O.SRNN_CHAIN_PARAMS
    return ("enc",) + (("h0",) if c.given else ()) + O.VRNN_SEQ_PARAMS


@contextlib.contextmanager
def one_thread():
    """The float32 sums in one fixed order."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(threads)


def standin_result(c, inp, free_nats, **kw):
    """The float32 stand-in in the kernel's place, and the float64 oracle that takes the free-nats decisions from its statistics."""
    stand = oracle(c, inp, torch.float32, backward=True, free_nats=free_nats, **kw)
    return stand, oracle(c, inp, torch.float64, backward=True, forced_stats=stand, free_nats=free_nats)


def measure(ct, kink=None):
    """-> the table entry of a backward case as measured on this host: kink32, seed, bars per tensor, bars per batch row, and the
    stand-in's own figures (`floor`, `row_floor`).  kink: the recorded KINK32 (seed and floors are then those of the recorded case)."""
    c, Tp = ct
    with one_thread():
        measured = L._round_up(STANDIN_FACTOR * max(kink_measure(c, Tp, s) for s in range(L.STANDIN_SEEDS)))
        kink = measured if kink is None else kink
        floor, row_floor = {}, {}
        for s in range(L.STANDIN_SEEDS):
            inp, fn, _ = inputs(c, Tp, s, kink)
            stand, ref = standin_result(c, inp, fn)
            for n in grad_names(c):
                floor[n] = max(floor.get(n, 0.0), L.rel_l2(stand["d_" + n], ref["d_" + n]))
            for n, dim in ROW_GRADS[c.family]:
                if "d_" + n in ref:
                    row_floor[n] = max(row_floor.get(n, 0.0), float(L.row_dist(stand["d_" + n], ref["d_" + n], dim).max()))
    seed = next(s for s in range(64) if not kink_conditions(inputs(c, Tp, s, kink)[0]["near_kink"]))
    bar = lambda v: max(L.FP32_GRAD_BAR, L._round_up(STANDIN_FACTOR * v)) if v > 0 else L.FP32_GRAD_BAR  # noqa: E731
    return dict(kink32=measured, seed=seed, bars={n: bar(v) for n, v in floor.items()}, row_bars={n: bar(v) for n, v in row_floor.items()},
                floor=floor, row_floor=row_floor)


@functools.lru_cache(maxsize=None)
def table():
    with open(BARS_FILE) as f:
        return json.load(f)


def backward_case(ct):
    """-> (inp, free nats, share above the floor, table entry) of a backward case: the recorded seed and KINK32."""
    e = table()[case_id(ct)]
    return inputs(ct[0], ct[1], e["seed"], e["kink32"]) + (e,)


# ----------------------------------------------------------------------------------------------------------------------
# one result against the oracle
# ----------------------------------------------------------------------------------------------------------------------


def value_pieces(c, res, Tp):
    """(name, [T', B, *]) of every stored tensor whose (t, b) rows are compared."""
    if c.family == "vrnn":
        return [("phi", res["decin"][:Tp, :, : c.H]), ("h", res["decin"][1:, :, c.H :])] + [(k, res[k]) for k in L.VRNN_STATS]
    return [("zs", res["zs"][1:])] + [(k, res[k]) for k in L.SRNN_STATS[1:]]


def judge(c, Tp, got, ref, inp, entry=None):
    """Hold `got` (the kernel's result dict, or the stand-in's) against `ref` (the float64 oracle's).  entry: the table entry of a
    backward case, then the gradients are held too.  -> (failures, figures)."""
    fails, fig = [], dict(row=0.0, kl=0.0, tensor=0.0, tensor_share=0.0, grad_row=0.0, grad_row_share=0.0, old_bar=True)
    B = c.B
    state0 = inp["h0" if c.family == "vrnn" else "z0"]
    state0 = torch.zeros(B, c.R if c.family == "vrnn" else c.Z) if state0 is None else state0
    got0 = got["decin"][0, :, c.H :] if c.family == "vrnn" else got["zs"][0]
    if not torch.equal(got0.detach().float().cpu(), state0):
        fails.append("the initial state is not stored as given")
    if c.family == "vrnn" and not bool((got["decin"][Tp, :, : c.H] == 0).all()):
        fails.append("the phi part of decin row T' is not zero")
    for (name, g), (_, r) in zip(value_pieces(c, got, Tp), value_pieces(c, ref, Tp)):
        g = g.detach().double().cpu()
        if not bool(torch.isfinite(g).all()):
            fails.append(f"{name}: non-finite values")
            continue
        d = L.row_dist(g.reshape(Tp * B, -1), r.reshape(Tp * B, -1), 0)
        k = int(d.argmax())
        fig["row"] = max(fig["row"], float(d[k]))
        if float(d[k]) > L.BAR_VALUE:
            fails.append(f"{name} row (step {k // B}, batch row {k % B}): {float(d[k]):.3e} > {L.BAR_VALUE:.0e} ({int((d > L.BAR_VALUE).sum())} rows over)")
    for name in ("kld", "kld_fn"):
        d = L.row_dist(got[name].reshape(B, 1), ref[name].reshape(B, 1), 0)
        k = int(d.argmax())
        fig["kl"] = max(fig["kl"], float(d[k]))
        if not float(d[k]) <= L.BAR_VALUE:
            fails.append(f"{name}[{k}]: {float(d[k]):.3e} > {L.BAR_VALUE:.0e}")
    if entry is None:
        return fails, fig
    for n in grad_names(c):
        g = got["d_" + n]
        if g is None or not bool(torch.isfinite(g).all()):
            fails.append(f"d_{n}: missing or non-finite")
            continue
        e, bar = L.rel_l2(g, ref["d_" + n]), entry["bars"][n]
        fig["tensor"], fig["tensor_share"] = max(fig["tensor"], e), max(fig["tensor_share"], e / bar)
        fig["old_bar"] = fig["old_bar"] and e <= OLD_GRAD_BAR
        if e > bar:
            fails.append(f"d_{n}: {e:.3e} > {bar:.1e}")
    for n, dim in ROW_GRADS[c.family]:
        if "d_" + n not in ref:
            continue
        d, bar = L.row_dist(got["d_" + n], ref["d_" + n], dim), entry["row_bars"][n]
        k = int(d.argmax())
        fig["grad_row"], fig["grad_row_share"] = max(fig["grad_row"], float(d[k])), max(fig["grad_row_share"], float(d[k]) / bar)
        if not float(d[k]) <= bar:
            fails.append(f"d_{n} batch row {k}: {float(d[k]):.3e} > {bar:.1e} ({int((d > bar).sum())} rows over)")
    return fails, fig
