"""Shared by tests/test_gpu_16bit_links.py (the kernels) and tests/test_rounded_oracle_cpu.py (the float32 stand-in): the cases, their
inputs, wrappers of the teacher-forced rounded-operand oracles (LSTM, GRU, WaveNet block, SRNN chain, VRNN sequence) and the bars.

One function per family makes the inputs of a case for both files, so what the CPU file establishes about a case (the stand-in's
floor, the distance between the mode and fp32, how many rows flip) is established for the inputs the GPU file runs.

Bars.  One product deep: the tight bar of tests/test_gpu_rnn_sequences.py, relative L2 <= 1e-5 per (t, b) row.  Several links deep:
`two_tier`.  Gradients run free through the rounding points of the backward, so a 1e-7 difference upstream flips an operand by a
16-bit ulp: per tensor the bar is `grad_bar` / `WN_GRAD_BAR` / `bwd_bars`, which the CPU file holds between 3 times the
stand-in's largest float32-vs-float64 distance over STANDIN_SEEDS seeds and half the smallest distance between the rounded and the
unrounded oracle, for every case and tensor; every batch row of an input's gradient is under a loose bar, a multiple of the case's
median row distance between the two oracles that is at least twice the stand-in's worst row in those units."""
import functools
import json
import math
import os

import torch

import blvm_oracle as O
from rnn_arms import PER_STEP, PROGRAM, REGS, unsorted_lens

MODES = ("bf16", "f16")
STANDIN_SEEDS = 5  # seed 0 is the one the GPU file runs
BAR_VALUE = 1e-5  # tests/test_gpu_rnn_sequences.py
# Gradient bars, relative L2 per tensor: [mode][arm class][tensor].  "persistent": both persistent arms (recurrent product rounded);
# "per_step": one launch per step (recurrent product in fp32, so d_h0 / d_c0 / the bias sums feel the mode only through the input
# projection and sit at the project's fp32 bars).  test_rounded_oracle_cpu.py holds every entry between 3 x the stand-in's floor and
# half the mode's own distance, for every case that uses it.
GRAD_BAR = {
    "bf16": {
        "persistent": dict(x=5e-4, h0=5e-4, c0=1e-4, Wih=5e-4, Whh=5e-4, bih=1e-4, bhh=1e-4),
        "per_step": dict(x=2e-4, h0=2e-5, c0=2e-5, Wih=2e-4, Whh=2e-4, bih=2e-5, bhh=2e-5),
    },
    "f16": {
        "persistent": dict(x=1.2e-4, h0=1.2e-4, c0=3e-5, Wih=1.2e-4, Whh=1.2e-4, bih=2e-5, bhh=2e-5),
        "per_step": dict(x=6e-5, h0=1e-5, c0=1e-5, Wih=6e-5, Whh=6e-5, bih=1e-5, bhh=1e-5),
    },
}
GRU_H0_F16 = 6e-5  # the GRU's d_h0 is half as far from fp32 as the LSTM's (h also passes the update gate unrounded): its own entry
LOOSE_MULTIPLE = 1.25
MODE_ON = 10.0  # the output is at least this many times closer to the rounded oracle than to the unrounded one

# (T, B, I, H, arm with the engine on): unsorted lengths with a row of length 0
LSTM_CASES = [
    (6, 21, 16, 32, PROGRAM),
    (5, 21, 16, 48, PROGRAM),     # k-tail
    (5, 37, 24, 128, REGS),
    (5, 37, 24, 384, REGS),       # the only NCH = 3
    (5, 17, 16, 128, REGS),       # the second tile holds one row
    (4, 129, 16, 256, PER_STEP),  # the recurrent product is fp32; the input projection and the weight gradients are rounded
    (3, 21, 16, 128, PER_STEP),
]
# (T, B, I, R, arm with the engine on, reversed)
GRU_CASES = [
    (5, 21, 16, 64, PROGRAM, False),
    (5, 21, 24, 384, PROGRAM, True),
    (5, 17, 16, 128, REGS, False),
    (5, 17, 16, 128, REGS, True),
    (4, 128, 16, 128, REGS, False),
    (4, 129, 16, 128, PER_STEP, False),
]
LSTM_GRADS = ("x", "h0", "c0", "Wih", "Whh", "bih", "bhh")
GRU_GRADS = ("x", "h0", "Wih", "Whh", "bih", "bhh")
ROW_GRADS = ("x", "h0", "c0")  # gradients with a batch-row axis: x on dim 1, the states on dim 0


def lstm_id(c):
    return f"T{c[0]}-B{c[1]}-I{c[2]}-H{c[3]}"


def gru_id(c):
    return f"T{c[0]}-B{c[1]}-I{c[2]}-R{c[3]}-{'reversed' if c[5] else 'forward'}"


def _uniform(g, shape, k):
    return (torch.rand(shape, generator=g) * 2 - 1) * k


@functools.lru_cache(maxsize=None)
def lstm_inputs(case, seed=0):
    """fp32; inputs, initial states and the upstream gradient `w` of unit scale (read-only: shared)."""
    T_, B, I, H, _ = case
    g = torch.Generator().manual_seed(100000 * seed + 1000 * H + 10 * B + T_)
    k = H ** -0.5
    p = dict(Wih=_uniform(g, (4 * H, I), k), Whh=_uniform(g, (4 * H, H), k), bih=_uniform(g, (4 * H,), k), bhh=_uniform(g, (4 * H,), k))
    return dict(x=torch.randn(T_, B, I, generator=g), h0=torch.randn(B, H, generator=g), c0=torch.randn(B, H, generator=g),
                w=torch.randn(T_, B, H, generator=g), lens=unsorted_lens(T_, B), **p)


@functools.lru_cache(maxsize=None)
def gru_inputs(case, seed=0):
    T_, B, I, R, _, reverse = case
    g = torch.Generator().manual_seed(100000 * seed + 3000 * R + 10 * B + T_ + int(reverse))
    k = R ** -0.5
    p = dict(Wih=_uniform(g, (3 * R, I), k), Whh=_uniform(g, (3 * R, R), k), bih=_uniform(g, (3 * R,), k), bhh=_uniform(g, (3 * R,), k))
    return dict(x=torch.randn(T_, B, I, generator=g), h0=torch.randn(B, R, generator=g), w=torch.randn(T_, B, R, generator=g),
                lens=unsorted_lens(T_, B, with_zero=False) if reverse else None, **p)


def grad_bar(family, mode, arm, name):
    if family == "gru" and mode == "f16" and name == "h0" and arm != PER_STEP:
        return GRU_H0_F16
    return GRAD_BAR[mode]["per_step" if arm == PER_STEP else "persistent"][name]


def recurrent_rounded(arm):
    """csrc/rnn.hip: `seq_ot` is the mode's type on both persistent arms and OP_F32 with one launch per step."""
    return arm != PER_STEP


def lstm_oracle(inp, mode, arm, dtype=torch.float64, forced_out=None):
    """-> dict(out, h_n, c_n, d_x, ...): `O.lstm_sequence_rounded_ref` on `inp` widened (exactly) to `dtype`, and its backward of
    (out * w).sum().  mode "f32": the unrounded oracle."""
    lv = {n: inp[n].clone().to(dtype).requires_grad_(True) for n in LSTM_GRADS}
    forced = None if forced_out is None else forced_out.detach().cpu().to(dtype)
    out, hn, cn = O.lstm_sequence_rounded_ref(lv["x"], lv["h0"], lv["c0"], inp["lens"], lv["Wih"], lv["Whh"], lv["bih"], lv["bhh"],
                                              O.operand_rounding(mode), recurrent_rounded(arm), forced)
    (out * inp["w"].to(dtype)).sum().backward()
    return dict(out=out.detach(), h_n=hn.detach(), c_n=cn.detach(), **{"d_" + n: lv[n].grad for n in LSTM_GRADS})


def gru_oracle(inp, mode, arm, reverse, dtype=torch.float64, forced_out=None):
    """The GRU likewise; reversed: between two `reverse_sequences`, which also carry the forced values into recurrence order."""
    lv = {n: inp[n].clone().to(dtype).requires_grad_(True) for n in GRU_GRADS}
    forced = None if forced_out is None else forced_out.detach().cpu().to(dtype)
    x = lv["x"]
    if reverse:
        x = O.reverse_sequences(x, inp["lens"])
        forced = None if forced is None else O.reverse_sequences(forced, inp["lens"])
    out, hn = O.gru_sequence_rounded_ref(x, lv["h0"], lv["Wih"], lv["Whh"], lv["bih"], lv["bhh"], O.operand_rounding(mode),
                                         recurrent_rounded(arm), forced)
    if reverse:
        out = O.reverse_sequences(out, inp["lens"])
    (out * inp["w"].to(dtype)).sum().backward()
    return dict(out=out.detach(), h_n=hn.detach(), **{"d_" + n: lv[n].grad for n in GRU_GRADS})


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / (ref.norm() + 1e-30))


def row_dist(got, ref, row_dim):
    """Per batch row: |got - ref| / |ref|, [B] (a zero reference row gives 0 when got is zero there too, inf otherwise)."""
    got, ref = got.detach().double().cpu().movedim(row_dim, 0), ref.detach().double().cpu().movedim(row_dim, 0)
    d, n = (got - ref).flatten(1).norm(dim=1), ref.flatten(1).norm(dim=1)
    return torch.where(n > 0, d / n.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))


def row_dim_of(name):
    return 1 if name == "x" else 0


def loose_bar(rounded, unrounded, name):
    """LOOSE_MULTIPLE x the median over the live batch rows of the distance between the two oracles' d_<name>."""
    d = row_dist(rounded["d_" + name], unrounded["d_" + name], row_dim_of(name))
    return LOOSE_MULTIPLE * float(d[d > 0].median())


# ----------------------------------------------------------------------------------------------------------------------
# WaveNet: ONE gated block through ops.wavenet_stack, so `skip` is the block's own output and x the only input
# ----------------------------------------------------------------------------------------------------------------------

# (C, B, L, dilation, T_skip): the shapes of test_wavenet_fused_block_kernels_match_torch, one block each
WN_CASES = [(32, 3, 77, 2, 50), (64, 5, 203, 8, 120), (96, 2, 131, 1, 100)]
WN_PARAMS = ("conv_w", "conv_b", "rs_w", "rs_b")


def wn_id(c):
    return f"C{c[0]}-B{c[1]}-L{c[2]}-d{c[3]}-skip{c[4]}"


@functools.lru_cache(maxsize=None)
def wn_inputs(case, seed=0):
    C, B, L, d, T_skip = case
    g = torch.Generator().manual_seed(100000 * seed + C + L)
    return dict(x=torch.randn(L, B, C, generator=g), conv_w=torch.randn(2 * C, C, 2, generator=g) * 0.08, conv_b=torch.randn(2 * C, generator=g) * 0.1,
                rs_w=torch.randn(2 * C, C, generator=g) * 0.08, rs_b=torch.randn(2 * C, generator=g) * 0.1, w=torch.randn(T_skip, B, C, generator=g))


def wn_oracle(inp, mode, case, dtype=torch.float64):
    """-> dict(skip, d_x, d_conv_w, d_conv_b, d_rs_w, d_rs_b); the rs gradients are the skip rows [C:] only."""
    C, B, L, d, T_skip = case
    lv = {n: inp[n].clone().to(dtype).requires_grad_(True) for n in ("x",) + WN_PARAMS}
    skip = O.wavenet_block_rounded_ref(lv["x"], lv["conv_w"], lv["conv_b"], lv["rs_w"], lv["rs_b"], d, T_skip, O.operand_rounding(mode))
    (skip * inp["w"].to(dtype)).sum().backward()
    out = dict(skip=skip.detach(), **{"d_" + n: lv[n].grad for n in ("x",) + WN_PARAMS})
    out["d_rs_w"], out["d_rs_b"] = out["d_rs_w"][C:], out["d_rs_b"][C:]
    return out


WN_TILE = 64  # rows (l, b) per workgroup tile of the block kernels
WN_LOOSE_MULTIPLE = 1.5
WN_BAR_DX = 2e-5  # the tight bar of a gradient row (tests/test_gpu_rnn_sequences.py)
# per tensor, relative L2.  d_rs_b is the column sum of the upstream gradient: no product, no mode, the fp32 bar.
WN_GRAD_BAR = {"bf16": dict(x=2e-4, conv_w=2e-4, conv_b=2e-5, rs_w=2e-4, rs_b=2e-5), "f16": dict(x=1e-4, conv_w=1e-4, conv_b=2e-5, rs_w=1e-4, rs_b=2e-5)}


def two_tier(got, ref, unr, tight, multiple, group=None, rows_per_flip=1):
    """Rows (step, batch) of [T, B, *] tensors where a hidden fp32 value is rounded inside the link: a row may miss the tight bar
    when a 1e-7 difference flipped a hidden operand by a 16-bit ulp, but then it is under the loose bar, `multiple` x the median
    row distance between the rounded and the unrounded oracle, and such rows are few: at most 1/8 of all rows, at most 1/4 of
    the rows of any one group (a step; or `group` consecutive rows of the flattened [T * B] axis: the kernel's row tile, where a
    step has too few rows for a quarter of them to mean anything), at most half of the steps of any one batch row.
    rows_per_flip: how many rows ONE flipped operand moves (2 for the WaveNet block's d_x: d_pre[r] feeds d_x[r] through tap 0 and
    d_x[r + dilation * B] through tap 1); a group always has room for one flip, so a short last group does not fail by one.
    -> (failures, figures)"""
    T_, B = ref.shape[:2]
    n = T_ * B
    group = B if group is None else group
    if not bool(torch.isfinite(got).all()):
        return ["non-finite values"], dict(over=n, rows=n, share=1.0, group_share=1.0, group_fill=4.0, row_steps=T_, steps=T_, worst=float("inf"),
                                           worst_tight=float("inf"), worst_over_in_medians=float("inf"), loose=0.0)
    d = row_dist(got.reshape((n,) + tuple(got.shape[2:])), ref.reshape((n,) + tuple(ref.shape[2:])), 0)
    m = row_dist(ref.reshape(n, -1), unr.reshape(n, -1), 0)
    loose = multiple * float(m[m > 0].median())
    over = d > tight
    fails = []
    if bool((d > loose).any()):
        t, b = divmod(int(d.argmax()), B)
        fails.append(f"row (step {t}, batch row {b}): {float(d.max()):.3e} > the loose bar {loose:.3e}")
    if int(over.sum()) * 8 > n:
        fails.append(f"{int(over.sum())} of {n} rows over the tight bar {tight:.0e} (cap 1/8)")
    group_share = group_fill = 0.0
    for r0 in range(0, n, group):
        k, size = int(over[r0:r0 + group].sum()), min(group, n - r0)
        group_share = max(group_share, k / size)
        if k > rows_per_flip:
            group_fill = max(group_fill, 4 * k / size)
        if k * 4 > size and k > rows_per_flip:
            fails.append(f"rows {r0}..{r0 + size - 1}: {k} of {size} over the tight bar (cap 1/4)")
    per_row = over.reshape(T_, B).sum(0)
    if int(per_row.max()) * 2 > T_:
        fails.append(f"batch row {int(per_row.argmax())}: {int(per_row.max())} of {T_} steps over the tight bar (cap 1/2)")
    worst_over = float(d[over].max()) / (loose / multiple) if bool(over.any()) else 0.0
    fig = dict(over=int(over.sum()), rows=n, share=float(over.sum()) / n, group_share=group_share, group_fill=group_fill, row_steps=int(per_row.max()), steps=T_,
               worst=float(d.max()), worst_tight=float(d[~over].max()) if bool((~over).any()) else 0.0, worst_over_in_medians=worst_over, loose=loose)
    return fails, fig


# ----------------------------------------------------------------------------------------------------------------------
# SRNN latent chain through ops.srnn_latent_chain
# ----------------------------------------------------------------------------------------------------------------------

SRNN_R = 32
# (T', B, H, Z, z0 given, residual posterior, recurrent products rounded)
SRNN_SHAPES = [(6, 5, 32, 16), (6, 21, 64, 32), (6, 17, 48, 16), (6, 37, 128, 48)]
SRNN_CASES = [s + (z0, res, True) for s in SRNN_SHAPES for z0 in (True, False) for res in (True, False)] + [(6, 150, 32, 16, True, True, False)]
SRNN_STATS = ("zs", "mu_q", "sd_q", "mu_p", "sd_p")
BWD_T = SRNN_BWD_T = 2  # a chain's backward runs at T' = 2: the recurrent gradient link is used exactly once
SRNN_FREE_NATS, SRNN_C_RAW, SRNN_C_FN = 4.0, 0.3, 0.7  # the KL terms of the backward's loss: c_raw * kld + c_fn * kld_fn
SRNN_LOOSE_MULTIPLE = 3.2  # the stand-in's worst flipped row over seeds 0..4 of every case: 1.58 medians
# the seed of a case's inputs where it is not 0: the first for which the stand-in, in both modes, uses at most half of the caps on all
# rows and on the rows of a step and at most floor(T' / 2) - 1 steps of a batch row (asserted in test_rounded_oracle_cpu.py)
SRNN_SEED = {(6, 21, 64, 32, False, True, True): 2, (6, 37, 128, 48, True, True, True): 10, (6, 37, 128, 48, False, True, True): 2,
             (6, 37, 128, 48, False, False, True): 2}


def srnn_id(c):
    return f"T{c[0]}-B{c[1]}-H{c[2]}-Z{c[3]}-{'z0' if c[4] else 'noz0'}-{'residual' if c[5] else 'plain'}"


@functools.lru_cache(maxsize=None)
def srnn_inputs(case, seed=0, Tp=None, R=SRNN_R):
    """fp32: d, a, z0, eps of unit scale; nn.Linear-style parameters; lengths in steps (row 0 full, one row of length 1); the
    upstream gradient `w` of zs[1:]."""
    T_, B, H, Z, has_z0, _, _ = case
    Tp = T_ if Tp is None else Tp
    g = torch.Generator().manual_seed(100000 * seed + 1000 * H + 10 * B + Tp + 7 * int(has_z0))
    p = {}
    for c in ("prior", "post"):
        for n, (o, i) in (("0", (H, R + Z)), ("1", (H, H)), ("2", (H, H)), ("h", (2 * Z, H))):
            k = i ** -0.5
            p[f"{c}_{'hw' if n == 'h' else 'w' + n}"] = _uniform(g, (o, i), k)
            p[f"{c}_{'hb' if n == 'h' else 'b' + n}"] = _uniform(g, (o,), k)
    lens = torch.tensor([1 + (5 * b + 2) % Tp for b in range(B)], dtype=torch.int64)
    lens[0], lens[B - 1] = Tp, 1
    return dict(d=torch.randn(Tp, B, R, generator=g), a=torch.randn(Tp, B, R, generator=g), z0=torch.randn(B, Z, generator=g) if has_z0 else None,
                eps=torch.randn(Tp, B, Z, generator=g), w=torch.randn(Tp, B, Z, generator=g), lens=lens, **p)


def _kl_terms(out, forced, lens, dtype, stride=1, free_nats=SRNN_FREE_NATS):
    """kld, kld_fn [B] over the rows' lengths: step t of row b is live where t * stride < lens[b].  Which elements sit on the
    free-nats floor (free_nats / Z per element) is decided from the FORCED statistics where there are any (they are stored fp32 values too): max(kl, floor) has a kink, and an element within a flip of the
    floor would otherwise switch its whole gradient on or off between two evaluations."""
    Tp = out["mu_q"].shape[0]
    mask = (torch.arange(Tp).unsqueeze(1) * stride < lens.unsqueeze(0)).to(dtype).unsqueeze(-1)  # [T',B,1]
    kl = O.kl_gaussian(out["mu_q"], out["sd_q"], out["mu_p"], out["sd_p"])
    floor = free_nats / kl.shape[-1]
    decide = kl if forced is None else O.kl_gaussian(*(forced[k].detach().cpu().to(dtype) for k in ("mu_q", "sd_q", "mu_p", "sd_p")))
    kl_fn = torch.where(decide > floor, kl, torch.full_like(kl, floor))
    return (kl * mask).sum((0, 2)), (kl_fn * mask).sum((0, 2))


def srnn_oracle(inp, mode, case, dtype=torch.float64, forced_zs=None, backward=False, forced_stats=None, stride=1, free_nats=SRNN_FREE_NATS, pre_out=None,
                coef=(SRNN_C_RAW, SRNN_C_FN)):
    """-> dict over SRNN_STATS (+ kld, kld_fn [B]; with `backward`: d_d, d_a, d_z0, d_<param>) of `O.srnn_latent_rounded_ref`; the
    loss of the backward is (zs[1:] * w).sum() + (SRNN_C_RAW * kld + SRNN_C_FN * kld_fn).sum()."""
    Z, residual, rec = case[3], case[5], case[6]
    names = ("d", "a") + (("z0",) if inp["z0"] is not None else ()) + O.SRNN_CHAIN_PARAMS
    lv = {n: inp[n].clone().to(dtype).requires_grad_(backward) for n in names}
    forced = None if forced_zs is None else forced_zs.detach().cpu().to(dtype)
    res = O.srnn_latent_rounded_ref(lv["d"], lv["a"], lv.get("z0"), inp["eps"].to(dtype), lv, residual, O.operand_rounding(mode), rec, forced, pre_out=pre_out)
    out = dict(zip(SRNN_STATS, res))
    out["kld"], out["kld_fn"] = _kl_terms(out, forced_stats, inp["lens"], dtype, stride, free_nats)
    if backward:
        ((out["zs"][1:] * inp["w"].to(dtype)).sum() + (coef[0] * out["kld"] + coef[1] * out["kld_fn"]).sum()).backward()
        out.update({"d_" + n: lv[n].grad for n in names})
    return {k: v.detach() for k, v in out.items()}


def median_row_distances(got, ref, unr):
    """'The mode is on' where single rows may have flipped: the median (t, b) row distance of got to the rounded and to the unrounded
    oracle ([T, B, *] tensors).  The flipped rows, at most 1/8 of all, do not move a median."""
    n = ref.shape[0] * ref.shape[1]
    flat = lambda t: t.detach().double().cpu().reshape(n, -1)  # noqa: E731
    return float(row_dist(flat(got), flat(ref), 0).median()), float(row_dist(flat(got), flat(unr), 0).median())


# ----------------------------------------------------------------------------------------------------------------------
# VRNN sequence through ops.vrnn_sequence (forward)
# ----------------------------------------------------------------------------------------------------------------------

VRNN_X = VRNN_R = 32
# (T', B, H, Z, h0 given); residual posterior on
VRNN_CASES = [s + (h0,) for s in SRNN_SHAPES for h0 in (True, False)]
VRNN_STATS = ("mu_q", "sd_q", "mu_p", "sd_p", "z")
VRNN_LOOSE_MULTIPLE = 3.2  # the stand-in's worst flipped row over seeds 0..4 of every case: 1.25 medians
VRNN_SEED = {(6, 17, 48, 16, True): 1, (6, 37, 128, 48, True): 3}  # as SRNN_SEED


def vrnn_pieces(res, H):
    """The rows a case checks, by piece: (name, tensor [T', B, *], strict).  h_{t-1} -> z_t (statistics and sample) and z_t -> phi_t
    cross hidden activations: two tiers.  (enc_t, phi_t, h_{t-1}) -> h_t is one product deep from stored values: strict."""
    return [(k, res[k], False) for k in VRNN_STATS] + [("phi", res["decin"][:-1, :, :H], False), ("h", res["decin"][1:, :, H:], True)]


def vrnn_id(c):
    return f"T{c[0]}-B{c[1]}-H{c[2]}-Z{c[3]}-{'h0' if c[4] else 'noh0'}"


@functools.lru_cache(maxsize=None)
def vrnn_inputs(case, seed=0, Tp=None, X=VRNN_X, R=VRNN_R):
    T_, B, H, Z, has_h0 = case
    Tp = T_ if Tp is None else Tp
    g = torch.Generator().manual_seed(100000 * seed + 1000 * H + 10 * B + Tp + 3 * int(has_h0) + 1)
    shapes = dict(prior_w0=(H, R), prior_w1=(H, H), prior_w2=(H, H), prior_hw=(2 * Z, H), post_w0=(H, R + X), post_w1=(H, H), post_w2=(H, H), post_hw=(2 * Z, H),
                  phi_w0=(H, Z), phi_w1=(H, H), phi_w2=(H, H), phi_w3=(H, H), gru_wih=(3 * R, X + H), gru_whh=(3 * R, R))
    p = {}
    for n in O.VRNN_SEQ_PARAMS:
        wn = n if n in shapes else {"gru_bih": "gru_wih", "gru_bhh": "gru_whh"}.get(n, n.replace("_b", "_w").replace("_hb", "_hw"))
        o, i = shapes[wn]
        k = (R if n.startswith("gru") else i) ** -0.5
        p[n] = _uniform(g, (o, i) if n in shapes else (o,), k)
    inp = dict(enc=torch.randn(Tp, B, X, generator=g), h0=torch.randn(B, R, generator=g) if has_h0 else None, eps=torch.randn(Tp, B, Z, generator=g), **p)
    inp["w"] = torch.randn(Tp + 1, B, H + R, generator=g)  # the upstream gradient of decin (a backward case)
    inp["w"][Tp] = 0  # include/blvm_hip.h: row T' of d_decin is ignored (it only carries h_n out)
    inp["lens"] = torch.tensor([1 + (5 * b + 2) % Tp for b in range(B)], dtype=torch.int64)
    inp["lens"][0], inp["lens"][B - 1] = Tp, 1
    return inp


def vrnn_oracle(inp, mode, case, dtype=torch.float64, forced=None, backward=False, residual=True, stride=1, free_nats=SRNN_FREE_NATS, forced_stats=None,
                kl=False, pre_out=None, coef=(SRNN_C_RAW, SRNN_C_FN)):
    """-> dict(decin, mu_q, sd_q, mu_p, sd_p, z) of `O.vrnn_sequence_rounded_ref`; forced: dict(decin, z), the kernel's stores.
    backward: also kld, kld_fn [B] over the rows' lengths (stride 1) and d_enc, d_h0, d_<param> of the loss
    (decin * w).sum() + (SRNN_C_RAW * kld + SRNN_C_FN * kld_fn).sum().
    residual: the posterior's mean is added to the prior's.  kl: kld, kld_fn also without `backward`.  forced_stats: a result dict whose
    statistics decide the free-nats branch (`_kl_terms`) where nothing is teacher forced (default: `forced`)."""
    names = ("enc",) + (("h0",) if inp["h0"] is not None else ()) + O.VRNN_SEQ_PARAMS
    lv = {n: inp[n].clone().to(dtype).requires_grad_(backward) for n in names}
    f = None if forced is None else {k: forced[k].detach().cpu().to(dtype) for k in ("decin", "z")}
    with torch.set_grad_enabled(backward):
        res = O.vrnn_sequence_rounded_ref(lv["enc"], lv.get("h0"), inp["eps"].to(dtype), lv, residual, O.operand_rounding(mode), True, f, pre_out=pre_out)
        out = dict(zip(("decin",) + VRNN_STATS, res))
        if backward or kl:
            out["kld"], out["kld_fn"] = _kl_terms(out, forced if forced_stats is None else forced_stats, inp["lens"], dtype, stride, free_nats)
        if backward:
            ((out["decin"] * inp["w"].to(dtype)).sum() + (coef[0] * out["kld"] + coef[1] * out["kld_fn"]).sum()).backward()
            out.update({"d_" + n: lv[n].grad for n in names})
    return {k: v.detach() for k, v in out.items()}


# ----------------------------------------------------------------------------------------------------------------------
# the backward of the two chains, T' = BWD_T, every variant of the forward cases
# ----------------------------------------------------------------------------------------------------------------------

FP32_GRAD_BAR = 2e-5  # tests/test_gpu_rnn_sequences.py: no gradient bar is below the project's fp32 one
# Batch rows of an input's gradient: every row is under BWD_LOOSE_MULTIPLE median row distances between the rounded and the unrounded
# oracle, at least twice the stand-in's worst row (1.72).
BWD_LOOSE_MULTIPLE = 3.6
BWD_ROW_GRADS = {"srnn": (("d", 1), ("a", 1), ("z0", 0)), "vrnn": (("enc", 1), ("h0", 0))}  # (input, its batch-row axis)
# Every variant of the forward cases, and the same widths at a larger batch (SRNN: + 64 rows, still one persistent launch; VRNN: up
# to 61, the row tiles of B <= 64), where one flipped operand weighs less against the mode's distance and more tensors have a bar.
SRNN_BWD_WIDE = [(6, 69, 32, 16), (6, 85, 64, 32), (6, 81, 48, 16), (6, 101, 128, 48)]
VRNN_BWD_WIDE = [(6, 53, 32, 16), (6, 61, 64, 32), (6, 49, 48, 16), (6, 61, 128, 48)]
BWD_CASES = ([("srnn", c) for c in SRNN_CASES] + [("srnn", s + (z0, res, True)) for s in SRNN_BWD_WIDE for z0 in (True, False) for res in (True, False)]
             + [("vrnn", c) for c in VRNN_CASES] + [("vrnn", s + (h0,)) for s in VRNN_BWD_WIDE for h0 in (True, False)])


def bwd_id(fc):
    return f"{fc[0]}-{(srnn_id if fc[0] == 'srnn' else vrnn_id)(fc[1])}"


KINK = 2e-5  # what ONE flipped fp16 operand moves a hidden pre-activation by: 2^-11 relative of a term |x| |w| of about 0.4 x 0.1


@functools.lru_cache(maxsize=None)
def bwd_inputs(family, case, seed=0, kink=KINK):
    """The inputs at T' = BWD_T.  A batch row in which a hidden pre-activation lies within KINK of zero (float64, either mode)
    carries no loss: its upstream gradient is zero and its length 0.  One flipped operand puts such a unit on the other branch of its
    (Leaky)ReLU, the kernel's saved activation and the oracle's then disagree about the derivative (1 against 0.01 or 0), and the
    gradient of that row, with every weight gradient it feeds, moves by percents: no reference exists for it at the mode's precision.
    The forward of such a row is compared like any other.  These are 15 % of all rows (366 of 2422), up to 28 of 61 in a case at
    H = 128; test_rounded_oracle_cpu.py caps the share.  KINK is the reach of an fp16 flip in both modes: a bf16 flip reaches 8 times
    further but is 8 times rarer, and its reach would cover most rows of every case."""
    base = (srnn_inputs if family == "srnn" else vrnn_inputs)(case, seed, BWD_T)
    inp = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in base.items()}
    near = torch.zeros(case[1], dtype=torch.bool)
    for mode in MODES:
        pre = []
        lv = {n: v.double() for n, v in inp.items() if isinstance(v, torch.Tensor)}
        with torch.no_grad():
            if family == "srnn":
                O.srnn_latent_rounded_ref(lv["d"], lv["a"], lv.get("z0"), lv["eps"], lv, case[5], O.operand_rounding(mode), case[6], pre_out=pre)
            else:
                O.vrnn_sequence_rounded_ref(lv["enc"], lv.get("h0"), lv["eps"], lv, True, O.operand_rounding(mode), True, pre_out=pre)
        near |= torch.stack([p.abs().min(1).values for p in pre]).min(0).values < kink
    inp["w"][:, near] = 0
    inp["lens"][near] = 0
    inp["near_kink"] = near
    return inp


def bwd_oracle(family, inp, mode, case, dtype=torch.float64, forced=None):
    """forced: the kernel's (or the stand-in's) own result dict; the SRNN takes its zs, the VRNN its decin and z."""
    if family == "srnn":
        return srnn_oracle(inp, mode, case, dtype, None if forced is None else forced["zs"], backward=True, forced_stats=forced)
    return vrnn_oracle(inp, mode, case, dtype, forced, backward=True)


def _variants(family, case):
    """The cases that share `case`'s shape and arm: with / without the initial state, with / without the residual posterior."""
    return [c for f, c in BWD_CASES if f == family and c[:4] == case[:4]]


@functools.lru_cache(maxsize=None)
def bwd_standin(family, case, mode):
    """Over STANDIN_SEEDS seeds of `case` at T' = BWD_T, the float32 stand-in against the forced float64 oracle: per gradient the
    largest distance (floor), the smallest distance between the rounded and the unrounded oracle (mode), and the worst batch row
    of an input's gradient in median row distances between the two oracles.  One thread: the float32 sums in one fixed order."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        floor, dist, worst = {}, {}, 0.0
        for seed in range(STANDIN_SEEDS):
            inp = bwd_inputs(family, case, seed)
            stand = bwd_oracle(family, inp, mode, case, torch.float32)
            ref, unr = bwd_oracle(family, inp, mode, case, forced=stand), bwd_oracle(family, inp, "f32", case)
            for k in ref:
                if k.startswith("d_"):
                    floor[k[2:]] = max(floor.get(k[2:], 0.0), rel_l2(stand[k], ref[k]))
                    dist[k[2:]] = min(dist.get(k[2:], float("inf")), rel_l2(ref[k], unr[k]))
            for n, dim in BWD_ROW_GRADS[family]:
                if "d_" + n in ref:
                    m = row_dist(ref["d_" + n], unr["d_" + n], dim)
                    worst = max(worst, float(row_dist(stand["d_" + n], ref["d_" + n], dim).max()) / float(m[m > 0].median()))
        return floor, dist, worst
    finally:
        torch.set_num_threads(threads)


def one_flip(case, mode):
    """What ONE flipped operand may move a gradient by, relative L2: half a 16-bit ulp relative (2^-8 bf16, 2^-11 fp16) of an element
    of 4 standard deviations in the smallest matrix the chain rounds, [T' * B rows, min(H, Z, R) columns].  bf16 flips are rare (one
    rounded element in 40 000 has a 1e-7 neighbour across a rounding point), so the stand-in's runs need not have met one in
    every tensor, while each is 8 times an fp16 one: without this term a bar would sit under the first flip a kernel meets."""
    rows, width = BWD_T * case[1], min(case[2], case[3], SRNN_R)
    return {"bf16": 2.0**-8, "f16": 2.0**-11}[mode] * 4 / (rows * width) ** 0.5


def bwd_grad_names(family, case):
    if family == "srnn":
        return ("d", "a") + (("z0",) if case[4] else ()) + O.SRNN_CHAIN_PARAMS
    return ("enc",) + (("h0",) if case[4] else ()) + O.VRNN_SEQ_PARAMS


def _round_up(v):
    """to two significant digits, upwards"""
    e = math.floor(math.log10(v)) - 1
    return round(math.ceil(v / 10.0**e - 1e-9) * 10.0**e, 12)


def measure_bwd_bars(family, case, mode):
    """-> {tensor: bar} as measured on this host.  A bar is 3.3 x the larger of `one_flip` and the stand-in's floor (the floor pooled
    over the variants of the case's shape: 4 x STANDIN_SEEDS runs for the SRNN, 2 x for the VRNN), not below the fp32 bar, rounded
    up to two digits.  It must not exceed half of the case's own mode distance (float64 on every host); a tensor for which it
    would has no bar.  3.3 and not 3: room for the float32 sums of another host, on which the recorded table must still be 3 x the
    floor measured there."""
    pooled = {}
    for c in _variants(family, case):
        for n, v in bwd_standin(family, c, mode)[0].items():
            pooled[n] = max(pooled.get(n, 0.0), v)
    dist = bwd_standin(family, case, mode)[1]
    bars = {n: _round_up(max(3.3 * pooled[n], 3.3 * one_flip(case, mode), FP32_GRAD_BAR)) for n in dist}
    return {n: b for n, b in bars.items() if b <= dist[n] / 2}


BWD_BARS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "links16_bwd_bars.json")


@functools.lru_cache(maxsize=None)
def _frozen_bars():
    with open(BWD_BARS_FILE) as f:
        return json.load(f)


def bwd_bars(family, case, mode):
    """-> ({tensor: bar}, [tensors without a bar]): the recorded table tests/golden/links16_bwd_bars.json, the same on every host
    (written by `python tests/links16.py`, i.e. `measure_bwd_bars` for every case; test_rounded_oracle_cpu.py holds every entry
    between 3 x the stand-in's floor and half the mode's distance where it runs).  A tensor without a bar is not compared, only
    required to be finite: a bound that the mode itself could miss by rounding luck pins nothing."""
    bars = _frozen_bars()[f"{bwd_id((family, case))}|{mode}"]
    return dict(bars), sorted(n for n in bwd_grad_names(family, case) if n not in bars)


def bwd_rows(family, got, ref, unr):
    """-> (failures, worst row in medians): every batch row of the inputs' gradients is under BWD_LOOSE_MULTIPLE."""
    fails, worst = [], 0.0
    for n, dim in BWD_ROW_GRADS[family]:
        if "d_" + n not in ref:
            continue
        m = row_dist(ref["d_" + n], unr["d_" + n], dim)
        d = row_dist(got["d_" + n], ref["d_" + n], dim) / float(m[m > 0].median())
        if not bool(torch.isfinite(d).all()):
            fails.append(f"d_{n}: non-finite rows or rows where the reference is zero")
            continue
        worst = max(worst, float(d.max()))
        if float(d.max()) > BWD_LOOSE_MULTIPLE:
            fails.append(f"d_{n} row {int(d.argmax())}: {float(d.max()):.2f} medians > {BWD_LOOSE_MULTIPLE}")
    return fails, worst


if __name__ == "__main__":  # record the backward bars
    table = {f"{bwd_id(fc)}|{mode}": measure_bwd_bars(fc[0], fc[1], mode) for fc in BWD_CASES for mode in MODES}
    with open(BWD_BARS_FILE, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
    print({mode: sum(len(v) for k, v in table.items() if k.endswith("|" + mode)) for mode in MODES}, "tensors with a bar of",
          {mode: sum(len(bwd_grad_names(*fc)) for fc in BWD_CASES) for mode in MODES})
