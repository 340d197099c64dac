"""The kernels with a 16-bit instantiation other than K6, link by link against float64 in both operand modes: the LSTM (K4) and GRU
(K2) sequence kernels on every arm, the WaveNet block kernels (K10), the SRNN latent chain (K3) and the VRNN step program (K1) on the
persistent-chain engine's 16-bit tiles.

The contract of a 16-bit mode: the operands of matrix products are rounded to bf16 / fp16, nearest even, once;
accumulation, epilogues and everything stored stay fp32.  `blvm_oracle.rounded_linear` states it for one product; the per-kernel
oracles (`lstm_sequence_rounded_ref`, `gru_sequence_rounded_ref`, `wavenet_block_rounded_ref`, `srnn_latent_rounded_ref`,
`vrnn_sequence_rounded_ref`) are explicit time loops built from it.  A free-running rounded oracle disagrees with itself (a 1e-7
difference upstream of a rounding point flips the operand by a whole 16-bit ulp), so the oracles are TEACHER FORCED: the input of
each link is the kernel's own stored fp32 value (out, zs, decin, z: same bits in, same bits out of the rounding) and only that link
is computed in float64; autograd stays connected (`forced + (own - own.detach())`), so the backward is the oracle's.

Which products are rounded, from the code: hoisted GEMMs, data gradients to the inputs and weight gradients in every arm (`gemm_f32`
follows the mode; the bias sums are fp32 sums of the unrounded gradient); the products inside a step where `pchain_optype(B)` /
`seq_ot` is 16-bit, i.e. on the persistent arms, not with one launch per step or per link (B > 128, T < 4).  The LSTM / GRU arm is
asserted with `blvm_rnn_path_counts`.

Cases, inputs, oracles' wrappers and bars: tests/links16.py.  Where the bars come from (the float32 "stand-in": the same oracle run
free in float32 in the kernel's place, 5 seeds): tests/test_rounded_oracle_cpu.py, which asserts every condition named here.

  * One product deep (LSTM / GRU steps from out[t-1]; the VRNN's GRU cell from decin): EVERY (t, b) row, and every batch row of
    h_n / c_n, at the project's fp32 bar, relative L2 <= 1e-5 (stand-in <= 1.8e-7); a row past its length is exactly zero.
  * Several links deep (an SRNN step z[t-1] -> z[t]; the VRNN's h[t-1] -> z[t] and z[t] -> phi[t]; the WaveNet block, whose gate
    output is rounded unseen): two tiers.  A row over 1e-5 (2e-5 for the WaveNet's d_x) is under the loose bar, a multiple of the
    case's median row distance between the rounded and the unrounded oracle: 3.2 (SRNN, VRNN; the stand-in's worst flipped row is
    1.58 / 1.25 medians) and 1.5 (WaveNet; 0.64).  Such rows are at most 1/8 of all, at most 1/4 of a step's rows (a step always
    has room for one flip), at most half of the steps of a batch row.  The WaveNet's steps hold 2 to 5 rows, so its unit is the
    kernels' 64-row tile instead, and one flipped operand of d_pre[r] moves the TWO d_x rows r and r + dilation * B (counted as
    one).  The inputs' seeds are the first for which the stand-in uses at most half of the first two caps and at most
    floor(T' / 2) - 1 steps of a batch row.
  * Gradients, per tensor: at least 3 x the stand-in's largest float32-vs-float64 distance and at most half the smallest distance
    between the rounded and the unrounded oracle.  LSTM / GRU (`links16.grad_bar`): bf16 5e-4 (d_x, d_h0, d_Wih, d_Whh) and 1e-4
    (d_c0, biases) on the persistent arms, 2e-4 and 2e-5 with one launch per step; fp16 1.2e-4 (GRU d_h0 6e-5), 3e-5 (d_c0), 2e-5
    (biases), and 6e-5 / 1e-5 per step.  WaveNet: 2e-4 (bf16) / 1e-4 (fp16), d_conv_b 2e-5; d_rs_b is a column sum of the
    upstream gradient, no product: the fp32 bar 2e-5.
  * The backward of the two chains (SRNN chain, VRNN step program) at T' = 2, so that the recurrent gradient link runs exactly once;
    the loss carries an upstream gradient of every stored row and both KL terms with free nats; every variant of the forward cases,
    and the same widths at a larger batch (SRNN B + 64, VRNN B up to 61).  Per tensor (`links16.bwd_bars`, the recorded table
    tests/golden/links16_bwd_bars.json, the same on every host): 3.3 x the larger of the stand-in's floor, pooled over the variants
    of the shape, and of what ONE flipped operand moves a gradient by (`one_flip`), not below the fp32 bar 2e-5, and at most half
    the mode's distance.  A tensor for which that window is empty has no bar and is only required to be finite: all tensors at
    B = 5 (10 rows: one flip is a third of the mode's distance), most at B = 17 to 37 in fp16, few at the larger batches in bf16;
    735 (bf16) and 392 (fp16) of 1083 tensors have one.  EVERY batch row of d_d, d_a, d_z0 / d_enc, d_h0 is under 3.6 medians of
    the mode's row distance (the stand-in's worst: 1.72).  A batch row with a hidden pre-activation within 2e-5 of zero, the reach
    of one flipped fp16 operand, carries no loss (`links16.bwd_inputs`): that flip puts the unit on the other branch of its
    (Leaky)ReLU and the row's gradient moves by percents, so no reference exists for it at the mode's precision.  These are 366 of
    the 2422 rows (15 %), at most 28 of a case's 61, never a whole row tile.
    LSTM / GRU: every batch row of d_x / d_h0 / d_c0 under 1.25 medians.
  * The mode is on: the output (its median row where rows may flip) is 10 times closer to the rounded than to the unrounded oracle.
  * No persistent launch gave up on a spin.

Measured on an MI355X, worst over a family's cases, bf16 / fp16:
  LSTM     out rows 1.5e-7 / 1.4e-7; gradients at 0.08 / 0.25 of their bar; batch rows at 0.05 / 0.37 of the loose bar
  GRU      out rows 8.7e-8 / 9.3e-8; gradients at 0.16 / 0.32; batch rows at 0.13 / 0.40
  WaveNet  rows over the tight bar 0.8 % / 3.1 %, worst of them 0.21 / 0.31 medians; gradients at 0.13 / 0.10 of their bar
  SRNN     rows over the tight bar 1.4 % / 4.1 %, worst 0.73 / 1.09 medians, at most 3 of 6 steps of a batch row
  VRNN     h rows 1.2e-7 / 1.3e-7; z / phi rows over the tight bar 0.5 % / 3.6 %, worst 0.43 / 0.97 medians
  chain backward: see DESIGN §3f
The pins bite.  With rnd replaced by the identity in ONE product of an oracle (input projection; recurrent product; only its weight
gradient; only its data gradient) all 26 LSTM / GRU cases fail on the GPU; with bf16 truncation in place of rounding, the 13 bf16
ones.  With the float32 stand-in as the kernel: every single-product weakening of the WaveNet, SRNN and VRNN forward fails every case
in both modes; in the chain backward, data gradients of the in-step products unrounded: all cases with a bar but one per mode
(SRNN) fail; only their weight gradients unrounded: all but 1 (bf16) / 2 (fp16) SRNN cases and one VRNN case; only the recurrent
link's data gradient unrounded: all VRNN cases, 20 of 29 SRNN cases in bf16 and 3 of 28 in fp16 (there that one product is a small
share of a gradient's mode distance).
"""
import math

import pytest
import torch

import blvm_oracle as O
import links16 as L
from blvm import _hip, ops
from test_gpu_rnn_sequences import GRU_BWD, GRU_FWD, LSTM_BWD, LSTM_FWD, Checks, expect_path

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(params=L.MODES)
def mode(request):
    """The operand mode with the engine on; the mode and `blvm_pchain_configure` restored afterwards."""
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    lib = _hip.load()
    assert lib.blvm_device_ok() == 1, "libblvm_hip: no gfx950 device visible"
    before = lib.blvm_pchain_max_batch()
    lib.blvm_pchain_configure(128, 0)
    _hip.set_operand_dtype(request.param)
    try:
        yield request.param
    finally:
        _hip.set_operand_dtype("f32")
        lib.blvm_pchain_configure(before, 0)


def _check(ck, family, mode, arm, T_, B, got, grads, ref, unr, names):
    ck.close("out", got["out"].reshape(T_ * B, -1), ref["out"].reshape(T_ * B, -1), L.BAR_VALUE, row_dim=0)
    for n in ("h_n", "c_n"):
        if n in got:
            ck.close(n, got[n], ref[n], L.BAR_VALUE, row_dim=0)
    share = 0.0
    for n in names:
        bar = L.grad_bar(family, mode, arm, n)
        ck.close("d_" + n, grads[n], ref["d_" + n], bar)
        share = max(share, L.rel_l2(grads[n], ref["d_" + n]) / bar)
    row_share = 0.0
    for n in names:
        if n in L.ROW_GRADS:
            loose = L.loose_bar(ref, unr, n)
            d = L.row_dist(grads[n], ref["d_" + n], L.row_dim_of(n))
            k = int(d.argmax())
            row_share = max(row_share, float(d[k]) / loose)
            print(f"{ck.tag} d_{n} rows: worst row {k}: {float(d[k]):.3e} (loose bar {loose:.3e})")
            if float(d[k]) > loose:
                ck.failures.append(f"d_{n} row {k}: {float(d[k]):.3e} > the loose bar {loose:.3e}")
    e_r, e_u = L.rel_l2(got["out"], ref["out"]), L.rel_l2(got["out"], unr["out"])
    print(f"{ck.tag} summary: out vs rounded {e_r:.3e}, vs unrounded {e_u:.3e}; gradients at {share:.2f} of their bar; rows at {row_share:.2f} of the loose bar")
    if not L.MODE_ON * e_r <= e_u:
        ck.failures.append(f"mode not on: out is {e_r:.3e} from the rounded oracle, {e_u:.3e} from the unrounded one")
    ck.done()


@pytest.mark.parametrize("case", L.LSTM_CASES, ids=L.lstm_id)
def test_lstm_links(case, mode):
    T_, B, I, H, arm = case
    inp = L.lstm_inputs(case)
    tag = f"lstm {L.lstm_id(case)} [{mode}]"
    dev = {n: inp[n].to(DEV).requires_grad_(True) for n in L.LSTM_GRADS}
    _hip.take_async_errors()
    with expect_path(LSTM_FWD, arm, tag + " forward"):
        out, hn, cn = ops.lstm_sequence(dev["x"], dev["h0"], dev["c0"], inp["lens"].to(DEV, torch.int32), dev["Wih"], dev["Whh"], dev["bih"], dev["bhh"])
    with expect_path(LSTM_BWD, arm, tag + " backward"):
        (out * inp["w"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    ref = L.lstm_oracle(inp, mode, arm, forced_out=out)
    unr = L.lstm_oracle(inp, "f32", arm)
    _check(Checks(tag), "lstm", mode, arm, T_, B, dict(out=out, h_n=hn, c_n=cn), {n: dev[n].grad for n in L.LSTM_GRADS}, ref, unr, L.LSTM_GRADS)


@pytest.mark.parametrize("case", L.GRU_CASES, ids=L.gru_id)
def test_gru_links(case, mode):
    T_, B, I, R, arm, reverse = case
    inp = L.gru_inputs(case)
    tag = f"gru {L.gru_id(case)} [{mode}]"
    dev = {n: inp[n].to(DEV).requires_grad_(True) for n in L.GRU_GRADS}
    lens_dev = inp["lens"].to(DEV, torch.int32) if reverse else None
    _hip.take_async_errors()
    with expect_path(GRU_FWD, arm, tag + " forward"):
        out, hn = ops.gru_sequence(dev["x"], dev["h0"], dev["Wih"], dev["Whh"], dev["bih"], dev["bhh"], lens_dev, reverse)
    with expect_path(GRU_BWD, arm, tag + " backward"):
        (out * inp["w"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    ref = L.gru_oracle(inp, mode, arm, reverse, forced_out=out)
    unr = L.gru_oracle(inp, "f32", arm, reverse)
    _check(Checks(tag), "gru", mode, arm, T_, B, dict(out=out, h_n=hn), {n: dev[n].grad for n in L.GRU_GRADS}, ref, unr, L.GRU_GRADS)


@pytest.mark.parametrize("npw", [None, "1", "whole"], ids=["npw_default", "npw_1", "npw_whole"])
@pytest.mark.parametrize("case", L.WN_CASES, ids=L.wn_id)
def test_wavenet_block_links(case, npw, mode, monkeypatch):
    """ONE gated block through `ops.wavenet_stack` (the fused forward kernel, backward A and B, the tall-skinny weight-gradient kernel
    in each of its column-tile forms), so `skip` is the block's own output and x the only input."""
    C, B, L_, d, T_skip = case
    if npw is not None:
        monkeypatch.setenv("BLVM_WN_WGRAD_NPW", "1" if npw == "1" else str(C // 16))
    inp = L.wn_inputs(case)
    tag = f"wavenet {L.wn_id(case)} {npw or 'default'} [{mode}]"
    dev = {n: inp[n].to(DEV).requires_grad_(True) for n in ("x",) + L.WN_PARAMS}
    _hip.take_async_errors()
    skip = ops.wavenet_stack(dev["x"], [tuple(dev[n] for n in L.WN_PARAMS)], [d], T_skip, math.sqrt(0.5), C)
    (skip * inp["w"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    ref, unr = L.wn_oracle(inp, mode, case), L.wn_oracle(inp, "f32", case)
    ck = Checks(tag)
    grads = {n: dev[n].grad for n in ("x",) + L.WN_PARAMS}
    grads["rs_w"], grads["rs_b"] = grads["rs_w"][C:], grads["rs_b"][C:]  # a single block's residual rows reach no output
    for name, got, tight in (("skip", skip, L.BAR_VALUE), ("d_x", grads["x"], L.WN_BAR_DX)):
        fails, fig = L.two_tier(got, ref[name], unr[name], tight, L.WN_LOOSE_MULTIPLE, L.WN_TILE, 2 if name == "d_x" else 1)
        print(f"{tag} {name} rows: {fig['over']} of {fig['rows']} over the tight bar {tight:.0e} (worst tile {fig['group_share']:.3f}, worst batch row {fig['row_steps']} of "
              f"{fig['steps']} steps), worst row under it {fig['worst_tight']:.3e}, worst row {fig['worst']:.3e} = {fig['worst_over_in_medians']:.2f} medians (loose bar {fig['loose']:.3e})")
        ck.failures += [f"{name} {f}" for f in fails]
    share = 0.0
    for n in ("x",) + L.WN_PARAMS:
        bar = L.WN_GRAD_BAR[mode][n]
        ck.close("d_" + n, grads[n], ref["d_" + n], bar)
        share = max(share, L.rel_l2(grads[n], ref["d_" + n]) / bar)
    e_r, e_u = L.rel_l2(skip, ref["skip"]), L.rel_l2(skip, unr["skip"])
    print(f"{tag} summary: skip vs rounded {e_r:.3e}, vs unrounded {e_u:.3e}; gradients at {share:.2f} of their bar")
    if not L.MODE_ON * e_r <= e_u:
        ck.failures.append(f"mode not on: skip is {e_r:.3e} from the rounded oracle, {e_u:.3e} from the unrounded one")
    ck.done()


@pytest.mark.parametrize("case", L.SRNN_CASES, ids=L.srnn_id)
def test_srnn_chain_forward_links(case, mode):
    """The SRNN latent chain (the persistent chain engine's 16-bit tiles: first layers on z, two more layers, both heads; B = 150:
    one launch per link, fp32 inside the step) one step at a time: the z that enters step t is the kernel's own zs[t], and the
    rows (t, b) of zs, mu_q, sd_q, mu_p, sd_p follow the two-tier rule (the activations between the layers are hidden)."""
    Tp, B, H, Z = case[:4]
    inp = L.srnn_inputs(case, L.SRNN_SEED.get(case, 0))
    tag = f"srnn {L.srnn_id(case)} [{mode}]"
    dev = {n: (inp[n].to(DEV) if inp[n] is not None else None) for n in ("d", "a", "z0", "eps")}
    params = [inp[n].to(DEV) for n in O.SRNN_CHAIN_PARAMS]
    _hip.take_async_errors()
    got = ops.srnn_latent_chain(dev["d"], dev["a"], dev["z0"], dev["eps"], inp["lens"].to(DEV, torch.int32), params, H, Z, L.SRNN_R, case[5], 1, L.SRNN_FREE_NATS)
    torch.cuda.synchronize()
    got = dict(zip(("zs", "kld", "kld_fn", "mu_q", "sd_q", "mu_p", "sd_p"), got))
    ref, unr = L.srnn_oracle(inp, mode, case, forced_zs=got["zs"]), L.srnn_oracle(inp, "f32", case)
    ck = Checks(tag)
    ck.exact("zs[0] is z0", torch.equal(got["zs"][0].cpu(), inp["z0"] if inp["z0"] is not None else torch.zeros(B, Z)))
    for name in L.SRNN_STATS:
        g, r, u = (x[name][1:] if name == "zs" else x[name] for x in (got, ref, unr))
        fails, fig = L.two_tier(g, r, u, L.BAR_VALUE, L.SRNN_LOOSE_MULTIPLE)
        print(f"{tag} {name} rows: {fig['over']} of {fig['rows']} over the tight bar (worst step {fig['group_share']:.3f}, worst batch row {fig['row_steps']} of {fig['steps']} steps), "
              f"worst row under it {fig['worst_tight']:.3e}, worst row {fig['worst']:.3e} = {fig['worst_over_in_medians']:.2f} medians (loose bar {fig['loose']:.3e})")
        ck.failures += [f"{name} {f}" for f in fails]
    e_r, e_u = L.median_row_distances(got["zs"][1:], ref["zs"][1:], unr["zs"][1:])
    print(f"{tag} summary: median row of zs vs rounded {e_r:.3e}, vs unrounded {e_u:.3e}")
    if not L.MODE_ON * e_r <= e_u:
        ck.failures.append(f"mode not on: the median row of zs is {e_r:.3e} from the rounded oracle, {e_u:.3e} from the unrounded one")
    ck.done()


@pytest.mark.parametrize("fc", L.BWD_CASES, ids=L.bwd_id)
def test_chain_backward_links(fc, mode):
    """The backward programs of the SRNN chain and the VRNN step at T' = 2 (the recurrent gradient link runs exactly once), the loss
    carrying an upstream gradient of every stored row and both KL terms with free nats.  Forward values are forced; the backward is
    the oracle's own.  Per tensor `links16.bwd_bars`; the batch rows of d_d, d_a, d_z0 / d_enc, d_h0 by `links16.bwd_rows`."""
    family, case = fc
    B, H, Z = case[1:4]
    inp = L.bwd_inputs(family, case)
    tag = f"{L.bwd_id(fc)} backward [{mode}]"
    lens = inp["lens"].to(DEV, torch.int32)
    _hip.take_async_errors()
    if family == "srnn":
        names = ("d", "a") + (("z0",) if inp["z0"] is not None else ()) + O.SRNN_CHAIN_PARAMS
        dev = {n: inp[n].to(DEV).requires_grad_(True) for n in names}
        res = ops.srnn_latent_chain(dev["d"], dev["a"], dev.get("z0"), inp["eps"].to(DEV), lens, [dev[n] for n in O.SRNN_CHAIN_PARAMS], H, Z, L.SRNN_R, case[5], 1, L.SRNN_FREE_NATS)
        got = dict(zip(("zs", "kld", "kld_fn", "mu_q", "sd_q", "mu_p", "sd_p"), res))
        out, rows = got["zs"][1:], ("zs", slice(1, None))
    else:
        names = ("enc",) + (("h0",) if inp["h0"] is not None else ()) + O.VRNN_SEQ_PARAMS
        dev = {n: inp[n].to(DEV).requires_grad_(True) for n in names}
        res = ops.vrnn_sequence(dev["enc"], dev.get("h0"), inp["eps"].to(DEV), lens, [dev[n] for n in O.VRNN_SEQ_PARAMS], L.VRNN_X, H, Z, L.VRNN_R, True, 1, L.SRNN_FREE_NATS)
        got = dict(zip(("decin", "kld", "kld_fn") + L.VRNN_STATS, res))
        out, rows = got["decin"], ("decin", slice(1, None))
    ((out * inp["w"].to(DEV)).sum() + (L.SRNN_C_RAW * got["kld"] + L.SRNN_C_FN * got["kld_fn"]).sum()).backward()
    torch.cuda.synchronize()
    got.update({"d_" + n: dev[n].grad for n in names})
    ref, unr = L.bwd_oracle(family, inp, mode, case, forced=got), L.bwd_oracle(family, inp, "f32", case)
    bars, without = L.bwd_bars(family, case, mode)
    ck = Checks(tag)
    share = 0.0
    for n in names:
        if n in bars:
            ck.close("d_" + n, got["d_" + n], ref["d_" + n], bars[n])
            share = max(share, L.rel_l2(got["d_" + n], ref["d_" + n]) / bars[n])
        elif not bool(torch.isfinite(got["d_" + n]).all()):
            ck.failures.append(f"d_{n}: non-finite values")
    fails, worst = L.bwd_rows(family, got, ref, unr)
    ck.failures += fails
    k, sl = rows
    h_part = (lambda t: t[..., H:]) if family == "vrnn" else (lambda t: t)
    e_r, e_u = L.median_row_distances(h_part(got[k][sl]), h_part(ref[k][sl]), h_part(unr[k][sl]))
    print(f"{tag} summary: {len(bars)} gradients at {share:.2f} of their bar ({len(without)} without a bar: {' '.join(without)}); worst batch row {worst:.2f} medians; "
          f"median row of {k} vs rounded {e_r:.3e}, vs unrounded {e_u:.3e}")
    if not L.MODE_ON * e_r <= e_u:
        ck.failures.append(f"mode not on: the median row of {k} is {e_r:.3e} from the rounded oracle, {e_u:.3e} from the unrounded one")
    ck.done()


@pytest.mark.parametrize("case", L.VRNN_CASES, ids=L.vrnn_id)
def test_vrnn_sequence_forward_links(case, mode):
    """The VRNN step program (prior / posterior runs, heads, the phi_z run, hidden projection and GRU link) in three separately
    forced pieces per step, each from the kernel's own stores: h[t-1] -> z[t] and z[t] -> phi[t] cross hidden activations (two
    tiers); (enc[t], phi[t], h[t-1]) -> h[t] is one product deep: every row under the tight bar."""
    Tp, B, H, Z, _ = case
    inp = L.vrnn_inputs(case, L.VRNN_SEED.get(case, 0))
    tag = f"vrnn {L.vrnn_id(case)} [{mode}]"
    h0 = inp["h0"].to(DEV) if inp["h0"] is not None else None
    lens = torch.full((B,), Tp, dtype=torch.int32, device=DEV)
    _hip.take_async_errors()
    res = ops.vrnn_sequence(inp["enc"].to(DEV), h0, inp["eps"].to(DEV), lens, [inp[n].to(DEV) for n in O.VRNN_SEQ_PARAMS], L.VRNN_X, H, Z, L.VRNN_R, True, 1)
    torch.cuda.synchronize()
    got = dict(zip(("decin", "kld", "kld_fn") + L.VRNN_STATS, res))
    ref, unr = L.vrnn_oracle(inp, mode, case, forced=got), L.vrnn_oracle(inp, "f32", case)
    ck = Checks(tag)
    ck.exact("decin[0, :, H:] is h0", torch.equal(got["decin"][0, :, H:].cpu(), inp["h0"] if inp["h0"] is not None else torch.zeros(B, L.VRNN_R)))
    ck.exact("the phi part of decin row T' is zero", (got["decin"][Tp, :, :H] == 0).all())
    for (name, g, strict), (_, r, _), (_, u, _) in zip(L.vrnn_pieces(got, H), L.vrnn_pieces(ref, H), L.vrnn_pieces(unr, H)):
        if strict:
            ck.close(name, g.reshape(Tp * B, -1), r.reshape(Tp * B, -1), L.BAR_VALUE, row_dim=0)
            continue
        fails, fig = L.two_tier(g, r, u, L.BAR_VALUE, L.VRNN_LOOSE_MULTIPLE)
        print(f"{tag} {name} rows: {fig['over']} of {fig['rows']} over the tight bar (worst step {fig['group_share']:.3f}, worst batch row {fig['row_steps']} of {fig['steps']} steps), "
              f"worst row under it {fig['worst_tight']:.3e}, worst row {fig['worst']:.3e} = {fig['worst_over_in_medians']:.2f} medians (loose bar {fig['loose']:.3e})")
        ck.failures += [f"{name} {f}" for f in fails]
    e_r, e_u = L.median_row_distances(got["decin"][1:, :, H:], ref["decin"][1:, :, H:], unr["decin"][1:, :, H:])
    print(f"{tag} summary: median row of h vs rounded {e_r:.3e}, vs unrounded {e_u:.3e}")
    if not L.MODE_ON * e_r <= e_u:
        ck.failures.append(f"mode not on: the median row of h is {e_r:.3e} from the rounded oracle, {e_u:.3e} from the unrounded one")
    ck.done()
