"""CPU: the K11 case tables, oracles, yardsticks and comparison of tests/convcoder_cases.py checked by themselves, no device touched.
  * the fused links' oracles equal `BlockSeparable`'s torch modules composed the long way, in float64, link by link;
  * every bar leaves room: TIMES * the float32 yardstick's own error is at most ROOM = 1e-2 of the slice's scale, for every case and
    tensor, so a wrong element of the size of the data is a hundred bars away;
  * the float32 yardstick flips no ReLU mask bit for the committed seeds;
  * `compare` fails for a yardstick output with ONE defect of the kind a subtly wrong kernel has, and passes for the untouched one;
  * a float32 restatement of the kernels' own order of operations passes every case (the bars can be met);
  * the tables hit every edge class, computed from the geometry constants at the top of the helper."""
import functools

import pytest
import torch
import torch.nn as nn

import convcoder_cases as K
from blvm.models.clockwork_vae.convolutional_coders import BlockSeparable

F64, F32 = torch.float64, torch.float32
ids = lambda c: c.name  # noqa: E731


@functools.lru_cache(maxsize=None)
def norm_results(c):
    x, gamma, beta, dy = K.norm_inputs(c)
    out = {}
    for relu in (False, True) if c.regime in K.NONNEG else (False,):
        torch32, order = K.norm_link(x, gamma, beta, dy, F32, relu), K.norm_kernel_order(x, gamma, beta, dy, relu)
        yard = {k: (order[k] if k in K.KERNEL_ORDER_YARDSTICK else v) for k, v in torch32.items()}
        out[relu] = (K.norm_link(x, gamma, beta, dy, F64, relu), yard, order, torch32)
    return out


def norm_tensors(c, relu):
    names = [t for t in NORM_TENSORS if not (t[0] == "dx" and K.dx_is_identically_zero(c))] + [("affine", "columns")]
    return names + [("dx_chan_sum", "elements")] if relu and c.regime in K.CHAN_SUM_REGIMES else names


@functools.lru_cache(maxsize=None)
def conv_results(c):
    x, w, bias, dy, affine = K.conv_inputs(c)
    return (K.conv_link(c, x, w, bias, dy, F64, affine), K.conv_link(c, x, w, bias, dy, F32, affine),
            K.conv_kernel_order(c, x, w, bias, dy, affine))  # fmt: skip


NORM_TENSORS = [("y", "columns"), ("dx", "columns"), ("dgamma", "elements"), ("dbeta", "elements"), ("mean", "elements"),
                ("rstd", "elements"), ("scale", "elements"), ("shift", "elements")]  # fmt: skip
CONV_TENSORS = [("y", "columns"), ("dx", "columns"), ("dw", "elements"), ("dbias", "elements")]


# ---- oracle checks ----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("stride", [1, 2, 4])
def test_fused_link_oracles_equal_the_torch_modules_composed_the_long_way(stride, transposed):
    torch.manual_seed(3 + stride + 10 * transposed)
    Cb, B, L = 3, 2, 23
    block = BlockSeparable(Cb, 5, stride, 1, nn.ReLU, transposed, bias=True).double()
    conv1, act, norm1, sep = block.block.module
    with torch.no_grad():
        for m in (norm1, sep.norm):
            m.weight.copy_(1 + 0.3 * torch.randn_like(m.weight))
            m.bias.copy_(0.3 * torch.randn_like(m.bias))
    C = conv1.out_channels
    x = torch.randn(B, Cb, L, dtype=F64)
    z1 = conv1(x)
    a1 = act(z1)
    n1 = norm1(a1)
    z2 = sep.depthwise_conv(n1)
    d = sep.activation(z2)
    n2 = sep.norm(d)
    for t in (z1, n1, z2):
        t.retain_grad()
    dn2 = torch.randn_like(n2)
    n2.backward(dn2)

    def close(a, b):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-12 * (1 + float(b.abs().max())), float((a - b).abs().max())

    a1_tm, d_tm = K.tm(a1.detach()), K.tm(d.detach())
    # norm 2 behind the stencil's ReLU: dx is the gradient with respect to the pre-activation
    o2 = K.norm_link(d_tm, sep.norm.weight.detach(), sep.norm.bias.detach(), K.tm(dn2), F64, relu_mask=True, eps=sep.norm.eps)
    close(o2["y"], K.tm(n2.detach()))
    close(o2["dx"], K.tm(z2.grad))
    close(o2["dgamma"], sep.norm.weight.grad)
    close(o2["dbeta"], sep.norm.bias.grad)
    # the statistics of norm 1 as a column affine, and the stencil that applies it on load
    o1 = K.norm_link(a1_tm, norm1.weight.detach(), norm1.bias.detach(), K.tm(n1.grad), F64, relu_mask=True, eps=norm1.eps)
    close(o1["affine"], K.tm(n1.detach()))
    case = K.ConvCase("block", B, C, L, 5, stride, 1, transposed, bias=True, relu=True, regime="post_relu")
    oc = K.conv_link(case, a1_tm, sep.depthwise_conv.weight.detach().view(C, 5), sep.depthwise_conv.bias.detach(), K.tm(_upstream_of_relu(d, dn2, sep)), F64,
                     affine=torch.stack([o1["scale"], o1["shift"]]))  # fmt: skip
    close(oc["y"], d_tm)
    close(oc["dx"], K.tm(n1.grad))
    close(oc["dw"], sep.depthwise_conv.weight.grad.view(C, 5))
    close(oc["dbias"], sep.depthwise_conv.bias.grad)
    # norm 1 behind the 1x1 convolution's ReLU: dx with respect to its pre-activation, and that layer's bias gradient in the same pass
    close(o1["dx"], K.tm(z1.grad))
    close(o1["dx_chan_sum"], conv1.bias.grad)
    close(o1["dgamma"], norm1.weight.grad)
    close(o1["dbeta"], norm1.bias.grad)
    close(torch.stack([o1["mean"], o1["rstd"]]), torch.stack([a1.detach().mean(2).reshape(-1), (a1.detach().var(2, unbiased=False) + norm1.eps).rsqrt().reshape(-1)]))


def _upstream_of_relu(d, dn2, sep):
    """The gradient that reaches the stencil's OUTPUT d (behind its fused ReLU, in front of norm 2), from the modules."""
    dd = d.detach().clone().requires_grad_()
    return torch.autograd.grad(sep.norm(dd), dd, dn2)[0]


@pytest.mark.parametrize("c", [c for c in K.CONV_CASES if not c.transposed and K.unread_rows(c)], ids=ids)
def test_oracle_gradient_is_exactly_zero_on_rows_never_read(c):
    ref, yard, _ = conv_results(c)
    rows = K.unread_rows(c)
    assert float(ref["dx"][rows].abs().max()) == 0.0 and float(yard["dx"][rows].abs().max()) == 0.0
    assert bool((ref["dx"] != 0).any())


@pytest.mark.parametrize("c", [c for c in K.CONV_CASES if K.unreached_outputs(c)], ids=ids)
def test_oracle_outputs_no_tap_reaches_hold_the_bias(c):
    ref, _, _ = conv_results(c)
    _, _, bias, _, _ = K.conv_inputs(c)
    want = torch.zeros(c.C) if bias is None else (torch.relu(bias) if c.relu else bias)
    rows = K.unreached_outputs(c)
    assert torch.equal(ref["y"][rows], want.double().expand(len(rows), c.B, c.C))


def test_resample_oracle_leaves_unread_rows_at_zero():
    g = torch.Generator().manual_seed(0)
    for Lx, Ly in K.RESAMPLE_CASES:
        if Ly < Lx:
            r = K.resample_link(torch.randn(Ly, 2, 4, generator=g), torch.randn(Lx, 2, 4, generator=g), torch.randn(Ly, 2, 4, generator=g))
            zero_rows = (r["dx"] == 0).all(2).all(1)
            assert int(zero_rows.sum()) == Lx - Ly, (Lx, Ly)


# ---- non-vacuity, mask flips --------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("c", K.NORM_CASES, ids=ids)
def test_norm_bars_leave_room(c):
    for relu, (ref, yard, _, _) in norm_results(c).items():
        for name, kind in norm_tensors(c, relu):
            room = K.yardstick_room(yard[name], ref[name], kind)
            assert room <= K.ROOM, f"{c.name} relu_mask={relu} {name}: TIMES * yardstick error is {room:.3e} of the scale"


@pytest.mark.parametrize("c", K.CONV_CASES, ids=ids)
def test_conv_bars_leave_room(c):
    ref, yard, _ = conv_results(c)
    for name, kind in CONV_TENSORS:
        if ref[name] is not None:
            room = K.yardstick_room(yard[name], ref[name], kind)
            assert room <= K.ROOM, f"{c.name} {name}: TIMES * yardstick error is {room:.3e} of the scale"


@pytest.mark.parametrize("c", [c for c in K.CONV_CASES if c.relu], ids=ids)
def test_no_mask_bit_is_ambiguous_for_the_committed_seeds(c):
    ref, yard, stand_in = conv_results(c)
    bars = K.compare(f"{c.name} y", yard["y"], yard["y"], ref["y"]).bars
    assert K.mask_flips(c.name, yard["y"], ref["pre"], bars) == 0
    assert K.mask_flips(c.name + " (kernel order)", stand_in["y"], ref["pre"], bars) == 0
    if c.zero_x:  # exactly-zero pre-activations: masked on both sides, not ambiguous — and under a gradient that is NOT zero there
        _, _, _, dy, _ = K.conv_inputs(c)
        assert torch.equal(yard["pre"] == 0, ref["pre"] == 0)
        assert int(((ref["pre"] == 0) & (dy != 0)).sum()) >= c.N, "a mask of y >= 0 would let nothing but zeros through"


# ---- a correct kernel's stand-in meets every bar -----------------------------------------------------------------------------------


@pytest.mark.parametrize("c", K.NORM_CASES, ids=ids)
def test_kernel_order_restatement_meets_the_norm_bars(c):
    x, gamma, beta, _ = K.norm_inputs(c)
    for relu, (ref, yard, got, _) in norm_results(c).items():
        for name, kind in norm_tensors(c, relu):
            K.compare(f"{c.name} relu_mask={relu} {name}", got[name], yard[name], ref[name], kind, exact_zeros=(name == "dx" and relu))
    if K.dx_is_identically_zero(c):
        for ref, _, got, _ in norm_results(c).values():
            assert float(got["dx"].abs().max()) == 0.0 and float(ref["dx"].abs().max()) <= 1e-12
    cols = K.constant_columns(c.regime, c.L, c.N)
    if cols:
        y = norm_results(c)[False][2]["y"].reshape(c.L, c.N)
        assert torch.equal(y[:, cols], beta.repeat(c.B)[cols].expand(c.L, len(cols)))


@pytest.mark.parametrize("c", K.CONV_CASES, ids=ids)
def test_kernel_order_restatement_meets_the_conv_bars(c):
    ref, yard, got = conv_results(c)
    for name, kind in CONV_TENSORS:
        if ref[name] is not None:
            K.compare(f"{c.name} {name}", got[name], yard[name], ref[name], kind, exact_zeros=(name == "dx"))


def test_cancelling_columns_need_the_kernel_order_yardstick():
    """Why `y`, `affine` (x*ss[0] + ss[1] against the norm), `dx` and `dgamma` are measured against the kernel-order restatement:
    against torch's float32 GroupNorm, a restatement that rounds the float64 mean ONCE, as the kernel does, is above TIMES x that
    yardstick in some columns (dgamma: elements) of the cancelling regimes — 1.96, 4.12, 1.42 and 8.80 times the bar at the worst.  Should this stop being so, KERNEL_ORDER_YARDSTICK has no reason left."""
    kinds = dict(NORM_TENSORS, affine="columns")
    for name in K.KERNEL_ORDER_YARDSTICK:
        worst, total = 0.0, 0
        for c in K.NORM_CASES:
            if c.regime in ("ratio100", "ratio1000", "tiny_spread"):
                ref, _, order, torch32 = norm_results(c)[False]
                rep = K.compare(f"{c.name} {name} against torch float32", order[name], torch32[name], ref[name], kinds[name], check=False)
                worst, total = max(worst, rep.ratio), total + c.N
        print(f"{name}, torch float32 yardstick: worst ratio {worst:.2f} over the {total} columns of the cancelling cases")
        assert worst > 1.0


# ---- the comparison notices a subtly wrong kernel -----------------------------------------------------------------------------------


def case(table, name):
    return next(c for c in table if c.name == name)


def fails(*args, **kw):
    return not K.compare(*args, check=False, **kw).ok


def test_defect_last_row_left_out_of_one_columns_sum():
    c = case(K.NORM_CASES, "rows65")
    x, gamma, beta, dy = K.norm_inputs(c)
    ref, yard, _, _ = norm_results(c)[False]
    assert not fails("y", yard["y"], yard["y"], ref["y"])
    n, L = 257, c.L
    col = x.reshape(L, c.N)[:, n]
    mean = col[:-1].sum() / L
    var = (col[:-1] ** 2).sum() / L - mean * mean
    bad = yard["y"].clone().reshape(L, c.N)
    bad[:, n] = (col - mean) * (var + K.EPS).rsqrt() * gamma[n % c.C] + beta[n % c.C]
    assert fails("y", bad.view_as(ref["y"]), yard["y"], ref["y"])
    # the same in a per-channel sum: one column's last term missing
    xhat = (col[-1] - col.mean()) * (col.var(unbiased=False) + K.EPS).rsqrt()
    bad = yard["dgamma"].clone()
    bad[n % c.C] -= dy.reshape(L, c.N)[-1, n] * xhat
    assert not fails("dgamma", yard["dgamma"], yard["dgamma"], ref["dgamma"], "elements")
    assert fails("dgamma", bad, yard["dgamma"], ref["dgamma"], "elements")


@pytest.mark.parametrize("name", ["gather_s2_out33", "scatter_s4_in9"])
def test_defect_one_tap_from_the_neighbouring_row_at_the_last_output(name):
    c = case(K.CONV_CASES, name)
    x, w, bias, dy, _ = K.conv_inputs(c)
    ref, yard, _ = conv_results(c)
    assert not fails("y", yard["y"], yard["y"], ref["y"])
    n, u = 259, c.L_out - 1
    j = 2 if not c.transposed else (u - (c.L_in - 1) * c.stride)  # a tap that reaches the last output
    r = u * c.stride + j if not c.transposed else c.L_in - 1
    x2 = x.reshape(c.L_in, c.N)
    bad = yard["pre"].clone().reshape(c.L_out, c.N)
    bad[u, n] += w[n % c.C, j] * (x2[r - 1, n] - x2[r, n])
    bad = torch.relu(bad) if c.relu else bad
    if float(bad[u, n]) == float(yard["y"].reshape(c.L_out, c.N)[u, n]):
        pytest.fail("the defect is invisible behind the ReLU at this element: choose another column")
    assert fails("y", bad.view_as(ref["y"]), yard["y"], ref["y"])


def test_defect_affine_applied_to_an_out_of_range_row_of_a_transposed_stencil():
    c = case(K.CONV_CASES, "affine_tconv_ordinary")
    x, w, bias, dy, affine = K.conv_inputs(c)
    ref, yard, _ = conv_results(c)
    assert not fails("y", yard["y"], yard["y"], ref["y"])
    worst = 0
    for n in range(c.N):  # row -1 read as x = 0 and then transformed to in_shift: tap `stride` of output 0 (tap 1 at stride 1 ...)
        j = c.stride
        bad = yard["pre"].clone().reshape(c.L_out, c.N)
        bad[0, n] += w[n % c.C, j] * affine[1, n]
        bad = torch.relu(bad) if c.relu else bad
        if float(bad[0, n]) != float(yard["y"].reshape(c.L_out, c.N)[0, n]):
            assert fails("y", bad.view_as(ref["y"]), yard["y"], ref["y"])
            worst += 1
    assert worst >= c.N // 4  # (behind the ReLU the defect shows wherever either value is positive)


def test_defect_gamma_from_four_channels_on():
    c = case(K.NORM_CASES, "rows65")
    x, gamma, beta, dy = K.norm_inputs(c)
    ref, yard, _, _ = norm_results(c)[False]
    n = 3
    ch = n % c.C
    bad = yard["y"].clone().reshape(c.L, c.N)
    bad[:, n] = (bad[:, n] - beta[ch]) / gamma[ch] * gamma[(ch + 4) % c.C] + beta[ch]
    assert fails("y", bad.view_as(ref["y"]), yard["y"], ref["y"])
    bad = yard["scale"].clone()
    bad[n] = bad[n] / gamma[ch] * gamma[(ch + 4) % c.C]
    assert not fails("scale", yard["scale"], yard["scale"], ref["scale"], "elements")
    assert fails("scale", bad, yard["scale"], ref["scale"], "elements")


def test_defect_one_relu_mask_bit_flipped():
    c = case(K.CONV_CASES, "gather_s1_out33")
    assert c.relu
    x, w, bias, dy, affine = K.conv_inputs(c)
    ref, yard, _ = conv_results(c)
    mask = yard["y"] > 0
    i = int(ref["pre"].abs().reshape(-1).argmax())  # nowhere near zero
    flipped = mask.clone().reshape(-1)
    flipped[i] = ~flipped[i]
    bad = K.conv_link(c, x, w, bias, dy, F32, affine, mask=flipped.view_as(mask))
    same = K.conv_link(c, x, w, bias, dy, F32, affine, mask=mask)
    for name, kind in (("dx", "columns"), ("dw", "elements"), ("dbias", "elements")):
        assert not fails(name, same[name], yard[name], ref[name], kind)
        assert fails(name, bad[name], yard[name], ref[name], kind), name
    y_bad = yard["y"].clone().reshape(-1)
    y_bad[i] = 0.0 if bool(mask.reshape(-1)[i]) else 1.0
    bars = K.compare("y", yard["y"], yard["y"], ref["y"]).bars
    assert K.mask_flips("flipped", y_bad.view_as(yard["y"]), ref["pre"], bars, check=False)[1]


@pytest.mark.parametrize("name", ["zero_stretch_conv", "zero_stretch_tconv"])
def test_defect_mask_taken_as_not_negative_at_an_exactly_zero_pre_activation(name):
    c = case(K.CONV_CASES, name)
    x, w, bias, dy, affine = K.conv_inputs(c)
    ref, yard, _ = conv_results(c)
    right = K.conv_link(c, x, w, bias, dy, F32, affine, mask=yard["pre"] > 0)
    wrong = K.conv_link(c, x, w, bias, dy, F32, affine, mask=yard["pre"] >= 0)
    assert not fails("dx", right["dx"], yard["dx"], ref["dx"], exact_zeros=True)
    assert fails("dx", wrong["dx"], yard["dx"], ref["dx"], exact_zeros=True)
    # rows whose every output has an exactly-zero pre-activation: 0.0 in the oracle, the upstream gradient's size in the defect
    dead = (ref["dx"] == 0).all(2).all(1)
    assert int(dead.sum()) >= 2 and float(wrong["dx"][dead].abs().max()) > 0.1


def test_defect_dead_columns_gradient_left_unmasked():
    c = case(K.NORM_CASES, "post_relu")
    x, gamma, beta, dy = K.norm_inputs(c)
    ref, yard, _, _ = norm_results(c)[True]
    _, unmasked, _, _ = norm_results(c)[False]
    assert not fails("dx", yard["dx"], yard["dx"], ref["dx"], exact_zeros=True)
    n = K.dead_columns(c.N)[0]
    assert float(ref["dx"].reshape(c.L, c.N)[:, n].abs().max()) == 0.0
    bad = yard["dx"].clone().reshape(c.L, c.N)
    bad[:, n] = unmasked["dx"].reshape(c.L, c.N)[:, n]
    assert fails("dx", bad.view_as(ref["dx"]), yard["dx"], ref["dx"], exact_zeros=True)
    # and a single live-column element at x = 0 left unmasked
    live = [m for m in range(c.N) if m not in K.dead_columns(c.N) and m != K.spike_column(c.N)][0]
    t = int((x.reshape(c.L, c.N)[:, live] == 0).nonzero()[0])
    bad = yard["dx"].clone().reshape(c.L, c.N)
    bad[t, live] = unmasked["dx"].reshape(c.L, c.N)[t, live]
    assert fails("dx", bad.view_as(ref["dx"]), yard["dx"], ref["dx"], exact_zeros=True)


# ---- coverage ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(K.edge_requirements()))
def test_tables_hit_every_edge_class(name):
    pred, table = K.edge_requirements()[name]
    hits = [c.name for c in table if pred(c)]
    assert hits, f"no case sits on the edge '{name}' any more"


def test_table_sizes_and_names():
    names = [c.name for c in K.NORM_CASES + K.CONV_CASES]
    assert len(names) == len(set(names))
    assert len(names) + len(K.RESAMPLE_CASES) <= 150
    assert all(c.edge for c in K.NORM_CASES + K.CONV_CASES)
    for c in K.CONV_CASES:
        assert c.L_out >= 1 and c.C % 4 == 0 and c.k <= 8, c.name
    # the long-strip shape is the smallest that leaves the minimum strips
    assert K.rows_per_block(K.LONG_L, K.LONG_B * K.LONG_C, K.STATS_MIN_ROWS) > K.STATS_MIN_ROWS
    assert K.rows_per_block(K.LONG_L - 4, K.LONG_B * K.LONG_C, K.STATS_MIN_ROWS) == K.STATS_MIN_ROWS
    assert K.rows_per_block(K.LONG_L, K.LONG_B * K.LONG_C // 2, K.STATS_MIN_ROWS) == K.STATS_MIN_ROWS
