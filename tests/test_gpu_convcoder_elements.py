"""GPU (MI355X): K11 (csrc/convcoder.hip) per COLUMN — the channel norm, the depthwise stencils and the nearest-resample residual
through `ops.chan_norm`, `ops.dwconv`, `ops.resample_add` and the private links `ops._chan_norm_stats`, `ops._chan_norm_bwd`,
`ops._dwconv_fwd`, `ops._dwconv_bwd`, over the case tables of tests/convcoder_cases.py: the edges of the kernels' thread geometry
(column blocks, row strips), the fusions only `ops.sep_block` reaches, and the regimes a trained coder produces.

Oracle: the torch operators in float64 on the CPU.  Bar of a slice: max(TIMES x the float32 yardstick's own error in that slice,
FLOOR x rms of the slice), TIMES = 4, FLOOR = 2e-5; one slice per column for activations and their gradients, every element against
the rms of the whole tensor for parameter gradients and statistics; a slice whose oracle is identically zero must be exactly zero.
The yardstick is the same torch composition in float32, except for the norm's y, affine, dx and dgamma, where it is the float32
restatement of the kernel's own order (convcoder_cases.norm_kernel_order says why), and for the long-strip test's float32 atomic
sums (convcoder_cases.tiled_atomic_sum).  Exact properties are asserted exactly: a constant
column normalises to beta, rows a strided convolution never reads get a gradient of 0.0, outputs of a transposed convolution that no tap
reaches hold the bias, dead columns behind a ReLU mask get 0.0.  Every figure is printed before it is asserted.

Measured on an MI355X, worst kernel error over its bar: 0.86 for a stencil output (transposed strip behind the affine, post-ReLU
input: 5.4e-8 in a column whose scale is 3e-3), 0.36 and below for every other stencil output, 0.14 and below for the stencils'
data, weight and bias gradients; 0.25 for the norm's y, affine, dx and dgamma wherever the restatement's error is above the floor
(the kernel's bits are the restatement's: errors 4.0e-5, 9.9e-5, 1.4e-5 at mean / spread = 1e3), 0.03 and below for dbeta and the
statistics, 0.28 for dx_chan_sum; long strips 0.34 (dw), 0.32 (dbias), 0.26 (dx_chan_sum), 0.05 and below elsewhere.  No ReLU mask
bit differed from the float64 mask.  The file takes 5 s."""
import pytest
import torch

import convcoder_cases as K
from blvm import _hip, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
ids = lambda c: c.name  # noqa: E731

@pytest.fixture(scope="module", autouse=True)
def _require_hip():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert _hip.load().blvm_device_ok() == 1, "libblvm_hip: no gfx950 device visible"


def dev(t):
    return t.to(DEV).contiguous() if t is not None else None


def check_all(reports):
    failures = [f for r in reports for f in r.failures]
    assert not failures, "\n".join(failures)


# ---- channel norm -----------------------------------------------------------------------------------------------------------------


def norm_yardstick(x, gamma, beta, dy, relu):
    torch32, order = K.norm_link(x, gamma, beta, dy, F32, relu), K.norm_kernel_order(x, gamma, beta, dy, relu)
    return {k: (order[k] if k in K.KERNEL_ORDER_YARDSTICK else v) for k, v in torch32.items()}


@pytest.mark.parametrize("c", K.NORM_CASES, ids=ids)
def test_chan_norm_per_column(c):
    """`ops.chan_norm` forward and backward, `_chan_norm_stats` (mr and the column affine), and — where the input can be a ReLU's
    output — `_chan_norm_bwd(relu_mask=True, dx_chan_sum=...)`."""
    x, gamma, beta, dy = K.norm_inputs(c)
    ref, yard = K.norm_link(x, gamma, beta, dy, F64), norm_yardstick(x, gamma, beta, dy, False)
    xd, gd, bd, dyd = dev(x).requires_grad_(), dev(gamma).requires_grad_(), dev(beta).requires_grad_(), dev(dy)
    y = ops.chan_norm(xd, gd, bd, K.EPS)
    y.backward(dyd)
    tag = f"[{c.name}]"
    reports = [K.compare(f"{tag} y", y, yard["y"], ref["y"], check=False),
               K.compare(f"{tag} dgamma", gd.grad, yard["dgamma"], ref["dgamma"], "elements", check=False),
               K.compare(f"{tag} dbeta", bd.grad, yard["dbeta"], ref["dbeta"], "elements", check=False)]  # fmt: skip
    if K.dx_is_identically_zero(c):
        assert float(xd.grad.abs().max()) == 0.0, "the gradient of a one-row norm is identically zero"
    else:
        reports.append(K.compare(f"{tag} dx", xd.grad, yard["dx"], ref["dx"], check=False))
    cols = K.constant_columns(c.regime, c.L, c.N)
    if cols:  # "evaluated exactly in that order": (x - mean) is exactly zero
        got = y.detach().cpu().reshape(c.L, c.N)[:, cols]
        assert torch.equal(got, beta.repeat(c.B)[cols].expand(c.L, len(cols))), "a constant column must normalise to exactly beta"

    with torch.no_grad():
        xk, gk, bk = xd.detach(), gd.detach(), bd.detach()
        mr, ss = ops._chan_norm_stats(xk, gk, bk, K.EPS)
        for name, t in (("mean", mr[0]), ("rstd", mr[1]), ("scale", ss[0]), ("shift", ss[1])):
            reports.append(K.compare(f"{tag} {name}", t, yard[name], ref[name], "elements", check=False))
        affine = x.double() * ss[0].cpu().double().view(c.B, c.C) + ss[1].cpu().double().view(c.B, c.C)
        reports.append(K.compare(f"{tag} affine", affine, yard["affine"], ref["affine"], check=False))
        if c.regime in K.NONNEG:
            ref, yard = K.norm_link(x, gamma, beta, dy, F64, True), norm_yardstick(x, gamma, beta, dy, True)
            dg, db, ds = (torch.zeros(c.C, device=DEV) for _ in range(3))
            dx = ops._chan_norm_bwd(xk, dyd, mr, gk, True, dg, db, dx_chan_sum=ds)
            if K.dx_is_identically_zero(c):
                assert float(dx.abs().max()) == 0.0
            else:
                reports.append(K.compare(f"{tag} relu_mask dx", dx, yard["dx"], ref["dx"], exact_zeros=True, check=False))
            reports.append(K.compare(f"{tag} relu_mask dgamma", dg, yard["dgamma"], ref["dgamma"], "elements", check=False))
            reports.append(K.compare(f"{tag} relu_mask dbeta", db, yard["dbeta"], ref["dbeta"], "elements", check=False))
            if c.regime in K.CHAN_SUM_REGIMES:
                reports.append(K.compare(f"{tag} relu_mask dx_chan_sum", ds, yard["dx_chan_sum"], ref["dx_chan_sum"], "elements", check=False))
            if c.regime == "post_relu":
                dead = K.dead_columns(c.N)
                assert float(dx.reshape(c.L, c.N)[:, dead].abs().max()) == 0.0, "a dead column's gradient must be exactly zero"
    check_all(reports)


# ---- depthwise stencils -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("c", K.CONV_CASES, ids=ids)
def test_dwconv_per_column(c):
    """Forward, data gradient, weight and bias gradient of one stencil configuration.  Plain cases go through `ops.dwconv` (autograd),
    the norm-as-affine cases through `_dwconv_fwd` / `_dwconv_bwd(in_affine=...)`, gradient buffers starting at zero."""
    x, w, bias, dy, affine = K.conv_inputs(c)
    cfg = (c.stride, c.dilation, c.transposed, c.relu)
    ref0, yard0 = K.conv_link(c, x, w, bias, dy, F64, affine), K.conv_link(c, x, w, bias, dy, F32, affine)
    xd, wd, bd, dyd = dev(x), dev(w.view(c.C, 1, c.k)), dev(bias), dev(dy)
    tag = f"[{c.name}]"
    if affine is None:
        xd.requires_grad_(), wd.requires_grad_()
        if bd is not None:
            bd.requires_grad_()
        y = ops.dwconv(xd, wd, bd, *cfg)
    else:
        y = ops._dwconv_fwd(xd, wd, bd, *cfg, in_affine=dev(affine))
    assert tuple(y.shape) == (c.L_out, c.B, c.C)
    fwd = K.compare(f"{tag} y", y, yard0["y"], ref0["y"], exact_zeros=not c.relu, check=False)
    check_all([fwd])  # the mask is taken from this output only once it has passed
    y_cpu = y.detach().cpu()
    rows = K.unreached_outputs(c)
    if rows:
        want = torch.zeros(c.C) if bias is None else (torch.relu(bias) if c.relu else bias)
        assert torch.equal(y_cpu[rows], want.expand(len(rows), c.B, c.C)), "outputs that no tap reaches must hold the bias exactly"
    mask = None
    if c.relu:
        K.mask_flips(f"{tag} mask", y_cpu, ref0["pre"], fwd.bars)
        mask = y_cpu > 0
    ref, yard = K.conv_link(c, x, w, bias, dy, F64, affine, mask), K.conv_link(c, x, w, bias, dy, F32, affine, mask)
    if affine is None:
        y.backward(dyd)
        dx, dw, dbias = xd.grad, wd.grad.view(c.C, c.k), (bd.grad if bd is not None else None)
    else:
        dw, dbias = torch.zeros(c.C, c.k, device=DEV), (torch.zeros(c.C, device=DEV) if bias is not None else None)
        dx = ops._dwconv_bwd(xd, wd, y if c.relu else None, dyd, *cfg, True, dw, dbias, in_affine=dev(affine))
    reports = [K.compare(f"{tag} dx", dx, yard["dx"], ref["dx"], exact_zeros=True, check=False),
               K.compare(f"{tag} dw", dw, yard["dw"], ref["dw"], "elements", check=False)]  # fmt: skip
    if bias is not None:
        reports.append(K.compare(f"{tag} dbias", dbias, yard["dbias"], ref["dbias"], "elements", check=False))
    rows = K.unread_rows(c)
    if rows:
        assert float(dx[rows].abs().max()) == 0.0, "rows that the strided convolution never reads must get a gradient of exactly 0.0"
    check_all(reports)


# ---- nearest-resampled residual ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("Lx,Ly", K.RESAMPLE_CASES)
def test_resample_add_bit_exact(Lx, Ly):
    B, C = K.ROWS_AT
    g = torch.Generator().manual_seed(Lx * 1009 + Ly)
    x, y, dout = (torch.randn(L, B, C, generator=g) for L in (Lx, Ly, Ly))
    ref = K.resample_link(y, x, dout)
    xd, yd = dev(x).requires_grad_(), dev(y).requires_grad_()
    out = ops.resample_add(yd, xd)
    out.backward(dev(dout))
    assert torch.equal(out.detach().cpu(), ref["out"])  # index arithmetic identical to torch's, one add: bit-exact
    assert torch.equal(yd.grad.cpu(), ref["dy"])
    dx = xd.grad.cpu()
    if Ly <= Lx:  # an injective map: one term per row, and rows that no output reads stay at exactly 0.0
        assert torch.equal(dx, ref["dx"])
        unread = (ref["dx"] == 0).all(2).all(1)
        assert int(unread.sum()) == Lx - Ly and float(dx[unread].abs().max() if bool(unread.any()) else 0.0) == 0.0
    else:  # atomics: the order of the (<= ceil(Ly/Lx)) adds per element is free
        ref64 = K.resample_link(y, x, dout, F64)
        K.compare(f"[resample {Lx}->{Ly}] dx", dx, ref["dx"], ref64["dx"])


# ---- the long-strip arm -----------------------------------------------------------------------------------------------------------


def test_long_strips():
    """rows_per_block above its minimum (pick_rows_per_block: L > 64 * ceil(4096 / column blocks)) at its smallest shape, N = 16384 and
    L = 4100: the statistics pass forward and backward, the norm apply passes, the weight-gradient strip at stride 2 and the masked
    column sum.  One [L, 64] base block is tiled across the 256 samples, so the float64 oracle is computed for 64 columns and the
    per-channel sums are the base sums times the number of tiles; operands are built and compared on the device.  The float32
    per-channel sums (dx_chan_sum, dw, dbias: 16 000 atomic adds each) are measured against `tiled_atomic_sum`."""
    B, C, L = K.LONG_B, K.LONG_C, K.LONG_L
    assert K.rows_per_block(L, B * C, K.STATS_MIN_ROWS) > K.STATS_MIN_ROWS
    base = K.NormCase("long", 1, C, L, regime="padded")
    x, gamma, beta, dy = K.norm_inputs(base)
    ref, yard = K.norm_link(x, gamma, beta, dy, F64, True), norm_yardstick(x, gamma, beta, dy, True)

    def tile(t):  # [L,1,C] -> [L,B,C] on the device
        return dev(t).expand(t.shape[0], B, C).contiguous()

    def columns(name, got, yard_t, ref_t):
        """Per column over all tiles, on the device: the worst tile of every base column against that column's bar."""
        r, yd = dev(ref_t.reshape(-1, C)), yard_t.reshape(-1, C).double()
        err = torch.zeros(C, dtype=F64, device=DEV)
        for b0 in range(0, B, 32):
            err = torch.maximum(err, (got[:, b0 : b0 + 32].double() - r[:, None, :]).abs().amax((0, 1)))
        err = err.cpu()
        err_y, scale = (yd - ref_t.reshape(-1, C)).abs().amax(0), ref_t.reshape(-1, C).pow(2).mean(0).sqrt()
        bars = torch.maximum(K.TIMES * err_y, K.FLOOR * scale)
        n = int((err / bars).argmax())
        print(f"[long] {name}: kernel {float(err[n]):.3e}  yardstick {float(err_y[n]):.3e}  bar {float(bars[n]):.3e}  ratio {float(err[n] / bars[n]):.3f}  (column {n})")
        return [f"[long] {name}[column {m}]: {float(err[m]):.3e} above {float(bars[m]):.3e}" for m in torch.nonzero(err > bars).flatten().tolist()[:4]]

    def sums(name, got, yard_t, ref_t, over="slice"):
        return K.compare(f"[long] {name}", got.cpu().double() / B, yard_t, ref_t, "elements", check=False, yard_over=over).failures

    failures = []
    with torch.no_grad():
        xd, dyd, gd, bd = tile(x), tile(dy), dev(gamma), dev(beta)
        y, mr = ops._chan_norm_fwd(xd, gd, bd, K.EPS)
        failures += columns("y", y, yard["y"], ref["y"])
        del y
        dg, db, ds = (torch.zeros(C, device=DEV) for _ in range(3))
        dx = ops._chan_norm_bwd(xd, dyd, mr, gd, True, dg, db, dx_chan_sum=ds)
        failures += columns("dx", dx, yard["dx"], ref["dx"])
        del dx, dyd
        failures += sums("dgamma", dg, yard["dgamma"], ref["dgamma"]) + sums("dbeta", db, yard["dbeta"], ref["dbeta"])
        apply_rows = K.rows_per_block(L, B * C, K.APPLY_MIN_ROWS)  # norm_bwd_apply_kernel's workgroups add their sums atomically
        failures += sums("dx_chan_sum", ds, K.tiled_atomic_sum(K.block_sums(yard["dx"].reshape(L, C), apply_rows), B), ref["dx_chan_sum"], "tensor")
        # transposed stencil at stride 2: the weight-gradient strip walks the L input rows, the masked column sum the L_out output rows
        c = K.ConvCase("long_tconv", 1, C, L, stride=2, transposed=True, relu=True)
        assert K.rows_per_block(c.L_out, B * C, K.STATS_MIN_ROWS) > K.STATS_MIN_ROWS
        _, w, bias, dy2, _ = K.conv_inputs(c)
        ref0, yard0 = K.conv_link(c, x, w, bias, dy2, F64), K.conv_link(c, x, w, bias, dy2, F32)
        wd, biasd = dev(w), dev(bias)
        y = ops._dwconv_fwd(xd, wd, biasd, 2, 1, True, True)
        bad = columns("tconv y", y, yard0["y"], ref0["y"])
        assert not bad, "\n".join(bad)
        mask = y[:, 0].cpu() > 0  # every tile holds the same columns: the first one's mask, checked to be everyone's
        assert bool(((y > 0) == dev(mask)[:, None, :]).all())
        mask = mask.view(c.L_out, 1, C)
        first = K.compare("[long] tconv y, first tile", y[:, :1], yard0["y"], ref0["y"])
        K.mask_flips("[long] tconv mask", y[:, :1], ref0["pre"], first.bars)
        ref, yard = K.conv_link(c, x, w, bias, dy2, F64, None, mask), K.conv_link(c, x, w, bias, dy2, F32, None, mask)
        dw, dbias = torch.zeros(C, c.k, device=DEV), torch.zeros(C, device=DEV)
        dx = ops._dwconv_bwd(xd, wd, y, tile(dy2), 2, 1, True, True, True, dw, dbias)
        failures += columns("tconv dx", dx, yard["dx"], ref["dx"])
        g = torch.where(mask.view(c.L_out, C), dy2.view(c.L_out, C), torch.zeros(()))  # the masked output gradient
        taps = torch.stack([x.view(L, C) * g[j : j + 2 * (L - 1) + 1 : 2] for j in range(c.k)], 2)  # [L,C,k]: dw[c,j] = sum_u x[u] g[2u + j]
        dw_yard = K.tiled_atomic_sum(K.block_sums(taps, K.rows_per_block(L, B * C, K.WGRAD_MIN_ROWS)), B)
        db_yard = K.tiled_atomic_sum(K.block_sums(g, K.rows_per_block(c.L_out, B * C, K.STATS_MIN_ROWS)), B)
        failures += sums("tconv dw", dw, dw_yard, ref["dw"], "tensor") + sums("tconv dbias", dbias, db_yard, ref["dbias"], "tensor")
    assert not failures, "\n".join(failures)


# ---- alignment --------------------------------------------------------------------------------------------------------------------


def test_views_offset_by_one_float_are_refused():
    """Every K11 entry point that moves 16 bytes per lane requires 16-byte-aligned tensors (BLVM_REQUIRE(aligned16(...)) in
    csrc/convcoder.hip): a view that starts one float into its storage is refused by the host-side check, before any launch."""
    L, B, C = 6, 2, 8
    N = B * C

    def off(*shape):  # contiguous, 4 bytes past a 16-byte boundary
        n = 1
        for s in shape:
            n *= s
        t = torch.zeros(n + 1, device=DEV)[1:].view(*shape)
        assert t.is_contiguous() and t.data_ptr() % 16 == 4
        return t

    def ok(*shape):
        return torch.zeros(*shape, device=DEV)

    g, b, w = ok(C), ok(C), ok(C, 5)
    ss = ok(2, N)
    ss_off = torch.zeros(2 * N + 5, device=DEV)[1:].view(-1)  # in_scale at +4 bytes, in_shift N floats further: both misaligned
    calls = {
        "resample_add_fwd: y": lambda: ops.resample_add(off(L, B, C), ok(L, B, C)),
        "resample_add_fwd: x": lambda: ops.resample_add(ok(L, B, C), off(L, B, C)),
        "chan_norm_fwd: x": lambda: ops._chan_norm_fwd(off(L, B, C), g, b, K.EPS),
        "chan_norm_fwd: gamma": lambda: ops._chan_norm_fwd(ok(L, B, C), off(C), b, K.EPS),
        "chan_norm_stats: x": lambda: ops._chan_norm_stats(off(L, B, C), g, b, K.EPS),
        "chan_norm_bwd: dy": lambda: ops._chan_norm_bwd(ok(L, B, C), off(L, B, C), ok(2, N), g, False, ok(C), ok(C)),
        "chan_norm_bwd: mr": lambda: ops._chan_norm_bwd(ok(L, B, C), ok(L, B, C), off(2, N), g, False, ok(C), ok(C)),
        "dwconv_fwd: x": lambda: ops._dwconv_fwd(off(L, B, C), w, b, 1, 1, False, False),
        "dwconv_fwd: bias": lambda: ops._dwconv_fwd(ok(L, B, C), w, off(C), 1, 1, False, False),
        "dwconv_fwd: in_scale": lambda: ops._dwconv_fwd(ok(L, B, C), w, b, 1, 1, False, False, in_affine=(ss_off[:N], ss_off[N : 2 * N])),
        "dwconv_bwd: dy": lambda: ops._dwconv_bwd(ok(L, B, C), w, None, off(2, B, C), 1, 1, False, False, True, ok(C, 5), ok(C)),
        "dwconv_bwd: y": lambda: ops._dwconv_bwd(ok(L, B, C), w, off(2, B, C), ok(2, B, C), 1, 1, False, True, True, ok(C, 5), ok(C)),
        "dwconv_bwd: in_scale": lambda: ops._dwconv_bwd(ok(L, B, C), w, None, ok(2, B, C), 1, 1, False, False, True, ok(C, 5), ok(C),
                                                        in_affine=(ss_off[:N], ss_off[N : 2 * N])),
    }  # fmt: skip
    for name, call in calls.items():
        with pytest.raises(_hip.BlvmHipError, match="alignment"):
            call()
        print(f"{name}: refused")
    torch.cuda.synchronize()
    # the aligned forms of the two calls this file's checks were added to go through
    ops.resample_add(ok(L, B, C), ok(L, B, C))
    ops._dwconv_bwd(ok(L, B, C), w, None, ok(2, B, C), 1, 1, False, False, True, ok(C, 5), ok(C), in_affine=(ss[0], ss[1]))
    torch.cuda.synchronize()
