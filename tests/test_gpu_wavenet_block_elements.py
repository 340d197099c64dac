"""GPU (MI355X): the fp32 training path of K10 (csrc/wavenet.hip) per COLUMN — one gated residual block through the private links
`ops._wavenet_block_fwd` / `ops._wavenet_block_bwd` (fused kernels at C = S in {32, 64, 96}; the unfused sequence at other widths,
with S = 0 or S != C, and for views that start 4 bytes past a 16-byte boundary), the tall-skinny weight-gradient kernel in its three
forms (BLVM_WN_WGRAD_NPW unset, 1, C/16), stacks that mix the two arms through `ops.wavenet_stack`, the causal convolution through
`ops.conv1d_k2` / `ops._conv1d_k2_bwd`, and `ops.scale_act` — over the case tables of tests/wavenet_block_cases.py: the edges of the
kernels' geometry (16 rows per wave, 64 per workgroup, the skip offset, shift > rows, the weight-gradient kernel's chunks and
slices) and the regimes a trained WaveNet produces (saturated gates, a grown residual stream, one-hot upstream gradients).

Oracle: `block_link` / `stack_link` / `conv_k2_link` in float64 on the CPU.  Bar of a slice: max(TIMES x the float32 yardstick's own
error in that slice, FLOOR x rms of the slice), TIMES = 4, FLOOR = 2e-5; one slice per (sample, channel) column over time for pre,
act, o, skip and d_x (d_x over all rows + shift rows), every element against the rms of the whole tensor for weight and bias
gradients.  The yardstick is the same link in float32, except for pre, act, dconv_w and dconv_b of the fused cases, where it is the
float32 restatement of the kernels' own accumulation order (wavenet_block_cases.block_kernel_order says why: with a grown residual
stream the rounding of pre is above the floor in any order and falls on different elements in different orders), and for the weight
and bias gradients at >= 1 537 rows, where it is the float32 sum in the kernel's own partition (wgrad_partition_sums).  The causal
convolution's one-frame outputs (L_in = d + 1) are judged per element against the rms of the tensor: a column of one element has that
element's size as its scale, which can be arbitrarily close to zero.  Exact properties are asserted exactly: one-hot causality and
batch independence, the band of d_x that neither tap reaches when shift > rows (d_x is handed over full of a sentinel value), nothing
written outside [0, T_skip*B) of the skip buffer or outside o and d_x, rows of drs_w / drs_b below C when there is no d_o.  Every
figure is printed before it is asserted.

Measured on an MI355X, worst kernel error over its bar.  Fused block: 0.74 for d_x (a one-hot column of two elements, 1.1e-8 against
a scale of 7e-4) and 0.54 for drs_w in the one-hot cases, 0.36 and below for d_x and 0.24 for drs_w in the dense ones; 0.28 for
dconv_w, 0.26 for dconv_b and act, 0.22 for pre (where the restatement's error is above the floor the kernel's error is the
restatement's: C = 96 `grown`, dconv_w 1.42e-4 against 1.27e-4, act 3.71e-6 against 3.65e-6), 0.14 for skip, 0.07 for o, 0.04 for
drs_b.  Against the
torch float32 yardstick the same run gave 1.25 (C = 64) and 2.47 (C = 96) for dconv_w and 1.6 for dconv_b in `grown`, and passed
everywhere else.  Unfused block: 0.36 dconv_w, 0.32 act, 0.29 dconv_b, 0.25 d_x, 0.20 and below for the rest.  Weight-gradient
forms: 0.22 dconv_w (8 309 rows, all column tiles), 0.13 drs_w, 0.12 dconv_b, 0.08 drs_b.  Stacks: 0.52 dconv_w, 0.46 d_x, 0.26 and
below for the rest (all in the saturated stack).  conv1d_k2: 0.10 dW, 0.08 out, 0.07 d_x, 0.03 db.  scale_act: every bit equal.
The file takes 5 s."""
import functools

import pytest
import torch

import wavenet_block_cases as K
from blvm import _hip, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
SENTINEL = 12345.0
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


class Bracketed:
    """A contiguous device tensor with sentinel floats on both sides, starting on a 16-byte boundary or 4 bytes past one."""

    def __init__(self, shape, fill=None, misaligned=False):
        n = 1
        for s in shape:
            n *= s
        pad = 4 * shape[-1]  # four rows (a multiple of 16 bytes: every width here is a multiple of 4)
        self.buf = torch.full((2 * pad + n + 4,), SENTINEL, device=DEV)
        self.start, self.n = pad + (1 if misaligned else 0), n
        self.view = self.buf[self.start : self.start + n].view(*shape)
        if fill is not None:
            self.view.copy_(fill)
        assert self.view.is_contiguous() and self.view.data_ptr() % 16 == (4 if misaligned else 0)

    def untouched(self):
        return bool((self.buf[: self.start] == SENTINEL).all()) and bool((self.buf[self.start + self.n :] == SENTINEL).all())


@functools.lru_cache(maxsize=None)
def block_links(c):
    """-> inputs, float64 oracle, yardstick (`block_yardstick`), the torch float32 link."""
    t = K.block_inputs(c)
    torch32 = K.block_link(c, t, F32)
    return t, K.block_link(c, t, F64), K.block_yardstick(c, t, torch32), torch32


def block_forward(c, t, x=None):
    """-> (x, weights) on the device, pre, act, reserve, o and skip (Bracketed or None)."""
    xd = dev(t["x"] if x is None else x)
    w = tuple(dev(t[k]) for k in ("conv_w", "conv_b", "rs_w", "rs_b"))
    o = Bracketed((c.L_out, c.B, c.C), misaligned=c.align == "o") if c.has_o else None
    skip = Bracketed((c.T_skip, c.B, c.S), t["skip0"], c.align == "skip") if c.S else None
    pre, act, reserve = ops._wavenet_block_fwd(xd, *w, c.dilation, c.T_skip, K.INV_STD, o.view if o else None, skip.view if skip else None)
    return xd, w, pre, act, reserve, o, skip


def run_block(c, t):
    xd, (cw, cb, rw, rb), pre, act, reserve, o, skip = block_forward(c, t)
    d_o = Bracketed((c.L_out, c.B, c.C), t["d_o"], c.align == "o").view if c.has_d_o else None
    d_skip = Bracketed((c.T_skip, c.B, c.S), t["d_skip"], c.align == "skip").view if c.S else None
    g = {k: torch.zeros_like(p) for k, p in zip(K.BLOCK_ELEMENTS, (cw, cb, rw, rb))}
    d_x = Bracketed((c.L_in, c.B, c.C))  # every element holds the sentinel: the zeros asserted below are the kernels' own
    ops._wavenet_block_bwd(xd, cw, rw, reserve, d_o, d_skip, c.dilation, c.T_skip, K.INV_STD, g["dconv_w"], g["dconv_b"], g["drs_w"], g["drs_b"], d_x.view)
    torch.cuda.synchronize()
    assert d_x.untouched(), "the block wrote outside d_x"
    assert o is None or o.untouched(), "the block wrote outside its residual output"
    assert skip is None or skip.untouched(), "the block wrote outside [0, T_skip*B) of the skip buffer"
    got = dict(pre=pre, act=act, o=o.view if o else None, skip=skip.view if skip else None, d_x=d_x.view, **g)
    return {k: (v.cpu() if v is not None else None) for k, v in got.items()}


def block_reports(c, got, ref, yard, tag, elements_yard=None):
    reports = []
    for k in K.BLOCK_COLUMNS:
        if ref[k] is not None:
            reports.append(K.compare(f"{tag} {k}", got[k], yard[k], ref[k], exact_zeros=k == "d_x", check=False))
    for k in K.BLOCK_ELEMENTS:
        if elements_yard is None:
            reports.append(K.compare(f"{tag} {k}", got[k], yard[k], ref[k], "elements", check=False))
        else:
            reports.append(K.compare(f"{tag} {k}", got[k], elements_yard[k], ref[k], "elements", check=False, yard_over="tensor"))
    return reports


def exact_block_properties(c, got):
    d_x = got["d_x"].reshape(c.L_in * c.B, c.C)
    if c.shift > c.rows:
        assert float(d_x[c.rows : c.shift].abs().max()) == 0.0, "rows [rows, shift) of d_x receive neither tap: exactly 0"
    if not c.has_d_o:
        assert float(got["drs_w"][: c.C].abs().max()) == 0.0 and float(got["drs_b"][: c.C].abs().max()) == 0.0, "no d_o: residual rows of drs get 0"
    if c.regime == "onehot":
        t, b, _ = K.hot_position(c)
        outside = torch.ones(c.L_in, c.B, dtype=torch.bool)
        outside[t, b], outside[t + c.dilation, b] = False, False
        assert float(got["d_x"][outside].abs().max()) == 0.0, "one-hot upstream gradient: d_x lives in rows t and t + d of one sample"
        assert bool((got["d_x"][t, b] != 0).any()) and bool((got["d_x"][t + c.dilation, b] != 0).any())


# ---- one block --------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("c", K.BLOCK_CASES, ids=ids)
def test_block_per_column(c):
    """Forward (pre, act, o, skip = prior + own) and backward (d_x, the four parameter gradients into zeroed buffers) of one block."""
    t, ref, yard, _ = block_links(c)
    got = run_block(c, t)
    exact_block_properties(c, got)
    check_all(block_reports(c, got, ref, yard, f"[{c.name}]"))


@pytest.mark.parametrize("c", K.WGRAD_CASES, ids=ids)
@pytest.mark.parametrize("form", [0, 1, 2], ids=["npw_unset", "npw_1", "npw_all"])
def test_wgrad_forms_per_element(c, form, monkeypatch):
    """Each form of wn_ts_wgrad_kernel against the oracle, at the row counts that move its chunks, slices and idle workgroups."""
    forced = K.npw_forms(c.C)[form]
    if forced:
        monkeypatch.setenv(K.ENV_NPW, str(forced))
    else:
        monkeypatch.delenv(K.ENV_NPW, raising=False)
    t, ref, yard, torch32 = block_links(c)
    got = run_block(c, t)
    plan = K.wgrad_plan(c.rows, c.C, True, forced)
    print(f"[{c.name} NPW {forced or 'unset'}] {plan}, idle workgroups {plan.idle}")
    part = K.block_partition_yardstick(c, t, torch32, forced) if c.rows >= K.PARTITION_ROWS else None
    check_all(block_reports(c, got, ref, yard, f"[{c.name} NPW {forced or 'unset'}]", part))


@pytest.mark.parametrize("name", [f"C{C}_off_last_tile" for C in K.FUSED_WIDTHS] + ["C32_off_last_tile_skip4", "C48"])
def test_block_outputs_of_a_sample_ignore_the_other_samples(name):
    """Rows of three samples share every 16-row tile: pre, act, o and skip of samples 1.. do not move by a bit when sample 0 changes."""
    c = next(c for c in K.BLOCK_CASES if c.name == name)
    assert c.B == 3
    t = block_links(c)[0]
    x2 = t["x"].clone()
    x2[:, 0] = torch.randn(c.L_in, c.C, generator=torch.Generator().manual_seed(5)) * 3
    outs = []
    for x in (t["x"], x2):
        _, _, pre, act, _, o, skip = block_forward(c, t, x)
        torch.cuda.synchronize()
        outs.append([v.cpu() for v in (pre, act, o.view, skip.view)])
    for k, a, b in zip(("pre", "act", "o", "skip"), *outs):
        assert torch.equal(a[:, 1:], b[:, 1:]), f"{k} of samples 1.. moved with sample 0"
        assert not torch.equal(a[:, 0], b[:, 0])


# ---- stacks that mix the arms -----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("c", K.STACK_CASES, ids=ids)
def test_stack_per_column(c):
    """`ops.wavenet_stack` with groups: blocks with a used skip run fused, the others (S = 0) unfused, handing d_o to one another
    through the d_x / d_scratch ping-pong; several blocks accumulate into one output."""
    t = K.stack_inputs(c)
    ref, yard = K.stack_link(c, t, F64), K.stack_link(c, t, F32)
    xd = dev(t["x"]).requires_grad_()
    params = [tuple(dev(p).requires_grad_() for p in blk) for blk in t["params"]]
    outs = ops.wavenet_stack(xd, params, list(c.dilations), c.T_skip, K.INV_STD, c.C, groups=list(c.groups))
    assert len(outs) == c.n_out
    sum((o * dev(g)).sum() for o, g in zip(outs, t["d_outs"])).backward()
    torch.cuda.synchronize()
    tag = f"[{c.name}]"
    reports = [K.compare(f"{tag} out{g}", o.detach().cpu(), y, r, check=False) for g, (o, y, r) in enumerate(zip(outs, yard["outs"], ref["outs"]))]
    reports.append(K.compare(f"{tag} d_x", xd.grad.cpu(), yard["d_x"], ref["d_x"], check=False))
    flat = [p for blk in params for p in blk]
    for i, (p, y, r) in enumerate(zip(flat, yard["grads"], ref["grads"])):
        name = f"{tag} block {i // 4} {K.BLOCK_ELEMENTS[i % 4]}"
        if i // 4 >= c.n_run:  # past the last used skip: the block is not run
            assert float(r.abs().max()) == 0.0 and float(p.grad.abs().max()) == 0.0, name
            continue
        reports.append(K.compare(name, p.grad.cpu(), y, r, "elements", check=False))
        if i % 4 >= 2 and (c.groups[i // 4] < 0 or i // 4 == c.n_run - 1):  # skip rows of an unused skip; residual rows of the last block
            rows = slice(c.C, None) if c.groups[i // 4] < 0 else slice(0, c.C)
            assert float(r[rows].abs().max()) == 0.0 and float(p.grad[rows].abs().max()) == 0.0, f"{name}: rows that reach no output"
    check_all(reports)


# ---- the causal first convolution ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("c", K.CONV_K2_CASES, ids=ids)
def test_conv1d_k2_per_column(c):
    """`blvm_conv1d_k2_fwd` and the four ways `blvm_conv1d_k2_bwd` is called: every output, no d_x, no dW (db through the column sum),
    db alone."""
    t = K.conv_k2_inputs(c)
    ref, yard = K.conv_k2_link(c, t, F64), K.conv_k2_link(c, t, F32)
    kind = "elements" if c.L_out == 1 else "columns"
    x, W, b, d_out = (dev(t[k]) for k in ("x", "W", "b", "d_out"))
    with torch.no_grad():
        out = ops.conv1d_k2(x, W, b, c.dilation)
    tag = f"[{c.name}]"
    reports = [K.compare(f"{tag} out", out.cpu(), yard["out"], ref["out"], kind, check=False)]
    for way, (need_dx, need_dW, need_db) in K.CONV_K2_WAYS.items():
        dW, db = (torch.zeros_like(W) if need_dW else None), (torch.zeros_like(b) if need_db else None)
        d_x = ops._conv1d_k2_bwd(x, W, d_out, c.dilation, need_dx, dW, db)
        torch.cuda.synchronize()
        assert (d_x is not None) == need_dx
        if need_dx:
            reports.append(K.compare(f"{tag} {way}: d_x", d_x.cpu(), yard["d_x"], ref["d_x"], kind, exact_zeros=True, check=False))
        if need_dW:
            reports.append(K.compare(f"{tag} {way}: dW", dW.cpu(), yard["dW"], ref["dW"], "elements", check=False))
        reports.append(K.compare(f"{tag} {way}: db", db.cpu(), yard["db"], ref["db"], "elements", check=False))
    # the autograd route picks its outputs by requires_grad: the input of the model's first convolution needs no gradient
    Wg, bg = W.clone().requires_grad_(), b.clone().requires_grad_()
    ops.conv1d_k2(x, Wg, bg, c.dilation).backward(d_out)
    reports.append(K.compare(f"{tag} autograd: dW", Wg.grad.cpu(), yard["dW"], ref["dW"], "elements", check=False))
    reports.append(K.compare(f"{tag} autograd: db", bg.grad.cpu(), yard["db"], ref["db"], "elements", check=False))
    check_all(reports)


# ---- scale_act ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("slope", K.SCALE_ACT_SLOPES)
@pytest.mark.parametrize("n", K.SCALE_ACT_N)
def test_scale_act_bitwise(n, slope):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g)
    x[:: 7] = 0.0
    x[3::11] = -0.0
    for scale in (1.0, K.INV_STD):
        with torch.no_grad():
            y = ops.scale_act(dev(x), scale, slope).cpu()
        want = K.scale_act_ref(x, scale, slope)
        assert torch.equal(y.view(torch.int32), want.view(torch.int32)), f"n = {n}, slope = {slope}, scale = {scale}"
