"""Cases, oracles, yardsticks and the comparison for K11 (csrc/convcoder.hip): the channel norm, the depthwise stencils and the
nearest-resample residual, per COLUMN, at the edges of the kernels' thread geometry and in the regimes a trained coder produces.
Used by test_convcoder_cases_cpu.py (no GPU: the oracles, the bars and the tables themselves) and test_gpu_convcoder_elements.py.

Everything here is time-major [L,B,C] float32 on the CPU, a (sample, channel) pair being a column n = b*C + c of the matrix [L, N].

ORACLE: float64, from the torch operators the reference builds its coders from (`nn.GroupNorm(C, C)`, `F.conv1d` /
`F.conv_transpose1d(groups=C)`, `F.interpolate(mode="nearest")`), gradients from autograd.  The fused links are compositions:
  `_dwconv_fwd/_bwd(in_affine=ss)`   y = [relu](conv(x*sc + sh)); dx is the gradient with respect to the TRANSFORMED input x*sc + sh
                                     (the norm's own backward follows as a separate link), dw and dbias as usual;
  `_chan_norm_stats`                 mr = [mean | rstd], and ss such that x*ss[0] + ss[1] equals the norm;
  `_chan_norm_bwd(relu_mask=True, dx_chan_sum=...)`   the input x = relu(z) is given as data, dx is the gradient with respect to z,
                                     dx_chan_sum[c] its sum over time and samples.
YARDSTICK: the same composition in float32 on the CPU (`dtype=torch.float32` of the same function): cancellation in fp32 is a property
of the input, and the yardstick says how much of it an input carries.
BAR of a slice: max(TIMES * max|yardstick - oracle| over the slice, FLOOR * rms(oracle over the slice)); a slice whose oracle is
identically zero must be exactly zero.  Activations and their gradients: one slice per column.  Parameter-like tensors (dw, dbias,
dgamma, dbeta, dx_chan_sum, and the statistics vectors): every element, against the rms of the whole tensor and the yardstick's error
at THAT element (`compare(..., yard_over="tensor")` takes the yardstick's worst element instead: the long-strip test's float32
atomic sums only, see `tiled_atomic_sum`).
`kernel_order_*`: float32 restatements of the kernels' own order of operations (float64 column sums rounded once, then float32,
fused multiply-adds down the taps) — a correct kernel's stand-in on the CPU, and the yardstick of the norm's y, affine, dx and
dgamma (KERNEL_ORDER_YARDSTICK, see `norm_kernel_order`)."""
import dataclasses

import torch
import torch.nn as nn
import torch.nn.functional as F

TIMES = 4.0  # tests/test_gpu_ctc.py: the same operation count in another order
FLOOR = 2e-5  # tests/test_gpu_convcoder.py: this family's documented bar
ROOM = 1e-2  # non-vacuity: TIMES * the yardstick's own error stays below this fraction of the slice's scale
FLIP_RATE = 1e-4  # ReLU mask bits that may differ from the float64 mask (each within the forward bar of its slice)
EPS = 1e-5  # nn.GroupNorm's default

# ---- thread geometry of csrc/convcoder.hip, each constant with the line it restates -----------------------------------------------
COLS_PER_LANE = 4  # "const int n = (blockIdx.x * 64 + lane) * 4;": one float4 per lane
LANES = 64  # "const int lane = threadIdx.x & 63"
WAVES = 4  # "wave = threadIdx.x >> 6" of a 256-thread workgroup; "for (int r = r0 + wave; r < r1; r += 4)"
COLS_PER_BLOCK = LANES * COLS_PER_LANE  # "const int cb = (N / 4 + 63) / 64;"
STRIP_R = 8  # "constexpr int R = 8;" in launch_stencil: per wave, outputs u (gather) or values of m = output row / stride (scatter)
STRIP_ROWS = WAVES * STRIP_R  # "(a.Ly + 4 * R - 1) / (4 * R)": per workgroup
STATS_MIN_ROWS = 64  # "pick_rows_per_block(L, cb, 64)": col_stats_kernel, masked_chan_sum_kernel
APPLY_MIN_ROWS = 32  # "pick_rows_per_block(L, cb, 32)": norm_apply_kernel, norm_bwd_apply_kernel
WGRAD_MIN_ROWS = 64  # "a.rows_per_block = pick_rows_per_block(a.LA, cb, 64);", "const int rows = a.rows_per_block / 4;" per wave
WGRAD_GENERIC_ROWS = 64  # "int rpb = 64;" in blvm_dwconv_bwd: rows of A per block of dw_wgrad_kernel
WGRAD_GENERIC_COLS = 64  # "const int col = blockIdx.x * 64 + (threadIdx.x & 63)" in dw_wgrad_kernel
STRIP_TAPS, STRIP_STRIDES = 5, (1, 2, 4)  # "a.k == 5 && a.d == 1 && (a.s == 1 || a.s == 2 || a.s == 4)"
WANT_BLOCKS = 4096  # "int want_blocks = (4096 + col_blocks - 1) / col_blocks;"


def rows_per_block(L, N, min_rows):
    """pick_rows_per_block of the host code."""
    cb = (N // COLS_PER_LANE + LANES - 1) // LANES
    want = (WANT_BLOCKS + cb - 1) // cb
    rpb = max((L + want - 1) // want, min_rows)
    return (rpb + 3) // 4 * 4


def is_strip(k, stride, dilation):
    return k == STRIP_TAPS and dilation == 1 and stride in STRIP_STRIDES


def conv_len(L_in, k, stride, dilation, transposed):
    k_eff = dilation * (k - 1) + 1
    return (L_in - 1) * stride + k_eff if transposed else (L_in - k_eff) // stride + 1


def tm(x_bct):  # [B,C,T] -> [T,B,C]
    return x_bct.permute(2, 0, 1).contiguous()


def bct(x_tm):  # [T,B,C] -> [B,C,T]
    return x_tm.permute(1, 2, 0)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------

REGIMES = ("ordinary", "post_relu", "constant", "padded", "ratio100", "ratio1000", "tiny_spread")
NONNEG = ("post_relu", "constant", "padded", "ratio100", "ratio1000", "tiny_spread")  # inputs a ReLU can have produced
# dx_chan_sum is compared where the ReLU mask really removes terms; with every x > 0 the channel sums of dx cancel identically
# (the oracle itself holds rounding noise of 1e-15 there) and there is nothing to compare against.  The constant columns of
# "constant" cancel the same way, at rstd = 1/sqrt(eps) = 316 times the size, and would leave only that noise to look at.
CHAN_SUM_REGIMES = ("post_relu", "padded")
# Tensors of the norm whose yardstick is `norm_kernel_order`, not torch's float32 GroupNorm: all that the once-rounded mean reaches
# (see there for the reason and test_convcoder_cases_cpu.py::test_cancelling_columns_need_the_kernel_order_yardstick for the figures).
KERNEL_ORDER_YARDSTICK = ("y", "affine", "dx", "dgamma")


def pad_rows(L):
    """Rows zeroed at EACH end by the padded forms (none when the tensor is too short to keep a live row)."""
    return min(max(1, L // 8), (L - 1) // 2) if L >= 3 else 0


def dead_columns(N):
    """post_relu: column 1 (dead inside a group of four whose other three are live), the whole of group 2, and the last column."""
    return sorted({1, N - 1} | {n for n in range(8, 12) if n < N})


SPIKE = 0.0625
"""Height of the single non-zero sample.  Behind the ReLU mask such a column keeps ONE gradient element, dy * eps / (var + eps) up to
the factors: the rest cancels.  At a height of 1.75 (var = 0.09) that is 1e-4 of the operands and the float32 yardstick's error is
3.7e-2 of the slice, above ROOM; at this height var = 1e-4 and the element keeps a tenth of the operands."""


def spike_column(N):
    return 2  # a single non-zero sample


def constant_columns(regime, L, N):
    if regime != "constant":
        return []
    return list(range(N)) if L == 1 else [n for n in range(N) if n % 2 == 0]


def make_x(regime, L, B, C, g):
    N = B * C
    r = torch.randn(L, N, generator=g)
    n = torch.arange(N)
    if regime == "ordinary":  # the existing tests' draw
        x = r * 3 + 1.5
    elif regime == "post_relu":
        x = torch.relu(r)
        x[:, dead_columns(N)] = 0.0
        x[:, spike_column(N)] = 0.0
        x[L // 2, spike_column(N)] = SPIKE
    elif regime == "constant":  # padding or silence through a 1x1 convolution with bias: the same value all the way down
        x = torch.relu(r)
        cols = constant_columns(regime, L, N)
        x[:, cols] = (0.25 + 0.375 * (n % 7).float())[cols]
    elif regime == "padded":  # `pad_level_tm`: zeros on the time axis
        x = torch.relu(r * 3 + 1.5)
        p = pad_rows(L)
        if p:
            x[:p], x[L - p :] = 0.0, 0.0
    elif regime in ("ratio100", "ratio1000"):  # mean / spread
        x = float(regime[5:]) * (1 + 0.125 * (n % 5).float()) + r
    elif regime == "tiny_spread":  # variance far below eps
        x = 0.7 + 1e-4 * r
    else:
        raise ValueError(regime)
    return x.view(L, B, C).contiguous()


def make_dy(kind, L, B, C, g):
    dy = torch.randn(L, B, C, generator=g)
    if kind == "padded":  # what a cropped transposed level sends back
        p = pad_rows(L)
        if p:
            dy[:p], dy[L - p :] = 0.0, 0.0
    return dy


@dataclasses.dataclass(frozen=True)
class NormCase:
    name: str
    B: int
    C: int
    L: int
    regime: str = "ordinary"
    dy: str = "randn"
    edge: str = ""
    seed: int = 0

    @property
    def N(self):
        return self.B * self.C


@dataclasses.dataclass(frozen=True)
class ConvCase:
    name: str
    B: int
    C: int
    L_in: int
    k: int = 5
    stride: int = 1
    dilation: int = 1
    transposed: bool = False
    bias: bool = True
    relu: bool = False
    regime: str = ""  # "": plain randn input, no affine; otherwise the norm-as-affine in front, on an input of that regime
    dy: str = "randn"
    edge: str = ""
    seed: int = 0
    zero_x: bool = False  # plain input with a stretch of zero rows at both ends: with no bias, pre-activations that are exactly zero

    @property
    def N(self):
        return self.B * self.C

    @property
    def m_total(self):  # rows m = output row / stride that the scatter strip of the FORWARD pass walks (transposed cases)
        return (self.L_out + self.stride - 1) // self.stride

    @property
    def L_out(self):
        return conv_len(self.L_in, self.k, self.stride, self.dilation, self.transposed)

    @property
    def LA(self):  # rows the weight-gradient kernels walk: conv output rows, or transposed input rows
        return self.L_in if self.transposed else self.L_out

    @property
    def strip(self):
        return is_strip(self.k, self.stride, self.dilation)


def _seed(*parts):
    h = 17
    for p in parts:
        for ch in str(p):
            h = (h * 131 + ord(ch)) % 2147483629
    return h


def _gamma_beta(C, g):
    """beta stays 0.2 away from zero: a constant column normalises to beta alone, which is then the whole scale of its slice, and
    torch's float32 GroupNorm (y = x*scale + shift) is off by an ulp of x*rstd there whatever beta is."""
    r = torch.randn(C, generator=g)
    return 1 + 0.3 * torch.randn(C, generator=g), torch.where(r < 0, -1.0, 1.0) * (0.2 + 0.3 * r.abs())


def dx_is_identically_zero(c: "NormCase"):
    """The norm of ONE row is beta whatever x is: its data gradient is identically zero, and the float64 autograd oracle holds only
    rounding noise (1e-16 of dy) there.  The kernel must give exactly 0.0; nothing else is compared."""
    return c.L == 1


def norm_inputs(c: NormCase):
    g = torch.Generator().manual_seed(_seed(c.name) + c.seed)
    x = make_x(c.regime, c.L, c.B, c.C, g)
    gamma, beta = _gamma_beta(c.C, g)
    return x, gamma, beta, make_dy(c.dy, c.L, c.B, c.C, g)


def conv_inputs(c: ConvCase):
    """x, w [C,k], bias or None, dy [L_out,B,C], affine [2,N] or None (the float64 statistics of x, rounded once: DATA for this link)."""
    g = torch.Generator().manual_seed(_seed(c.name) + c.seed)
    x = make_x(c.regime, c.L_in, c.B, c.C, g) if c.regime else torch.randn(c.L_in, c.B, c.C, generator=g)
    if c.zero_x:  # a zero stretch with zero bias: pre-activations that are exactly zero, under a DENSE upstream gradient
        p = pad_rows(c.L_in)
        if p:
            x[:p], x[c.L_in - p :] = 0.0, 0.0
    w = torch.randn(c.C, c.k, generator=g)
    bias = torch.randn(c.C, generator=g) if c.bias else None
    dy = make_dy(c.dy, c.L_out, c.B, c.C, g)
    affine = None
    if c.regime:
        gamma, beta = _gamma_beta(c.C, g)
        xd = x.double()
        mean, var = xd.mean(0), xd.var(0, unbiased=False)
        sc = (var + EPS).rsqrt() * gamma.double()
        affine = torch.stack([sc, beta.double() - mean * sc]).float().view(2, c.N).contiguous()
    return x, w, bias, dy, affine


# ---- oracles (dtype float64) and yardsticks (dtype float32) -----------------------------------------------------------------------


def norm_link(x, gamma, beta, dy, dtype, relu_mask=False, eps=EPS):
    """nn.GroupNorm(C, C) on x [L,B,C] (relu_mask: on relu(z), z = x) and its gradients.  `affine` is x*scale + shift evaluated in
    float64 from THIS dtype's scale and shift: what a consumer that normalises on load gets."""
    L, B, C = x.shape
    gn = nn.GroupNorm(C, C, eps=eps).to(dtype)
    with torch.no_grad():
        gn.weight.copy_(gamma)
        gn.bias.copy_(beta)
    with torch.enable_grad():
        z = bct(x).to(dtype).clone().requires_grad_()
        a = torch.relu(z) if relu_mask else z
        y = gn(a)
        y.backward(bct(dy).to(dtype))
    a = a.detach()
    mean, var = a.mean(2), a.var(2, unbiased=False)
    rstd = (var + eps).rsqrt()
    scale = rstd * gn.weight.detach()
    shift = gn.bias.detach() - mean * scale
    affine = a.double() * scale.double()[:, :, None] + shift.double()[:, :, None]
    return dict(y=tm(y.detach()), dx=tm(z.grad), dgamma=gn.weight.grad, dbeta=gn.bias.grad, dx_chan_sum=z.grad.sum((0, 2)),
                mean=mean.reshape(-1), rstd=rstd.reshape(-1), scale=scale.reshape(-1), shift=shift.reshape(-1), affine=tm(affine))  # fmt: skip


def norm_kernel_order(x, gamma, beta, dy, relu_mask=False, eps=EPS):
    """The kernels' own order in float32: column sums in float64 rounded ONCE to float32 (finalize_stats_kernel), then
    y = fma((x - mean) * rstd, gamma, beta), scale = rstd * gamma, shift = fma(-scale, mean, beta), and
    dx = (gamma * rstd) * fma(-xhat, s2/L, dy - s1/L) with s1, s2 float64 sums of float32 terms — the multiply-adds fused where the
    compiler fuses them for gfx950 (read from the kernels' code: v_fma_f32 / v_pk_fma_f32 in finalize_stats_kernel, norm_apply_kernel
    and norm_bwd_apply_kernel).
    `y` and `affine` take this restatement as their yardstick.  In a cancelling column (mean / spread of 1e3, or a spread far below
    sqrt(eps)) the whole error of a column is ONE or two roundings that all its rows share: of the mean, and of scale and shift.
    torch's float32 GroupNorm rounds other quantities (it evaluates x*scale + shift with moments of its own), so per column its error is
    below a quarter of the error of this order in a fixed fraction of the columns, whatever a kernel does; a correct kernel in the
    order below then misses TIMES x that yardstick (test_convcoder_cases_cpu.py measures it: ratios up to 4.1 in 1300 columns for
    `affine`, 1.9 for `y`, 1.4 for dx and 8.8 for an element of dgamma, which see the same mean through xhat).  The order below has the kernel's
    roundings, so it says what fp32 delivers in THIS order; the oracle stays torch's float64 GroupNorm."""
    L, B, C = x.shape
    N = B * C
    f = torch.float32
    x2, dy2 = x.reshape(L, N), dy.reshape(L, N)
    g, b = gamma.repeat(B), beta.repeat(B)
    xd = x2.double()
    mean64 = xd.sum(0) / L
    var64 = ((xd * xd).sum(0) / L - mean64 * mean64).clamp_min(0.0)
    eps = float(torch.tensor(eps, dtype=f))  # the ABI takes eps as a float: "var + (double)eps"
    m, rs = mean64.to(f), (1.0 / (var64 + eps).sqrt()).to(f)
    xhat = (x2 - m) * rs
    y = _fma(xhat, g, b)
    sc = rs * g
    sh = _fma(-sc, m, b)
    s1, s2 = dy2.double().sum(0), (dy2.double() * xhat.double()).sum(0)
    m1, m2 = (s1 / L).to(f), (s2 / L).to(f)
    dx = (g * rs) * _fma(-xhat, m2, dy2 - m1)
    if relu_mask:
        dx = torch.where(x2 > 0, dx, torch.zeros_like(dx))
    affine = xd * sc.double() + sh.double()
    return dict(y=y.view(L, B, C), dx=dx.view(L, B, C), dgamma=s2.view(B, C).sum(0).to(f), dbeta=s1.view(B, C).sum(0).to(f),
                dx_chan_sum=dx.view(L, B, C).sum((0, 1)), mean=m, rstd=rs, scale=sc, shift=sh, affine=affine.view(L, B, C))  # fmt: skip


def conv_link(c: ConvCase, x, w, bias, dy, dtype, affine=None, mask=None):
    """[relu](conv(x*sc + sh)) and its gradients; `pre` is the pre-activation.  mask [L_out,B,C] (bool): the ReLU derivative to use in
    the backward pass instead of this dtype's own (the kernel's, once its forward output has passed)."""
    L, B, C = x.shape
    xt = bct(x).to(dtype)
    if affine is not None:
        xt = xt * affine[0].view(B, C, 1).to(dtype) + affine[1].view(B, C, 1).to(dtype)
    fn = F.conv_transpose1d if c.transposed else F.conv1d
    with torch.enable_grad():
        xt = xt.detach().clone().requires_grad_()
        wt = w.to(dtype).view(C, 1, c.k).clone().requires_grad_()
        bt = bias.to(dtype).clone().requires_grad_() if bias is not None else None
        pre = fn(xt, wt, bt, stride=c.stride, dilation=c.dilation, groups=C)
        y = pre
        if c.relu:
            y = torch.relu(pre) if mask is None else pre * bct(mask).to(dtype)
        y.backward(bct(dy).to(dtype))
    return dict(y=tm(y.detach()), pre=tm(pre.detach()), dx=tm(xt.grad), dw=wt.grad.view(C, c.k),
                dbias=bt.grad if bt is not None else None)  # fmt: skip


def _fma(a, b, acc):  # float32 fused multiply-add: the product is exact in float64
    return (a.double() * b.double() + acc.double()).float()


def _stencil_f32(x, w, bias, Ly, k, s, d, scatter):
    """x [Lx,N], w [k,N], bias [N] or None: taps in ascending order, one fma each, as all four stencil kernels do."""
    Lx, N = x.shape
    acc = bias.expand(Ly, N).clone() if bias is not None else torch.zeros(Ly, N)
    for j in range(k):
        if not scatter:
            if Lx - 1 - j * d < 0:
                continue
            n = min(Ly, (Lx - 1 - j * d) // s + 1)
            acc[:n] = _fma(w[j], x[j * d : j * d + (n - 1) * s + 1 : s], acc[:n])
        else:
            if Ly - 1 - j * d < 0:
                continue
            n = min(Lx, (Ly - 1 - j * d) // s + 1)
            sl = slice(j * d, j * d + (n - 1) * s + 1, s)
            acc[sl] = _fma(w[j], x[:n], acc[sl])
    return acc


def conv_kernel_order(c: ConvCase, x, w, bias, dy, affine=None):
    """The stencil kernels' order in float32: x*sc + sh as ONE fma on in-range rows, taps ascending with one fma each; the data gradient
    as the other stencil form on the masked output gradient; dw and dbias as float32 sums."""
    L, B, C = x.shape
    N = B * C
    x2 = x.reshape(L, N)
    if affine is not None:
        x2 = _fma(x2, affine[0], affine[1])
    wn = w.t().repeat(1, B)  # [k,N]
    pre = _stencil_f32(x2, wn, bias.repeat(B) if bias is not None else None, c.L_out, c.k, c.stride, c.dilation, c.transposed)
    y = torch.relu(pre) if c.relu else pre
    g = dy.reshape(c.L_out, N)
    if c.relu:
        g = torch.where(y > 0, g, torch.zeros_like(g))
    dx = _stencil_f32(g, wn, None, L, c.k, c.stride, c.dilation, not c.transposed)
    a, bm = (x2, g) if c.transposed else (g, x2)  # dw[c,j] = sum_u A[u] * Bm[u*s + j*d]
    dw = torch.zeros(c.k, N)
    for j in range(c.k):
        n = min(a.shape[0], (bm.shape[0] - 1 - j * c.dilation) // c.stride + 1) if bm.shape[0] - 1 - j * c.dilation >= 0 else 0
        if n > 0:
            dw[j] = (a[:n] * bm[j * c.dilation : j * c.dilation + (n - 1) * c.stride + 1 : c.stride]).sum(0)
    return dict(y=y.view(c.L_out, B, C), pre=pre.view(c.L_out, B, C), dx=dx.view(L, B, C), dw=dw.view(c.k, B, C).sum(1).t().contiguous(),
                dbias=g.view(c.L_out, B, C).sum((0, 1)) if bias is not None else None)  # fmt: skip


def block_sums(t, rows):
    """float32 sums of t [L,...] over consecutive blocks of `rows` rows: what one workgroup adds to a per-channel total."""
    L = t.shape[0]
    R = (L + rows - 1) // rows
    pad = torch.zeros(R * rows - L, *t.shape[1:], dtype=t.dtype)
    return torch.cat([t, pad]).view(R, rows, *t.shape[1:]).sum(1)


def tiled_atomic_sum(partials, tiles):
    """The per-channel total of `tiles` identical tiles, per tile: the workgroups' partial sums [R,...] added one after another in
    float32, tile after tile.  The order of float32 atomics is free; this is one admissible order.  It is the yardstick of the
    long-strip test's float32 per-channel sums: identical tiles add the SAME partials again and again, so the roundings of the running
    total do not average out as they do over independent data, and 16 000 of them weigh 5e-5 of the total where the torch float32
    composition of one tile shows 5e-6.  Which element a given order of addition hits hardest differs from order to order (measured on
    an MI355X: dbias element 16 off by 6.4e-3 where this order is off by 3.3e-4 there and by 4.6e-3 at its worst element), so these
    sums, and only these, are compared with `compare(..., yard_over="tensor")`."""
    acc = torch.zeros_like(partials[0])
    for _ in range(tiles):
        for r in range(partials.shape[0]):
            acc += partials[r]
    return acc / tiles


def unreached_outputs(c: ConvCase):
    """Output rows of a transposed convolution that no tap of any input row reaches: they hold the bias alone."""
    hit = {r * c.stride + j * c.dilation for r in range(c.L_in) for j in range(c.k)}
    return [t for t in range(c.L_out) if t not in hit] if c.transposed else []


def unread_rows(c: ConvCase):
    """Input rows that a strided convolution never reads: their data gradient is exactly zero."""
    if c.transposed:
        return []
    read = {u * c.stride + j * c.dilation for u in range(c.L_out) for j in range(c.k)}
    return [r for r in range(c.L_in) if r not in read]


def resample_link(y, x, dout, dtype=torch.float32):
    """y + nearest-resampled x, and the gradients; float32 by default: the forward is a single add, compared bit for bit."""
    yt, xt = bct(y).to(dtype).clone().requires_grad_(), bct(x).to(dtype).clone().requires_grad_()
    Ly, Lx = y.shape[0], x.shape[0]
    with torch.enable_grad():
        out = yt + (F.interpolate(xt, size=Ly, mode="nearest") if Lx != Ly else xt)
        out.backward(bct(dout).to(dtype))
    return dict(out=tm(out.detach()), dy=tm(yt.grad), dx=tm(xt.grad))


# ---- the comparison ---------------------------------------------------------------------------------------------------------------


@dataclasses.dataclass
class Report:
    name: str
    ratio: float  # worst kernel error over its bar
    bars: torch.Tensor  # per slice
    line: str
    failures: list

    @property
    def ok(self):
        return not self.failures


def _slices(t, kind):
    t = t.detach().double().cpu()
    return t.reshape(t.shape[0], -1) if kind == "columns" else t.reshape(1, -1)


def yardstick_room(yard, ref, kind="columns"):
    """Worst TIMES * (yardstick's own error) / (scale of the slice): at most ROOM, or a wrong element of the size of the data hides."""
    y, r = _slices(yard, kind), _slices(ref, kind)
    err = (y - r).abs().amax(0) if kind == "columns" else (y - r).abs()[0]
    scale = r.pow(2).mean(0).sqrt() if kind == "columns" else r.pow(2).mean().sqrt().expand(r.shape[1])
    live = scale > 0
    return float((TIMES * err[live] / scale[live]).max()) if bool(live.any()) else 0.0


def compare(name, got, yard, ref, kind="columns", exact_zeros=False, check=True, yard_over="slice"):
    """got (kernel), yard (float32 yardstick) against ref (float64).  kind "columns": [L,...] tensors, one slice per column;
    "elements": every element against the rms of the whole tensor and the yardstick's error at that element (yard_over="tensor": the
    yardstick's worst element, for sums whose order of addition is free on the device).  Prints the worst slice, then asserts (check=False: returns
    the Report with its failures instead)."""
    assert got.shape == ref.shape == yard.shape, f"{name}: shapes {tuple(got.shape)} / {tuple(yard.shape)} / {tuple(ref.shape)}"
    g, y, r = _slices(got, kind), _slices(yard, kind), _slices(ref, kind)
    failures = []
    if not bool(torch.isfinite(g).all()):
        failures.append(f"{name}: non-finite values")
        g = torch.nan_to_num(g, nan=float("inf"))
    if kind == "columns":
        err, err_y, scale = (g - r).abs().amax(0), (y - r).abs().amax(0), r.pow(2).mean(0).sqrt()
        zero = (r == 0).all(0)
        nonzero_got = (g != 0).any(0)
    else:
        err, err_y = (g - r).abs()[0], (y - r).abs()[0]
        if yard_over == "tensor":
            err_y = err_y.max().expand(r.shape[1])
        scale = r.pow(2).mean().sqrt().expand(r.shape[1])
        zero = (r == 0).all().expand(r.shape[1])
        nonzero_got = g[0] != 0
    bars = torch.maximum(TIMES * err_y, FLOOR * scale)
    for n in torch.nonzero(zero & nonzero_got).flatten().tolist()[:4]:
        failures.append(f"{name}[slice {n}]: the oracle is identically zero, the kernel is not (max |value| {float(g[:, n].abs().max()):.3e})")
    if exact_zeros:
        bad = (r == 0) & (g != 0)
        if bool(bad.any()):
            i = torch.nonzero(bad)[0].tolist()
            failures.append(f"{name}: {int(bad.sum())} elements are not exactly zero where the oracle is, first at {i} = {float(g[i[0], i[1]]):.3e}")
    live = ~zero
    ratio, line = 0.0, f"{name}: every slice is identically zero"
    if bool(live.any()):
        q = torch.where(live, err / bars.clamp_min(1e-300), torch.zeros_like(err))
        n = int(q.argmax())
        ratio = float(q[n])
        line = (f"{name}: kernel {float(err[n]):.3e}  yardstick {float(err_y[n]):.3e}  bar {float(bars[n]):.3e}  ratio {ratio:.3f}"
                f"  (slice {n} of {q.numel()}, scale {float(scale[n]):.3e})")  # fmt: skip
        over = torch.nonzero(q > 1.0).flatten().tolist()
        for n in over[:4]:
            failures.append(f"{name}[slice {n}]: error {float(err[n]):.3e} above the bar {float(bars[n]):.3e} "
                            f"(yardstick {float(err_y[n]):.3e}, scale {float(scale[n]):.3e}); {len(over)} slices in all")  # fmt: skip
    print(line)
    rep = Report(name, ratio, bars, line, failures)
    if check:
        assert rep.ok, "\n".join(failures)
    return rep


def mask_flips(name, y_got, pre_ref, fwd_bars, check=True):
    """Elements where the kernel's ReLU mask (y > 0) differs from the float64 one (pre > 0).  Each must have a float64 pre-activation no
    larger than the forward bar of its column, and there may be at most FLIP_RATE of them.  Returns the count."""
    g, p = _slices(y_got, "columns"), _slices(pre_ref, "columns")
    flip = (g > 0) != (p > 0)
    count = int(flip.sum())
    outside = flip & (p.abs() > fwd_bars[None, :])
    print(f"{name}: {count} mask bits of {flip.numel()} differ from the float64 mask")
    failures = []
    if bool(outside.any()):
        i = torch.nonzero(outside)[0].tolist()
        failures.append(f"{name}: mask differs at {i} where the float64 pre-activation is {float(p[i[0], i[1]]):.3e}, bar {float(fwd_bars[i[1]]):.3e}")
    if count > FLIP_RATE * flip.numel():
        failures.append(f"{name}: {count} mask bits differ, more than {FLIP_RATE} of {flip.numel()}")
    if check:
        assert not failures, "\n".join(failures)
    return count if check else (count, failures)


# ---- the case tables --------------------------------------------------------------------------------------------------------------

COLUMNS = [(1, 4, "a single lane"), (7, 36, "one group short of a block; C no power of two: a wave's lanes wrap across samples"),
           (2, 128, "exactly one block"), (5, 52, "the second block with one live lane"), (193, 4, "four blocks, the last with one lane")]  # fmt: skip
ROWS_AT = (5, 52)  # every row list runs at N = 260
NORM_ROWS = [1, 3, 4, 5, 63, 64, 65, 129]
GATHER_OUT_ROWS = [1, 8, 9, 32, 33]
SCATTER_IN_ROWS = [1, 2, 8, 9, 32, 33]
WGRAD_ROWS = [1, 16, 17, 64, 65, 129]
GENERIC = [(3, 1, 1), (5, 3, 1), (5, 2, 2), (8, 1, 1), (1, 1, 1), (3, 4, 1)]  # (k, stride, dilation)


def _norm_cases():
    B, C = ROWS_AT
    out = [NormCase(f"rows{L}", B, C, L, edge=f"L = {L}") for L in NORM_ROWS]
    out += [NormCase(f"cols{b * c}", b, c, 65, edge=e) for b, c, e in COLUMNS if (b, c) != ROWS_AT]
    out += [NormCase(f"{r}", B, C, 65, regime=r, edge=f"regime {r}") for r in REGIMES[1:]]
    out += [NormCase("constant_L1", B, C, 1, regime="constant", edge="a constant column of one row"),
            NormCase("ratio1000_L5", B, C, 5, regime="ratio1000", edge="mean / spread = 1000 over five rows"),
            NormCase("tiny_spread_L5", B, C, 5, regime="tiny_spread", edge="variance far below eps over five rows"),
            NormCase("post_relu_N4", 1, 4, 33, regime="post_relu", edge="dead, spike and live columns in one lane"),
            NormCase("ordinary_dy_padded", B, C, 65, dy="padded", edge="upstream gradient with a zeroed stretch at both ends"),
            NormCase("post_relu_dy_padded", B, C, 64, regime="post_relu", dy="padded", edge="the same behind a ReLU")]  # fmt: skip
    return out


def _gather_in(L_out, s, slack=0):
    return (L_out - 1) * s + STRIP_TAPS + slack


def _conv_cases():
    B, C = ROWS_AT
    out = []
    # gather strips (Conv1d forward; its data gradient is the scatter strip over L_out rows, its weight gradient walks L_out rows)
    for s in STRIP_STRIDES:
        for i, Lo in enumerate(GATHER_OUT_ROWS):
            slack = s - 1 if (s > 1 and Lo == 9) else 0  # once per stride: (L_in - 5) % stride != 0, trailing rows never read
            out.append(ConvCase(f"gather_s{s}_out{Lo}", B, C, _gather_in(Lo, s, slack), stride=s, relu=bool((i + s) % 2), bias=bool(i % 3),
                                edge=f"{Lo} outputs" + (f", {slack} unread rows" if slack else "")))  # fmt: skip
    # scatter strips (ConvTranspose1d forward; its data gradient is the gather strip with L_in outputs)
    for s in STRIP_STRIDES:
        for i, Li in enumerate(SCATTER_IN_ROWS):
            out.append(ConvCase(f"scatter_s{s}_in{Li}", B, C, Li, stride=s, transposed=True, relu=bool((i + s + 1) % 2), bias=bool((i + 1) % 3),
                                edge=f"{Li} transposed input rows"))  # fmt: skip
    # the same kernel counted the way it hands out work: R values of m = output row / stride per wave, m_total = ceil(L_out / stride)
    for s in STRIP_STRIDES:
        for mt in (STRIP_R, STRIP_R + 1, STRIP_ROWS, STRIP_ROWS + 1):
            Li = mt - {1: 4, 2: 2, 4: 1}[s]  # ceil(((L_in - 1) * s + 5) / s)
            if Li not in SCATTER_IN_ROWS:
                out.append(ConvCase(f"scatter_s{s}_m{mt}", B, C, Li, stride=s, transposed=True, relu=bool((mt + s) % 2), bias=bool(mt % 3),
                                    edge=f"m_total = {mt}: a wave or a workgroup exactly full, or one row over"))  # fmt: skip
    # weight-gradient strips: LA rows
    for LA in WGRAD_ROWS[1:]:
        s = STRIP_STRIDES[LA % 3]
        out.append(ConvCase(f"wgrad_conv_s{s}_LA{LA}", B, C, _gather_in(LA, s), stride=s, relu=bool(LA % 2), edge=f"LA = {LA}"))
        out.append(ConvCase(f"wgrad_tconv_s{s}_LA{LA}", B, C, LA, stride=s, transposed=True, relu=not LA % 2, edge=f"LA = {LA}"))
    # columns, at one length per strip kernel
    for b, c, e in COLUMNS:
        if (b, c) != ROWS_AT:
            out.append(ConvCase(f"strip_conv_cols{b * c}", b, c, _gather_in(33, 2), stride=2, relu=True, edge=e))
            out.append(ConvCase(f"strip_tconv_cols{b * c}", b, c, 33, stride=2, transposed=True, relu=True, edge=e))
    # exactly-zero pre-activations: a zero input stretch, no bias
    out.append(ConvCase("zero_stretch_conv", B, C, 72, stride=1, bias=False, relu=True, zero_x=True, edge="pre-activations exactly zero under a non-zero upstream gradient"))
    out.append(ConvCase("zero_stretch_tconv", B, C, 40, stride=2, transposed=True, bias=False, relu=True, zero_x=True, edge="pre-activations exactly zero under a non-zero upstream gradient"))
    # generic kernels
    for i, (k, s, d) in enumerate(GENERIC):
        for t in (False, True):
            L = 37 if not t else 13
            out.append(ConvCase(f"generic_{'t' if t else ''}conv_k{k}s{s}d{d}", B, C, L, k, s, d, t, bias=bool((i + t) % 2), relu=bool((i // 2 + t) % 2),
                                edge="generic kernels" + (", outputs no tap reaches" if t and s > (k - 1) * d + 1 else "")))  # fmt: skip
    for t in (False, True):  # the flag combinations the alternation above leaves out, both directions
        out.append(ConvCase(f"generic_{'t' if t else ''}conv_nobias_relu", B, C, 21, 3, 4, 1, t, bias=False, relu=True, edge="no bias: null dbias, no masked column sum"))
        out.append(ConvCase(f"generic_{'t' if t else ''}conv_bias_relu", B, C, 21, 3, 4, 1, t, bias=True, relu=True, edge="relu(bias) where no tap reaches"))
        out.append(ConvCase(f"generic_{'t' if t else ''}conv_bias_plain", B, C, 21, 3, 4, 1, t, bias=True, relu=False, edge="bias where no tap reaches"))
        out.append(ConvCase(f"generic_{'t' if t else ''}conv_nobias_plain", B, C, 70 if t else 197, 5, 3, 1, t, bias=False, relu=False, edge="no bias; LA = 70 / 65: two row blocks of the generic weight gradient"))
        for b, c, e in COLUMNS + [(1, 68, "the generic weight gradient's second column block, four live columns")]:
            if (b, c) != ROWS_AT:
                out.append(ConvCase(f"generic_{'t' if t else ''}conv_cols{b * c}", b, c, 19, 3, 1, 1, t, relu=bool(b % 2), edge=e))
    # the norm-as-affine in front of the stencil, one regime per case
    for t in (False, True):
        for i, r in enumerate(REGIMES):
            s = STRIP_STRIDES[(i + t) % 3]
            # (tiny_spread without the ReLU: every pre-activation of a column is bias + beta * sum(w) to within 3 %, and where that is
            # just above zero the ReLU leaves a column whose scale is a hundredth of its float32 error)
            out.append(ConvCase(f"affine_{'t' if t else ''}conv_{r}", B, C, 41 if not t else 19, stride=s, transposed=t, relu=r != "tiny_spread", regime=r,
                                dy="padded" if i % 2 else "randn", edge=f"in_scale / in_shift on {'A' if t else 'Bm'}, regime {r}"))  # fmt: skip
        out.append(ConvCase(f"affine_{'t' if t else ''}conv_generic", 1, 68, 23, 3, 2, 1, t, relu=True, regime="post_relu", edge="affine in the generic kernels, N = 68"))
        out.append(ConvCase(f"affine_{'t' if t else ''}conv_nobias", B, C, 33, stride=2, transposed=t, bias=False, relu=False, regime="ordinary", edge="affine, no bias, no ReLU"))
    return out


NORM_CASES = _norm_cases()
CONV_CASES = _conv_cases()
RESAMPLE_CASES = [(100, 100), (100, 48), (48, 99), (7, 31), (1000, 251), (3, 3 * 16 + 4), (1, 7), (7, 1), (33, 32), (32, 33)]  # (Lx, Ly)

# The long-strip arm: rows_per_block above its minimum needs L > min_rows * ceil(4096 / column blocks).
LONG_B, LONG_C, LONG_L = 256, 64, 4100


def edge_requirements():
    """Every edge class the tables must hit, computed from the geometry constants: {class name: (predicate over a case, table)}."""
    W, Q, P = WAVES, COLS_PER_LANE, COLS_PER_BLOCK
    req = {}
    for n, what in [(Q, "a single lane"), (P - Q, "one group short of a block"), (P, "one full block"), (P + Q, "a second block with one lane"),
                    (3 * P + Q, "several blocks")]:  # fmt: skip
        req[f"norm: N = {n} ({what})"] = (lambda c, n=n: c.N == n, NORM_CASES)
        for t in (False, True):
            req[f"strip stencil {'transposed' if t else 'plain'}: N = {n} ({what})"] = (lambda c, n=n, t=t: c.N == n and c.strip and c.transposed == t and not c.regime, CONV_CASES)
            req[f"generic stencil {'transposed' if t else 'plain'}: N = {n} ({what})"] = (lambda c, n=n, t=t: c.N == n and not c.strip and c.transposed == t, CONV_CASES)
    for t in (False, True):
        req[f"generic weight gradient {'transposed' if t else 'plain'}: N = {WGRAD_GENERIC_COLS + Q}"] = (
            lambda c, t=t: c.N == WGRAD_GENERIC_COLS + Q and not c.strip and c.transposed == t, CONV_CASES)
        req[f"generic weight gradient {'transposed' if t else 'plain'}: a second row block"] = (
            lambda c, t=t: WGRAD_GENERIC_ROWS < c.LA <= 2 * WGRAD_GENERIC_ROWS and not c.strip and c.transposed == t, CONV_CASES)
        req[f"exactly-zero pre-activations {'transposed' if t else 'plain'}"] = (lambda c, t=t: c.zero_x and c.relu and not c.bias and c.transposed == t, CONV_CASES)
    for L in (1, W - 1, W, W + 1, STATS_MIN_ROWS - 1, STATS_MIN_ROWS, STATS_MIN_ROWS + 1, 2 * STATS_MIN_ROWS + 1, 2 * APPLY_MIN_ROWS, 2 * APPLY_MIN_ROWS + 1):
        req[f"norm: L = {L}"] = (lambda c, L=L: c.L == L and c.N == P + Q and c.regime == "ordinary", NORM_CASES)
    for s in STRIP_STRIDES:
        for Lo in (1, STRIP_R, STRIP_R + 1, STRIP_ROWS, STRIP_ROWS + 1):
            req[f"gather strip, stride {s}: {Lo} outputs"] = (lambda c, s=s, Lo=Lo: c.strip and not c.transposed and c.stride == s and c.L_out == Lo and c.N == P + Q, CONV_CASES)
        for Li in (1, 2, STRIP_R, STRIP_R + 1, STRIP_ROWS, STRIP_ROWS + 1):
            req[f"scatter strip, stride {s}: {Li} input rows"] = (lambda c, s=s, Li=Li: c.strip and c.transposed and c.stride == s and c.L_in == Li and c.N == P + Q, CONV_CASES)
        for mt in (STRIP_R, STRIP_R + 1, STRIP_ROWS, STRIP_ROWS + 1):
            req[f"scatter strip, stride {s}: m_total = {mt}"] = (lambda c, s=s, mt=mt: c.strip and c.transposed and c.stride == s and c.m_total == mt and c.N == P + Q, CONV_CASES)
        if s > 1:
            req[f"gather strip, stride {s}: trailing rows never read"] = (lambda c, s=s: c.strip and c.stride == s and bool(unread_rows(c)), CONV_CASES)
    for t in (False, True):
        for LA in (1, WGRAD_MIN_ROWS // W, WGRAD_MIN_ROWS // W + 1, WGRAD_MIN_ROWS, WGRAD_MIN_ROWS + 1, 2 * WGRAD_MIN_ROWS + 1):
            req[f"weight-gradient strip {'transposed' if t else 'plain'}: LA = {LA}"] = (lambda c, t=t, LA=LA: c.strip and c.transposed == t and c.LA == LA and c.N == P + Q, CONV_CASES)
        for k, s, d in GENERIC:
            req[f"generic {'transposed' if t else 'plain'}: k={k} stride={s} dilation={d}"] = (
                lambda c, t=t, k=k, s=s, d=d: (c.k, c.stride, c.dilation, c.transposed) == (k, s, d, t), CONV_CASES)
        for bias in (False, True):
            for relu in (False, True):
                req[f"generic {'transposed' if t else 'plain'}: bias={bias} relu={relu}"] = (
                    lambda c, t=t, bias=bias, relu=relu: not c.strip and not c.regime and (c.transposed, c.bias, c.relu) == (t, bias, relu), CONV_CASES)
                req[f"strip {'transposed' if t else 'plain'}: bias={bias} relu={relu}"] = (
                    lambda c, t=t, bias=bias, relu=relu: c.strip and (c.transposed, c.bias, c.relu) == (t, bias, relu), CONV_CASES)
        for r in REGIMES:
            req[f"affine {'transposed' if t else 'plain'}: regime {r}"] = (lambda c, t=t, r=r: c.strip and c.regime == r and c.transposed == t, CONV_CASES)
        req[f"affine {'transposed' if t else 'plain'}: generic kernels"] = (lambda c, t=t: bool(c.regime) and not c.strip and c.transposed == t, CONV_CASES)
    req["transposed: outputs that no tap reaches, with bias"] = (lambda c: bool(unreached_outputs(c)) and c.bias and not c.relu, CONV_CASES)
    req["transposed: outputs that no tap reaches, relu(bias)"] = (lambda c: bool(unreached_outputs(c)) and c.bias and c.relu, CONV_CASES)
    req["eight taps"] = (lambda c: c.k == 8, CONV_CASES)
    for r in REGIMES:
        req[f"norm: regime {r}"] = (lambda c, r=r: c.regime == r, NORM_CASES)
    req["norm: a constant column of one row"] = (lambda c: c.regime == "constant" and c.L == 1, NORM_CASES)
    req["norm: upstream gradient with zeroed ends"] = (lambda c: c.dy == "padded", NORM_CASES)
    return req
