"""GPU (MI355X): the likelihood heads (K7 DMoL, K7b Gaussian mixture, K7c Gaussian) and the KL (K8) per frame / per element
in trained-model regimes, against the CPU oracle in float64 on the crafted inputs of tests/golden/heads_stress.npz
(oracle/gen_golden.py::gen_heads_stress; tests/test_oracle_golden.py pins the float32 oracle to the reference's values and
gradients on the same inputs).

Bar, per frame (forward ll) and per element (gradients): |hip - truth| <= max(4 |ref32 - truth|, floor), truth = the float64
oracle, ref32 = the reference's float32 result (the fixture; the float32 oracle for random-W cases).  The floor covers frames
where the float32 reference happens to be exact.  It is an fp32 error bound of the computation, not tuned against mutants:
  * a frame's log-likelihood is a chain of ~60 roundings (hardware exp / log / rcp to ~1 ulp, sums of 10 terms) over
    quantities of size at most S_f = 1 + |ll| + max |logit| (|m| of the dominant component is below |ll| + the logit spread),
    so  floor_ll = 64 u S_f,  u = 2^-24;
  * a gradient entry is a responsibility (relative error ~ u S_f) times a per-component factor (a few roundings, terms no
    larger than the largest entry of its group of ten: locations | log-scales); a logit's entry is the difference of a
    responsibility and a softmax weight, so its terms are those two.  floor_g = 64 u S_f (|g| + term size) + 2^-100
    (responsibilities / softmax weights under 2^-126 flush to 0);
  * dW, db are sums over frames: each frame contributes its floor_g, plus 2 n u per term of an n-term fp32 accumulation;
  * KL sums: 64 u times the sum of |KL| over the utterance; KL gradients: 64 u |coef| times the sum of the magnitudes of the
    terms of each closed form.
Assertion messages name the quantity (ll, lp, d_dec, dW, db, kld, kld_fn, d_mu_q ...), the worst frame and the margin
(err / bar at the worst frame; <= 1 passes)."""
import os

import numpy as np
import pytest
import torch

import blvm_oracle as O
from blvm import _hip, ops

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0**-24
ABS = 2.0**-100
SENTINEL = 12345.0
LIB = None


@pytest.fixture(scope="module", autouse=True)
def _require_hip():
    global LIB
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    LIB = _hip.load()
    assert LIB.blvm_device_ok() == 1, "libblvm_hip: no gfx950 device visible"


@pytest.fixture(scope="module")
def hs():
    return {k: v for k, v in np.load(os.path.join(GOLDEN, "heads_stress.npz")).items()}


def T(a):
    return torch.from_numpy(np.asarray(a))


def p_(t):
    return _hip.ptr(t)


def check_bar(name, got, truth, ref32, floor, frame_of=None):
    """Per-element bar; the message names the quantity, the worst frame and its margin."""
    got, truth, ref32 = got.detach().double().cpu().reshape(-1), truth.detach().double().reshape(-1), ref32.detach().double().reshape(-1)
    floor = floor.double().reshape(-1)
    err = (got - truth).abs()
    bar = torch.maximum(4 * (ref32 - truth).abs(), floor)
    ratio = torch.nan_to_num(err / bar, nan=float("inf"))
    i = int(ratio.argmax())
    where = frame_of(i) if frame_of is not None else i
    msg = (f"{name}: worst at {where}: hip {float(got[i]):.9g} truth {float(truth[i]):.9g} err {float(err[i]):.3e} bar {float(bar[i]):.3e} "
           f"(ref32 err {float((ref32[i] - truth[i]).abs()):.3e}, floor {float(floor[i]):.3e}); margin err/bar {float(ratio[i]):.3g}")
    assert float(ratio[i]) <= 1.0, msg
    return float(ratio[i])


# ----------------------------------------------------------------------------------------------------------------------
# frame layout: B utterances of Tp*S frames (the last S // 2 beyond T), ragged lengths, garbage in every padded frame
# ----------------------------------------------------------------------------------------------------------------------


def frames_layout(B, Tp, S):
    T_ = Tp * S - S // 2
    x_sl = torch.tensor([max(1, T_ - (k * T_) // (B + 1) - (k % 3)) for k in range(B)])
    x_sl[0] = T_
    tau = torch.arange(Tp * S)
    valid = (tau.unsqueeze(0) < torch.minimum(x_sl, torch.tensor(T_)).unsqueeze(1))  # [B, Tp*S]
    return T_, x_sl, valid


def to_rows(fr, B, Tp, S, layout):
    """batch-major frames [B, Tp*S, F] -> kernel rows [rows, S*F]."""
    F = fr.shape[-1]
    if layout == 0:
        return fr.reshape(B * Tp, S * F)
    return fr.reshape(B, Tp, S * F).transpose(0, 1).reshape(Tp * B, S * F)


def from_rows(d, B, Tp, S, layout, F):
    d = d.detach().cpu()
    if layout == 0:
        return d.reshape(B, Tp * S, F)
    return d.reshape(Tp, B, S * F).transpose(0, 1).reshape(B, Tp * S, F)


def dev_buf(host, unaligned):
    """Contiguous device copy; unaligned: starts 4 bytes past a 16-byte boundary (a view one float into its buffer)."""
    host = host.contiguous().view(-1)
    if not unaligned:
        return host.to(DEV).view(-1)
    buf = torch.empty(host.numel() + 1, device=DEV)
    v = buf[1:]
    v.copy_(host.to(DEV))
    assert v.data_ptr() % 16 == 4
    return v


def run_head_abi(kind, dec_rows, W, bias, y, x_sl, g_b, layout, B, T_, Tp, S, bins=2**16, beta=1.0, sd_eps=0.0, unaligned=False):
    """Forward (ll_twise over a sentinel, per-utterance fp64 sums) and backward (d_dec, d_par) through the C ABI."""
    F = dec_rows.shape[1] // S
    dec = dev_buf(dec_rows, unaligned)
    Wd = W.contiguous().to(DEV) if W is not None else None
    bd = bias.contiguous().to(DEV) if bias is not None else None
    yd, xs, gb = y.contiguous().to(DEV), x_sl.to(DEV, torch.int32), g_b.float().to(DEV)
    lp = torch.zeros(B, device=DEV, dtype=torch.float64)
    ll = torch.full((B, T_), SENTINEL, device=DEV)
    d_dec = dev_buf(torch.full((dec.numel(),), float("nan")), unaligned)
    d_par = dev_buf(torch.full((dec.numel(),), float("nan")), unaligned) if W is not None else None
    a = (p_(dec), layout, p_(Wd), p_(bd), p_(yd), p_(xs))
    if kind == "dmol":
        _hip.check(LIB.blvm_dmol_fwd(*a, B, T_, Tp, S, 10, bins, -7.0, p_(lp), p_(ll), _hip.stream_ptr()), "dmol_fwd")
        _hip.check(LIB.blvm_dmol_bwd(*a, p_(gb), B, T_, Tp, S, 10, bins, -7.0, p_(d_dec), p_(d_par), _hip.stream_ptr()), "dmol_bwd")
    elif kind == "gmm":
        _hip.check(LIB.blvm_gmm_fwd(*a, B, T_, Tp, S, 10, beta, sd_eps, p_(lp), p_(ll), _hip.stream_ptr()), "gmm_fwd")
        _hip.check(LIB.blvm_gmm_bwd(*a, p_(gb), B, T_, Tp, S, 10, beta, sd_eps, p_(d_dec), p_(d_par), _hip.stream_ptr()), "gmm_bwd")
    else:
        _hip.check(LIB.blvm_gauss_head_fwd(*a, B, T_, Tp, S, beta, sd_eps, p_(lp), p_(ll), _hip.stream_ptr()), "gauss_fwd")
        _hip.check(LIB.blvm_gauss_head_bwd(*a, p_(gb), B, T_, Tp, S, beta, sd_eps, p_(d_dec), p_(d_par), _hip.stream_ptr()), "gauss_bwd")
    torch.cuda.synchronize()
    d_par = d_par.view(B * Tp, S * F) if d_par is not None else None
    return ll.cpu(), lp.cpu(), d_dec.view(B * Tp, S * F), d_par


# ----------------------------------------------------------------------------------------------------------------------
# float64 truth per frame
# ----------------------------------------------------------------------------------------------------------------------


def head_ll(kind, par, y, bins, beta, sd_eps):
    """Per-frame log-likelihood of head outputs par [n, F] (any dtype) for targets y [n]."""
    if kind == "dmol":
        lg, lc, ls = O.dmol_head(par, torch.eye(30, dtype=par.dtype), torch.zeros(30, dtype=par.dtype))
        return O.dmol_ll(y.unsqueeze(1), lg, lc, ls, bins)
    if kind == "gmm":
        sd = torch.nn.functional.softplus(par[:, 20:], beta=beta) + sd_eps
        return O.gaussian_mixture_ll(y.unsqueeze(1), par[:, :10], par[:, 10:20].unsqueeze(1), sd.unsqueeze(1), epsilon=0)
    return O.gaussian_ll(y, par[:, 0], torch.nn.functional.softplus(par[:, 1], beta=beta) + sd_eps, epsilon=0)


def head_truth(kind, par, y, bins, beta, sd_eps, dtype=torch.float64):
    p = par.to(dtype).clone().requires_grad_(True)
    ll = head_ll(kind, p, y.to(dtype), bins, beta, sd_eps)
    ll.sum().backward()
    return ll.detach(), p.grad


def groups(F):
    return [slice(0, 10), slice(10, 20), slice(20, 30)] if F == 30 else [slice(0, 1), slice(1, 2)]


def scale_f(kind, par, ll):
    s = 1 + ll.abs()
    if kind != "gauss":
        s = s + par[:, :10].double().abs().max(1).values
    return s


def floor_grad(kind, par, ll, g):
    """floor_g per entry of a frame's gradient g [n, F] (module docstring)."""
    S_f = scale_f(kind, par, ll).unsqueeze(1)
    gm = torch.zeros_like(g)
    for sl in groups(g.shape[1]):
        gm[:, sl] = g[:, sl].abs().max(1, keepdim=True).values
    if kind != "gauss":  # a logit's entry is responsibility - softmax weight: the size of its terms, not of their difference
        pm = torch.softmax(par[:, :10].double(), 1)
        gm[:, :10] = (pm + g[:, :10]).abs() + pm
    return 64 * U * S_f * (g.abs() + gm) + ABS


# ----------------------------------------------------------------------------------------------------------------------
# the crafted frames through each dispatch path
# ----------------------------------------------------------------------------------------------------------------------


def fixture_frames(hs, kind, bins):
    key = f"dmol{bins}" if kind == "dmol" else kind
    par = T(hs[f"{key}_par"])
    y = T(hs[f"{key}_y"] if kind == "dmol" else hs["gmm_y"])
    return par, y, T(hs[f"{key}_ll"]).double(), T(hs[f"{key}_grad"]).double()


def head_case(hs, kind, bins, B, Tp, S, layout, linear, unaligned=False, seed=0):
    """Crafted frames (cycled, shifted by `seed`) in the valid frames of a ragged batch, finite garbage in the padded ones;
    linear: "eye" (identity W, zero bias: the crafted parameters reach the likelihood exactly), "none" (W = NULL)."""
    par, y, ref_ll, ref_g = fixture_frames(hs, kind, bins)
    beta = float(hs["gmm_beta"]) if kind != "dmol" else 1.0
    sd_eps = float(hs["gmm_sd_eps"]) if kind != "dmol" else 0.0
    F = par.shape[1]
    T_, x_sl, valid = frames_layout(B, Tp, S)
    gen = torch.Generator().manual_seed(1000 + seed)
    n_valid = int(valid.sum())
    idx = (torch.arange(n_valid) * 37 + seed) % par.shape[0]
    fr = torch.randn(B, Tp * S, F, generator=gen) * 8  # garbage: finite, never read as a valid frame
    fr[valid] = par[idx]
    yy = torch.full((B, T_), 5.0)  # garbage targets outside [-1, 1] beyond each length
    yv = torch.zeros(B, Tp * S)
    yv[valid] = y[idx]
    yy[valid[:, :T_]] = yv[:, :T_][valid[:, :T_]]
    g_b = torch.randn(B, generator=gen)
    W = torch.eye(F) if linear == "eye" else None
    bias = torch.zeros(F) if linear == "eye" else None
    ll, lp, d_dec, d_par = run_head_abi(kind, to_rows(fr, B, Tp, S, layout), W, bias, yy, x_sl, g_b, layout, B, T_, Tp, S, bins, beta, sd_eps, unaligned)

    tr_ll, tr_g = head_truth(kind, par, y, bins, beta, sd_eps)
    bi, ti = valid.nonzero(as_tuple=True)
    frame_of = lambda i: f"frame (b={int(bi[i])}, tau={int(ti[i])}) = fixture frame {int(idx[i])}"  # noqa: E731
    margins = {}
    # forward: per-frame ll; ll_twise untouched beyond each length; per-utterance fp64 sums
    got_ll = ll[valid[:, :T_]]
    S_f = scale_f(kind, par, tr_ll)
    margins["ll"] = check_bar(f"{kind}/{bins} ll", got_ll, tr_ll[idx], ref_ll[idx], 64 * U * S_f[idx], frame_of)
    pad = ~valid[:, :T_]
    assert bool((ll[pad] == SENTINEL).all()), f"{kind}/{bins} ll_twise written in a padded frame: {ll[pad][ll[pad] != SENTINEL][:5]}"
    own = (ll.double() * valid[:, :T_]).sum(1)
    assert torch.allclose(lp, own, rtol=1e-12, atol=1e-9), f"{kind}/{bins} lp: per-utterance sums {lp} != sums of ll_twise {own}"
    tr_lp = torch.zeros(B, dtype=torch.float64).index_add_(0, bi, tr_ll[idx])
    ref_lp = torch.zeros(B, dtype=torch.float64).index_add_(0, bi, ref_ll[idx])
    fl_lp = torch.zeros(B, dtype=torch.float64).index_add_(0, bi, 64 * U * S_f[idx])
    margins["lp"] = check_bar(f"{kind}/{bins} lp", lp, tr_lp, ref_lp, fl_lp, lambda i: f"utterance {i}")
    # backward: per-entry d_dec (= d_par under identity W), exact zeros in every padded frame
    dd = from_rows(d_dec, B, Tp, S, layout, F)
    gbv = g_b.double()[bi].unsqueeze(1)
    tr_d = tr_g[idx] * gbv
    fl = floor_grad(kind, par, tr_ll, tr_g)[idx] * gbv.abs()
    margins["d_dec"] = check_bar(f"{kind}/{bins} d_dec", dd[valid], tr_d, ref_g[idx] * gbv, fl, lambda i: frame_of(i // F) + f" entry {i % F}")
    assert bool((dd[~valid] == 0).all()), f"{kind}/{bins} d_dec: nonzero in a padded frame ({int((dd[~valid] != 0).sum())} entries)"
    if d_par is not None:
        assert torch.equal(d_par.cpu(), d_dec.cpu()), f"{kind}/{bins} d_par != d_dec under identity W"
    return margins


@pytest.mark.parametrize("bins", [2**16, 256])
@pytest.mark.parametrize("B,Tp,S,layout,linear,unaligned", [
    (3, 2, 64, 0, "eye", False),    # rows kernel, batch-major
    (3, 2, 64, 1, "eye", False),    # rows kernel, time-major
    (2, 3, 64, 1, "none", False),   # rows kernel, W = NULL
    (3, 100, 1, 0, "eye", False),   # generic kernel, S = 1
    (3, 20, 5, 0, "eye", False),    # generic kernel, S = 5 (the open DESIGN row's shape)
    (3, 20, 5, 1, "none", False),   # generic kernel, W = NULL
    (2, 3, 64, 0, "eye", True),     # S = 64 through an unaligned base pointer: generic kernel
    (300, 2, 1, 1, "eye", False),   # B > 256: per-utterance sums by global fp64 atomics
    # rows kernel with several 64-frame units per stack row (upr = S / 64 > 1)
    (3, 5, 128, 1, "eye", False),   # upr 2: 10 units in chunks [0,3) [3,6) [6,10), boundaries inside a row; the last row's 2nd unit is past T
    (3, 5, 128, 0, "eye", False),   # the same, batch-major
    (3, 5, 192, 1, "none", False),  # upr 3 (odd), W = NULL: 15 units in 4 chunks
    (2, 3, 256, 1, "eye", False),   # upr 4: chunks coincide with rows (the contrast case)
    (400, 3, 256, 1, "eye", False),  # the chunk count capped by the chip's fill: 2 chunks of 6 units, the boundary inside row 1
    (2, 3, 128, 0, "eye", True),    # S = 128 through an unaligned base pointer: generic kernel
])
def test_dmol_per_frame_vs_float64(hs, bins, B, Tp, S, layout, linear, unaligned):
    if S >= 128:
        # (the unaligned case takes the generic kernel: no chunks; its frames are laid out the same way)
        rows_units_setup(B, Tp, S, expect_chunks=None if unaligned else {(3, 128): 3, (3, 192): 4, (2, 256): 3, (400, 256): 2}[(B, S)])
    margins = head_case(hs, "dmol", bins, B, Tp, S, layout, linear, unaligned, seed=B + S + layout)
    print(f"[heads dmol/{bins} B={B} Tp={Tp} S={S} layout={layout} {linear}{' unaligned' if unaligned else ''}] worst err / bar: "
          + ", ".join(f"{k} {v:.3g}" for k, v in margins.items()))


def rows_units_setup(B, Tp, S, expect_chunks):
    """What a several-units-per-row case is there for, from the host-side index arithmetic alone (dmol.hip: unit u of an utterance
    is frames [64 u, 64 u + 64); chunk c walks units [c units / n, (c + 1) units / n), n = min(ceil(units / 4), ceil(fill / B)),
    fill = resident workgroups per CU x CUs): some unit has no valid frame, some unit is cut by x_sl mid-way, and the chunk split is
    the one the case names."""
    _, x_sl, _ = frames_layout(B, Tp, S)
    units = Tp * (S // 64)
    start = 64 * torch.arange(units).unsqueeze(0)
    ln = x_sl.unsqueeze(1)
    assert bool((start >= ln).any()), "set-up: no unit without a valid frame"
    assert bool(((start < ln) & (ln < start + 64)).any()), "set-up: no unit that x_sl cuts mid-way"
    if expect_chunks is None:
        return
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for per_cu in (2, 3):  # resident workgroups per CU: 3 by the launch bounds, 2 the library's fallback
        n = max(1, min((units + 3) // 4, (per_cu * cus + B - 1) // B))
        assert n == expect_chunks, f"set-up: {n} chunks at {per_cu} workgroups x {cus} CUs (want {expect_chunks})"
    bounds = [c * units // expect_chunks for c in range(1, expect_chunks)]
    if S != 256 or B == 400:
        assert any(bd % (S // 64) for bd in bounds), f"set-up: no chunk boundary inside a stack row ({bounds})"


@pytest.mark.parametrize("kind", ["gmm", "gauss"])
@pytest.mark.parametrize("B,Tp,S,layout,linear", [(3, 2, 64, 0, "eye"), (3, 2, 64, 1, "none"), (3, 20, 5, 1, "eye"), (300, 2, 1, 1, "eye")])
def test_gaussian_heads_per_frame_vs_float64(hs, kind, B, Tp, S, layout, linear):
    if kind == "gauss" and S == 64 and linear == "none":
        S = 8  # (the single-Gaussian kernel has one path; a second shape instead of a duplicate)
    head_case(hs, kind, 2**16, B, Tp, S, layout, linear, seed=3 * B + S)


@pytest.mark.parametrize("kind,S,layout", [("dmol", 64, 1), ("dmol", 5, 0), ("gmm", 64, 0), ("gmm", 1, 1), ("gauss", 8, 0), ("dmol", 256, 1)])
def test_heads_random_linear_vs_float64(hs, kind, S, layout):
    """The head's Linear (random W, bias) on the crafted frames' neighbourhood: d_dec, dW, db per element against float64,
    through the autograd wrappers (rows kernel at S = 64 and, four units per row, at S = 256; generic kernel otherwise)."""
    par, y, _, _ = fixture_frames(hs, kind, 256 if kind == "dmol" else 2**16)
    beta = float(hs["gmm_beta"]) if kind != "dmol" else 1.0
    sd_eps = float(hs["gmm_sd_eps"]) if kind != "dmol" else 0.0
    F = par.shape[1]
    B, Tp = 3, max(1, 192 // S)
    T_, x_sl, valid = frames_layout(B, Tp, S)
    gen = torch.Generator().manual_seed(S + F)
    # W = I + off-diagonal multiples of 2^-6 (|.| <= 1/16), bias and activations on grids of 2^-14 and 2^-8 (|dec| < 64): every
    # product and partial sum of W dec + b is exact in float32, so the kernel's head outputs equal the float64 ones whatever the
    # summation order, and the bars measure the likelihood and the Linear's backward, not the conditioning of a rounded input
    W = torch.eye(F) + torch.randint(-4, 5, (F, F), generator=gen).float() * (1 - torch.eye(F)) / 64
    bias = torch.randint(-256, 257, (F,), generator=gen).float() / 2**14
    # decoder activations whose head outputs are near the crafted frames
    idx = (torch.arange(B * Tp * S) * 11) % par.shape[0]
    dec_f = torch.linalg.solve(W.double(), (par[idx].double() - bias.double()).t()).t()
    dec_f = (dec_f.clamp(-63, 63) * 256).round().div(256).float().view(B, Tp * S, F)
    yy = torch.where(valid[:, :T_], y[idx].view(B, Tp * S)[:, :T_], torch.full((B, T_), 5.0))
    g_b = torch.randn(B, generator=gen).double()

    def oracle(dt):
        d0, W0, b0 = (t.to(dt).clone().requires_grad_(True) for t in (dec_f, W, bias))
        pp = d0[valid] @ W0.t() + b0
        ll = head_ll(kind, pp, y[idx].view(B, Tp * S)[valid].to(dt), 256 if kind == "dmol" else 2**16, beta, sd_eps)
        bi = valid.nonzero(as_tuple=True)[0]
        lp = torch.zeros(B, dtype=torch.float64).index_add(0, bi, ll.double())
        (lp * g_b).sum().backward()
        return ll.detach().double(), lp.detach(), d0.grad.double(), W0.grad.double(), b0.grad.double(), pp.detach().double()

    r32, tr = oracle(torch.float32), oracle(torch.float64)
    dd = to_rows(dec_f, B, Tp, S, layout).to(DEV).requires_grad_(True)
    Wd, bd = W.to(DEV).requires_grad_(True), bias.to(DEV).requires_grad_(True)
    args = (dd, Wd, bd, yy.to(DEV), x_sl.to(DEV, torch.int32), layout, B, T_, Tp, S)
    if kind == "dmol":
        lp = ops.dmol_log_prob(*args, 10, 256, -7.0)
    elif kind == "gmm":
        lp = ops.gmm_log_prob(*args, 10, beta, sd_eps)
    else:
        lp = ops.gauss_log_prob(*args, beta, sd_eps)
    (lp * g_b.to(DEV)).sum().backward()
    S_f = scale_f(kind, tr[5], tr[0])
    check_bar(f"{kind} lp", lp, tr[1], r32[1], torch.zeros(B, dtype=torch.float64).index_add(0, valid.nonzero(as_tuple=True)[0], 64 * U * S_f),
              lambda i: f"utterance {i}")
    # per-frame gradient w.r.t. the head outputs (d_par) in float64, its floor, and what the Linear makes of them
    p64 = tr[5].clone().requires_grad_(True)
    ll64 = head_ll(kind, p64, y[idx].view(B, Tp * S)[valid].double(), 256 if kind == "dmol" else 2**16, beta, sd_eps)
    ll64.sum().backward()
    gbv = g_b[valid.nonzero(as_tuple=True)[0]].unsqueeze(1)
    fl_par = floor_grad(kind, tr[5], tr[0], p64.grad) * gbv.abs()
    dpar_abs = (p64.grad * gbv).abs()
    d_in = fl_par @ W.double().abs() + 64 * U * (dpar_abs @ W.double().abs())
    got = from_rows(dd.grad, B, Tp, S, layout, F)
    check_bar(f"{kind} d_dec", got[valid], tr[2][valid], r32[2][valid], d_in, lambda i: f"valid frame {i // F} entry {i % F}")
    assert bool((got[~valid] == 0).all()), f"{kind} d_dec: nonzero in a padded frame"
    dec_abs = dec_f[valid].double().abs()
    n = dec_abs.shape[0]
    acc = fl_par + 2 * n * U * dpar_abs  # fp32 sums over n frames: gamma_n ~ n u per term
    fl_w = acc.t() @ dec_abs
    check_bar(f"{kind} dW", Wd.grad, tr[3], r32[3], fl_w, lambda i: f"W[{i // F}, {i % F}]")
    check_bar(f"{kind} db", bd.grad, tr[4], r32[4], acc.sum(0), lambda i: f"b[{i}]")


# ----------------------------------------------------------------------------------------------------------------------
# K8 KL: both layouts, float4 and scalar paths, many step chunks, stride > 1, free-nats ties
# ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("layout,B,Tp,Z,stride,unaligned", [
    (1, 5, 9, 48, 8, False),     # float4 path, time-major
    (0, 5, 9, 48, 8, False),     # float4 path, batch-major
    (1, 4, 7, 30, 4, False),     # scalar path: Z % 4 != 0
    (0, 4, 7, 48, 4, True),      # scalar path: unaligned base
    (1, 2, 250, 256, 1, False),  # Z = 256, several step chunks per utterance (blockIdx.y)
])
def test_kl_per_element_vs_float64(hs, layout, B, Tp, Z, stride, unaligned):
    R = T(hs["kl_mq"]).shape[0]
    rows = B * Tp
    ri = torch.arange(rows) % R
    src = {k: T(hs[f"kl_{k}"])[ri, :Z] for k in ("mq", "sq", "mp", "sp")}  # kernel rows in the kernel's own order
    ref = {f"{t}_{k}": T(hs[f"kl_grad_{t}_{k}"])[ri, :Z].double() for t in ("kl", "fn") for k in ("mq", "sq", "mp", "sp")}
    ref_kl, ref_fn = T(hs["kl_out"])[ri, :Z].double(), T(hs["kl_fn"])[ri, :Z].double()
    free_nats = 0.125 * Z  # floor 1/8 exactly: every 16th element of the fixture ties it
    # lengths: multiples of the stride (a step t with t * stride == x_sl is masked), one of them a single step
    x_sl = torch.tensor([stride * max(1, Tp - 1 - 2 * k) for k in range(B)])
    x_sl[-1] = 1
    r_idx = torch.arange(rows)
    b_of, t_of = (r_idx // Tp, r_idx % Tp) if layout == 0 else (r_idx % B, r_idx // B)
    live = (t_of * stride < x_sl[b_of]).double().unsqueeze(1)
    c = torch.randn(2, B, generator=torch.Generator().manual_seed(Z + B)).double()
    # float64 truth
    ins = [src[k].double().clone().requires_grad_(True) for k in ("mq", "sq", "mp", "sp")]
    kl = O.kl_gaussian(*ins)
    fn = O.discount_free_nats(kl, free_nats)
    tr_kld = torch.zeros(B, dtype=torch.float64).index_add(0, b_of, (kl * live).sum(1))
    tr_fn = torch.zeros(B, dtype=torch.float64).index_add(0, b_of, (fn * live).sum(1))
    (tr_kld * c[0] + tr_fn * c[1]).sum().backward()
    # device
    dins = [dev_buf(src[k], unaligned).view(rows, Z).requires_grad_(True) for k in ("mq", "sq", "mp", "sp")]
    kd, kfd = ops.gaussian_kl_sums(*dins, x_sl.to(DEV, torch.int32), layout, B, Tp, Z, stride, free_nats)
    (kd * c[0].to(DEV) + kfd * c[1].to(DEV)).sum().backward()
    per_b = lambda v: torch.zeros(B, dtype=torch.float64).index_add(0, b_of, (v * live).sum(1))  # noqa: E731
    sum_abs = per_b(kl.detach().abs())
    check_bar("kld", kd, tr_kld, per_b(ref_kl), 64 * U * sum_abs, lambda i: f"utterance {i}")
    check_bar("kld_fn", kfd, tr_fn, per_b(ref_fn), 64 * U * per_b(fn.detach().abs()), lambda i: f"utterance {i}")
    # per-element gradients; coefficient magnitude |c_raw| + |c_fn| on live rows
    mq, sq, mp, sp = (t.detach() for t in ins)
    d = mq - mp
    coef = (c[0].abs() + c[1].abs())[b_of].unsqueeze(1) * live
    terms = {"mq": d.abs() / sp**2, "mp": d.abs() / sp**2, "sq": sq / sp**2 + 1 / sq, "sp": 1 / sp + (sq**2 + d**2) / sp**3}
    cr, cf = (c[0][b_of].unsqueeze(1) * live), (c[1][b_of].unsqueeze(1) * live)
    for k, a, t in zip(("mq", "sq", "mp", "sp"), dins, ins):
        ref32 = cr * ref[f"kl_{k}"] + cf * ref[f"fn_{k}"]
        check_bar(f"d_{k}", a.grad, t.grad, ref32, 64 * U * coef * terms[k] + ABS,
                  lambda i: f"row {i // Z} (b={int(b_of[i // Z])}, t={int(t_of[i // Z])}) element {i % Z}")
        dead = a.grad.detach().cpu()[live.squeeze(1) == 0]
        assert bool((dead == 0).all()), f"d_{k}: nonzero gradient on a masked step"


def test_kl_free_nats_tie_takes_half_the_gradient():
    """At KL == free_nats / Z exactly, max(kl, floor) passes half the gradient (torch.maximum, what the reference runs)."""
    Z, B, Tp = 16, 1, 1
    sp = torch.full((1, Z), 2.0)
    sq = sp.clone()
    mp = torch.zeros(1, Z)
    mq = torch.full((1, Z), 1.0)  # KL = 1 / 8 in every precision
    mq[0, 1] = 3.0  # above the floor
    mq[0, 2] = 0.5  # below
    dins = [t.to(DEV).requires_grad_(True) for t in (mq, sq, mp, sp)]
    kd, kfd = ops.gaussian_kl_sums(*dins, torch.tensor([1], device=DEV, dtype=torch.int32), 1, B, Tp, Z, 1, 0.125 * Z)
    kfd.sum().backward()
    g = dins[0].grad.cpu()[0]
    assert float(g[0]) == 0.5 * 1.0 / 4.0 and float(g[1]) == 3.0 / 4.0 and float(g[2]) == 0.0, g[:3]


# ----------------------------------------------------------------------------------------------------------------------
# which path a launch takes, where the kernel name shows it
# ----------------------------------------------------------------------------------------------------------------------


def test_dispatch_paths_by_kernel_name():
    """Aligned S % 64 == 0 takes the rows kernel, an unaligned base the generic one; KL Z % 4 == 0 the float4 path, Z = 30 the
    scalar one (kernel names from the profiler's device trace)."""
    from torch.profiler import ProfilerActivity, profile

    def names(fn):
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return " | ".join(e.name for e in prof.events())

    B, Tp, S = 2, 1, 64
    y = torch.zeros(B, S, device=DEV)
    xs = torch.full((B,), S, device=DEV, dtype=torch.int32)
    lp = torch.zeros(B, device=DEV, dtype=torch.float64)

    def dmol(unaligned):
        dec = dev_buf(torch.zeros(B * Tp * S * 30), unaligned)
        return lambda: _hip.check(LIB.blvm_dmol_fwd(p_(dec), 0, None, None, p_(y), p_(xs), B, S, Tp, S, 10, 256, -7.0, p_(lp), None,
                                                    _hip.stream_ptr()), "dmol_fwd")

    n = names(dmol(False))
    assert "dmol_rows_kernel" in n, n
    n = names(dmol(True))
    assert "dmol_kernel" in n and "dmol_rows_kernel" not in n, n

    def kl(Z):
        t = torch.ones(2, Z, device=DEV)
        return lambda: ops.gaussian_kl_sums(t, t, t, t, torch.full((1,), 2, device=DEV, dtype=torch.int32), 1, 1, 2, Z, 1, 0.0)

    n = names(kl(48))
    assert "kl_fwd_kernel<true>" in n, n
    n = names(kl(30))
    assert "kl_fwd_kernel<false>" in n, n
