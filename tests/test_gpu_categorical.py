"""GPU: the categorical head (K7d, csrc/cathead.hip) from the kernels up to `WaveNet.forward` / `.generate`.

Op level, per element against the float64 truth of tests/cat_cases.py (`log_softmax` + gather + mask and its autograd):

    |hip - truth| <= max(4 |ref32 - truth|, floor)

with ref32 the same composition in float32 on the CPU — the reference's arithmetic (`nn.Linear`, `logits - logits.logsumexp`,
`.gather`), which tests/test_categorical_cpu.py ties to the reference's own values in tests/golden/categorical.npz — and `floor` an
any-order fp32 bound that is written down, not tuned.  With u = 2^-24 and A_r = max_k (sum_c |x_rc w_kc| + |b_k|):

    floor_ll   = 2 (C + 2) u A_r + 64 u (1 + |l_y| + |lse|)
    eps_rk     = 2 (C + 2) u A_r + 64 u (1 + |l_k| + |lse|)                 relative error of p_k = exp(l_k - lse)
    floor_ddec = sum_k |w_kc| |g| p_k eps_rk + (V + 2) u sum_k |d_rk w_kc|
    floor_dW   = sum_r |x_rc| |g| p_k eps_rk + 2 n u sum_r |d_rk x_rc|      n = counted frames;  floor_db: the same with x = 1
    floor_log_prob[b] = sum_t floor_ll[b, t]                                (the sum itself is carried in float64)

2 (C + 2) u A_r bounds a C-term fp32 dot product plus the bias add in any order; 64 u (1 + |l| + |lse|) covers the roundings of
exp / log / the running-maximum rescalings, whose arguments are of size |l| + |lse|; the second terms bound the V-term (2n-term)
fp32 sums of the gradient products in any order.

| B, skip, S | C   | V    | exercises                                   |
| 3, 43, 1   | 16  | 10   | row tail, V below one class tile            |
| 2, 33, 2   | 32  | 256  | frame stacks, T not a multiple of S         |
| 1, 130, 1  | 96  | 1000 | class-tile tail, the benchmark's C          |
| 5, 13, 1   | 64  | 4096 | many class tiles                            |
| 2, 9, 1    | 512 | 256  | the deepest k                               |
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import cat_cases as CC
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"


def T_(a):
    return torch.from_numpy(np.asarray(a))


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


@functools.lru_cache(maxsize=None)
def reference(shape, regime):
    """(case, float64 truth, float32 composition, floors): computed once, shared, never modified."""
    case = CC.make_case(shape, regime)
    t64, t32 = CC.compose(case, torch.float64), CC.compose(case, torch.float32)
    return case, t64, t32, CC.floors(case, t64)


def run_hip(case):
    from blvm import ops

    B, T, Tp, S = case["B"], case["T"], case["Tp"], case["S"]
    dec = CC.to_rows(case["X_in"], B, Tp, S).to(DEV).requires_grad_(True)
    W, b = case["W"].to(DEV).requires_grad_(True), case["b"].to(DEV).requires_grad_(True)
    y, x_sl = case["y_in"].to(DEV), ops.upload_i32(case["x_sl"], DEV)
    log_prob = ops.categorical_log_prob(dec, W, b, y, x_sl, B, T, Tp, S)
    assert log_prob.dtype == torch.float64 and tuple(log_prob.shape) == (B,)
    (log_prob * case["g"].to(DEV).double()).sum().backward()
    ll = ops.categorical_ll_twise(dec, W, b, y, x_sl, B, T, Tp, S)
    torch.cuda.synchronize()
    return dict(log_prob=log_prob.detach().cpu(), ll=ll.cpu(), d_x=CC.from_rows(dec.grad.cpu(), B, Tp, S), dW=W.grad.cpu(), db=b.grad.cpu())


@pytest.mark.parametrize("regime", CC.REGIMES)
@pytest.mark.parametrize("shape", CC.SHAPES, ids=lambda s: "B{}_T{}_S{}_C{}_V{}".format(*s))
def test_fused_head_meets_the_bar_per_element(shape, regime):
    case, t64, t32, fl = reference(tuple(shape), regime)
    got = run_hip(case)
    B, T, C, V, Tall = case["B"], case["T"], case["C"], case["V"], case["Tp"] * case["S"]
    assert torch.isfinite(got["ll"]).all() and torch.isfinite(got["d_x"]).all() and torch.isfinite(got["dW"]).all()
    assert (got["ll"][~case["valid"][:, :T]] == 0).all() and (got["d_x"][~case["valid"]] == 0).all(), "a frame that does not count leaked"
    CC.check_bar("ll", got["ll"], t64["ll"], t32["ll"], fl["ll"], lambda i: f"(b {i // T}, tau {i % T})")
    CC.check_bar("log_prob", got["log_prob"], t64["log_prob"], t32["log_prob"], fl["ll"].sum(1), lambda i: f"utterance {i}")
    CC.check_bar("d_dec", got["d_x"], t64["d_x"], t32["d_x"], fl["d_x"], lambda i: f"(b {i // (Tall * C)}, tau {i // C % Tall}, c {i % C})")
    CC.check_bar("dW", got["dW"], t64["dW"], t32["dW"], fl["dW"], lambda i: f"(class {i // C}, c {i % C})")
    CC.check_bar("db", got["db"], t64["db"], t32["db"], fl["db"], lambda i: f"class {i}")


def _raw_fwd_bwd(case, poison):
    """The C ABI itself on output buffers (and a workspace) filled with `poison`."""
    from blvm import ops
    from blvm._hip import check, load, ptr, stream_ptr

    B, T, Tp, S, C, V = (case[k] for k in ("B", "T", "Tp", "S", "C", "V"))
    lib = load()
    dec = CC.to_rows(case["X_in"], B, Tp, S).to(DEV)
    W, b, g = case["W"].to(DEV), case["b"].to(DEV), case["g"].to(DEV)
    y, x_sl = case["y_in"].to(DEV).to(torch.int32), ops.upload_i32(case["x_sl"], DEV)
    full = lambda *s: torch.full(s, poison, device=DEV, dtype=torch.float32)  # noqa: E731
    lse, ll, log_prob = full(B * Tp * S), full(B, T), torch.zeros(B, device=DEV, dtype=torch.float64)
    check(lib.blvm_cat_fwd(ptr(dec), ptr(W), ptr(b), ptr(y), ptr(x_sl), B, T, Tp, S, C, V, ptr(lse), ptr(ll), ptr(log_prob), stream_ptr()), "fwd")
    d_dec, dW, db = full(Tp * B, S * C), full(V, C), full(V)
    n_ws = lib.blvm_cat_bwd_workspace_floats(B * Tp * S, C, V)
    ws = full(max(n_ws, 1))
    check(lib.blvm_cat_bwd(ptr(dec), ptr(W), ptr(b), ptr(y), ptr(x_sl), ptr(lse), ptr(g), B, T, Tp, S, C, V, ptr(d_dec), ptr(dW), ptr(db),
                           ptr(ws), stream_ptr()), "bwd")  # fmt: skip
    torch.cuda.synchronize()
    return [t.cpu() for t in (lse, ll, log_prob, d_dec, dW, db)]


@pytest.mark.parametrize("shape,regime", [(CC.SHAPES[0], "garbage_padding"), (CC.SHAPES[1], "random"), (CC.SHAPES[3], "peaked")])
def test_forward_and_backward_twice_on_poisoned_buffers_are_bit_identical(shape, regime):
    """Caller-owned buffers: nothing depends on what lse, ll, d_dec, dW, db or the workspace held (NaN, then 1e30), and without float
    atomics two calls agree to the bit."""
    case = reference(tuple(shape), regime)[0]
    first, second = _raw_fwd_bwd(case, float("nan")), _raw_fwd_bwd(case, 1e30)
    for name, a, b in zip(("lse", "ll", "log_prob", "d_dec", "dW", "db"), first, second):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), f"{name}: {int((a != b).sum())} elements differ between the two calls"


def test_unsupported_widths_are_refused_by_the_library():
    from blvm._hip import CONSTANTS, load, ptr, stream_ptr

    lib = load()
    t = torch.zeros(64, device=DEV)
    i = torch.zeros(4, device=DEV, dtype=torch.int32)
    for C, V in ((24, 10), (16, 1), (528, 10), (16, 65537)):
        rc = lib.blvm_cat_fwd(ptr(t), ptr(t), ptr(t), ptr(i), ptr(i), 1, 1, 1, 1, C, V, ptr(t), ptr(t), None, stream_ptr())
        assert rc == CONSTANTS["BLVM_ENOSUP"], (C, V, rc)


# ---- the memory condition: the point of the kernel ----------------------------------------------------------------------------------


def test_sixteen_bit_head_runs_without_materialising_the_logits():
    """B = 2, skip = 1024, C = 64, V = 65536: the logits would be 512 MiB (and as much again for their gradient).  Forward + backward
    through `ops.categorical_log_prob` may raise the peak of allocated device memory by less than 128 MiB over the operands and the
    returned gradients.  ll of 64 sampled frames and dW / db of 16 sampled classes meet the bar of this file; the float64 truth is
    computed on the CPU in chunks of frames."""
    from blvm import ops
    from blvm._hip import load

    B, Tp, S, C, V = 2, 1024, 1, 64, 65536
    T = Tp
    rng = np.random.RandomState(99)
    X = torch.from_numpy(rng.standard_normal((B, T, C)).astype(np.float32))
    W = torch.from_numpy((2.0 * rng.standard_normal((V, C)) / np.sqrt(C)).astype(np.float32))
    bias = torch.from_numpy((0.1 * rng.standard_normal(V)).astype(np.float32))
    y = torch.from_numpy(rng.randint(0, V, size=(B, T)).astype(np.int64))
    y[0, :8] = V - 1
    x_sl = torch.tensor([T, T - 101])
    g = torch.tensor([1.0, -0.5])
    valid = torch.arange(T).unsqueeze(0) < x_sl.unsqueeze(1)
    X = X * valid.unsqueeze(-1)
    y = y * valid

    lib = load()
    assert lib.blvm_cat_bwd_workspace_floats(2048, C, V) == lib.blvm_cat_bwd_workspace_floats(2048000, C, V)

    dec = CC.to_rows(X, B, Tp, S).to(DEV).requires_grad_(True)
    Wd, bd = W.to(DEV).requires_grad_(True), bias.to(DEV).requires_grad_(True)
    yd, sl, gd = y.to(DEV), ops.upload_i32(x_sl, DEV), g.to(DEV).double()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    log_prob = ops.categorical_log_prob(dec, Wd, bd, yd, sl, B, T, Tp, S)
    (log_prob * gd).sum().backward()
    torch.cuda.synchronize()
    grads = sum(t.grad.numel() * 4 for t in (dec, Wd, bd))
    rise = torch.cuda.max_memory_allocated() - base - grads
    print(f"peak rise over operands and gradients: {rise / 2**20:.1f} MiB (logits would be {B * T * V * 4 / 2**20:.0f} MiB)")
    assert rise < 128 * 2**20, f"{rise / 2**20:.1f} MiB"
    ll = ops.categorical_ll_twise(dec, Wd, bd, yd, sl, B, T, Tp, S).cpu()
    dW, db = Wd.grad.cpu(), bd.grad.cpu()

    # truth, chunk by chunk: lse, l_y, A_r per frame and the logits of the 16 sampled classes
    cls = torch.linspace(0, V - 1, 16).round().long()
    Xf, yf, gm = X.reshape(-1, C), y.reshape(-1), (g.unsqueeze(1) * valid).reshape(-1).double()
    n_fr = Xf.shape[0]
    W64, b64, Wabs = W.double(), bias.double(), W.double().abs()
    lse64, ly64, A, lk64 = torch.empty(n_fr, dtype=torch.float64), torch.empty(n_fr, dtype=torch.float64), torch.empty(n_fr, dtype=torch.float64), torch.empty(n_fr, 16, dtype=torch.float64)
    lse32, ly32, lk32 = torch.empty(n_fr), torch.empty(n_fr), torch.empty(n_fr, 16)
    for i in range(0, n_fr, 256):
        s = slice(i, i + 256)
        l = Xf[s].double() @ W64.t() + b64
        lse64[s], ly64[s], lk64[s] = l.logsumexp(-1), l.gather(-1, yf[s].unsqueeze(-1)).squeeze(-1), l[:, cls]
        A[s] = (Xf[s].double().abs() @ Wabs.t() + b64.abs()).max(-1).values
        l = torch.nn.functional.linear(Xf[s], W, bias)
        lse32[s], ly32[s], lk32[s] = l.logsumexp(-1), l.gather(-1, yf[s].unsqueeze(-1)).squeeze(-1), l[:, cls]
    fr = torch.linspace(0, n_fr - 1, 64).round().long()
    vf = valid.reshape(-1).double()
    prod = 2 * (C + 2) * CC.U * A
    CC.check_bar("ll (64 frames)", ll.reshape(-1)[fr], ((ly64 - lse64) * vf)[fr], ((ly32 - lse32).double() * vf)[fr],
                 (prod + 64 * CC.U * (1 + ly64.abs() + lse64.abs()))[fr], lambda i: f"frame {int(fr[i])}")  # fmt: skip
    onehot = (yf.unsqueeze(1) == cls.unsqueeze(0)).double()
    p64 = (lk64 - lse64.unsqueeze(1)).exp()
    d64 = gm.unsqueeze(1) * (onehot - p64)  # [frames, 16]
    d32 = (gm.float().unsqueeze(1) * (onehot.float() - (lk32 - lse32.unsqueeze(1)).exp()))
    eps = prod.unsqueeze(1) + 64 * CC.U * (1 + lk64.abs() + lse64.abs().unsqueeze(1))
    pe = gm.abs().unsqueeze(1) * p64 * eps
    n = float(valid.sum())
    X64 = Xf.double()
    CC.check_bar("dW (16 classes)", dW[cls], d64.t() @ X64, (d32.t() @ Xf).double(), pe.t() @ X64.abs() + 2 * n * CC.U * (d64.abs().t() @ X64.abs()),
                 lambda i: f"(class {int(cls[i // C])}, c {i % C})")  # fmt: skip
    CC.check_bar("db (16 classes)", db[cls], d64.sum(0), d32.sum(0).double(), pe.sum(0) + 2 * n * CC.U * d64.abs().sum(0),
                 lambda i: f"class {int(cls[i])}")  # fmt: skip


# ---- sampler ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("regime", CC.SAMPLER_REGIMES)
@pytest.mark.parametrize("V", CC.SAMPLER_V)
def test_sampler_draw_by_draw(V, regime):
    """Every one of the 64 draws lies between the float64 prefix sums around u S (`cat_cases.check_draws`); without uniforms the
    arg-max, which on materialised logits is exact: the float64 arg-max wherever the maximum is unique, the lowest index on a tie."""
    from blvm import ops

    logits, u = CC.sampler_case(V, regime)
    k = ops.categorical_sample(logits.to(DEV), u.to(DEV))
    assert k.dtype == torch.int64 and tuple(k.shape) == (CC.SAMPLER_ROWS,)
    print(f"worst draw margin {CC.check_draws(logits, u, k):.3g}")
    mode = ops.categorical_sample(logits.to(DEV)).cpu()
    top = logits.double().max(-1, keepdim=True).values
    first = (logits.double() == top).int().argmax(-1)  # the lowest index that holds the maximum
    assert torch.equal(mode, first)
    if regime == "equal":
        assert (mode == 0).all()


# ---- the model ---------------------------------------------------------------------------------------------------------------------


def tiny_wavenet(nsf):
    from blvm.models import WaveNet
    from blvm.modules.distributions import CategoricalDense

    g = np.load(os.path.join(GOLDEN, "categorical.npz"))
    m = WaveNet(likelihood=CategoricalDense(16, 32), n_layers=2, n_stacks=2, res_channels=16, kernel_size=2, base_dilation=2, n_stack_frames=nsf)
    tag = f"wn{nsf}.sd."
    m.load_state_dict({k[len(tag) :]: T_(g[k]) for k in g.files if k.startswith(tag)})
    assert m.receptive_field == int(g[f"wn{nsf}.rf"])
    return m.to(DEV), g


@pytest.mark.parametrize("nsf", [1, 2])
@pytest.mark.parametrize("give_y", [False, True])
def test_tiny_wavenet_vs_reference_golden(nsf, give_y):
    """Loss, per-utterance log-prob, frame-wise ll and every parameter gradient against the reference's modules (the fixture), at the
    tolerances tests/test_gpu_parity.py uses for the WaveNet DMoL goldens; the targets quantised on the device equal the reference's."""
    m, g = tiny_wavenet(nsf)
    x, x_sl, y = T_(g[f"wn{nsf}.x"]).to(DEV), T_(g[f"wn{nsf}.x_sl"]), T_(g[f"wn{nsf}.y"])
    loss, metrics, out = m(x, x_sl, y=y.to(DEV) if give_y else None)
    loss.backward()
    assert torch.equal(out.y.squeeze(-1).cpu(), y)
    assert float(loss) == pytest.approx(float(g[f"wn{nsf}.loss"]), rel=1e-5)
    torch.testing.assert_close(out.log_prob.cpu(), T_(g[f"wn{nsf}.log_prob"]), rtol=1e-5, atol=1e-3)
    torch.testing.assert_close(out.log_prob_twise.cpu(), T_(g[f"wn{nsf}.ll"]), rtol=1e-4, atol=1e-4)
    assert len(metrics) == 3
    for k, p in m.named_parameters():
        assert rel_l2(p.grad, T_(g[f"wn{nsf}.grad.{k}"])) < 1e-3, k
    assert tuple(out.parameters.shape) == (3, 37, 32)
    assert out.predictions.shape == out.predictions_mode.shape == (3, 37)
    assert torch.equal(out.predictions_mode.cpu(), out.parameters.cpu().double().argmax(-1))


def test_forward_split_over_two_splits_sums_to_the_whole():
    m, g = tiny_wavenet(1)
    torch.manual_seed(5)
    rf = m.receptive_field
    B, L = 2, 3 * rf
    T = 2 * L - rf  # the second split starts at L - rf and predicts frames L .. T - 1
    x = (torch.rand(B, T) * 2 - 1).to(DEV)
    x_sl = torch.tensor([T, T - 3])
    x = x * (torch.arange(T, device=DEV).unsqueeze(0) < x_sl.to(DEV).unsqueeze(1))
    whole = m(x, x_sl)[2].log_prob.double().cpu()
    xs, sls = m.split_sequence(x, x_sl, length=L)
    assert len(xs) == 2 and all(xi.size(0) == B for xi in xs)
    parts = sum(m.forward_split(xi.contiguous(), sli, i_split=i)[2].log_prob.double().cpu() for i, (xi, sli) in enumerate(zip(xs, sls)))
    torch.testing.assert_close(parts, whole, rtol=1e-5, atol=1e-3)


def test_generate_window_cached_prompt_and_state_agree():
    """The window path and the block-by-block cached path draw the same classes from the same uniforms; a prompt plus `state=` in two
    chunks equals one call; every returned value is a `dequantize` value."""
    m, g = tiny_wavenet(1)
    lik = m.likelihood
    assert not m._decode_kernel_applies()
    B, n = 3, 14
    gen = torch.Generator().manual_seed(11)
    uni = [torch.rand(B, generator=gen).to(DEV) for _ in range(n)]
    xw = m.generate(B, n_frames=n, uniforms=uni)
    xc = m.generate(B, n_frames=n, uniforms=uni, cached=True)
    assert tuple(xw.shape) == tuple(xc.shape) == (B, n, 1) and xw.dtype == torch.float32
    levels = torch.linspace(-1, 1, 32)
    for xx in (xw, xc):
        assert (xx.cpu().reshape(-1, 1) == levels.unsqueeze(0)).any(-1).all(), "a returned value is no dequantize value"
    kw, kc = (torch.bucketize(xx.cpu().squeeze(-1), levels) for xx in (xw, xc))
    assert torch.equal(kw, kc)
    assert torch.equal(lik.dequantize(kw.to(DEV)).cpu(), xw.cpu().squeeze(-1))
    assert len(kw.unique()) > 4, "degenerate draws"

    prompt = xw[:, :5]
    one = m.generate(B, n_frames=8, x=prompt, uniforms=uni[:8], cached=True)
    a, st = m.generate(B, n_frames=3, x=prompt, uniforms=uni[:3], cached=True, return_state=True)
    b_ = m.generate(B, n_frames=5, uniforms=uni[3:8], cached=True, state=st)
    assert torch.equal(torch.cat([a, b_], 1), one)
    assert (one.cpu().reshape(-1, 1) == levels.unsqueeze(0)).any(-1).all()
