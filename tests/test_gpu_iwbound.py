"""GPU (MI355X): K8m, the two reductions of the importance-weighted bound (csrc/iwbound.hip).

`blvm_gauss_logratio_fwd` per utterance against the formula in float64 on the same fp32 inputs, on K8's case table (both layouts,
float4 and scalar paths, an unaligned base, many steps, stride > 1, a length of a single step) plus a row of length 0.  Operands from
the trained-regime fixture tests/golden/heads_stress.npz (kl_mq, kl_sq, kl_mp, kl_sp), tiled as tests/test_gpu_heads.py tiles them
for K8; eps seeded normals with planted +-5 and exact zeros; z = fl32(mu_q + sd_q eps).
Bar per utterance: K8's rule for its sums, 64 u sum |r| over the live elements (u = 2^-24; tests/test_gpu_heads.py): each element is
a handful of fp32 roundings of terms that sum |r| bounds up to cancellation, added in float64.

`blvm_iw_reduce` against torch.logsumexp in float64 on the CPU: |err| <= 4 K 2^-53 max(1, |bound|), a bound on K double roundings
(K exponentials of at most 1 summed in order, one log, two additions at the size of the bound); the identities K = 1 and K equal
weights bitwise; ess to 1e-12 relative."""
import math
import os

import numpy as np
import pytest
import torch

from blvm import _hip, ops

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0**-24
LIB = None


@pytest.fixture(scope="module", autouse=True)
def _require_hip():
    global LIB
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    LIB = _hip.load()
    assert LIB.blvm_device_ok() == 1, "libblvm_hip: no gfx950 device visible"


@pytest.fixture(scope="module")
def hs():
    return {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(os.path.join(GOLDEN, "heads_stress.npz")).items() if k.startswith("kl_")}


def check_bar(name, got, truth, ref32, floor, frame_of=None):
    """Per-element bar; the message names the quantity, the worst frame and its margin.  (tests/test_gpu_heads.py's helper.)"""
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


def operands(hs, layout, B, Tp, Z, stride, zero_row=False):
    """(six fp32 host operands [rows, Z] in the kernel's row order, x_sl [B], live [rows, 1], b_of [rows])."""
    R = hs["kl_mq"].shape[0]
    rows = B * Tp
    ri = torch.arange(rows) % R
    mq, sq, mp, sp = (hs[f"kl_{k}"][ri, :Z].float().contiguous() for k in ("mq", "sq", "mp", "sp"))
    g = torch.Generator().manual_seed(1000 * Z + 10 * B + layout)
    eps = torch.randn(rows, Z, generator=g)
    flat = eps.view(-1)
    flat[0::97] = 5.0
    flat[1::101] = -5.0
    flat[2::89] = 0.0
    z = mq + sq * eps  # fp32: the value a chain stores (its fma may differ in the last bit; the kernel takes z as given)
    # lengths: multiples of the stride (a step t with t * stride == x_sl is masked), one of them a single step
    x_sl = torch.tensor([stride * max(1, Tp - 1 - 2 * k) for k in range(B)])
    x_sl[-1] = 1
    if zero_row:
        x_sl[1] = 0
    r_idx = torch.arange(rows)
    b_of, t_of = (r_idx // Tp, r_idx % Tp) if layout == 0 else (r_idx % B, r_idx // B)
    live = (t_of * stride < x_sl[b_of]).double().unsqueeze(1)
    return (mq, sq, mp, sp, z, eps), x_sl, live, b_of


def truth64(ops6, live, b_of, B):
    """(float64 per-utterance sums of r, of |r|) from the formula on the same fp32 inputs."""
    mq, sq, mp, sp, z, e = (t.double() for t in ops6)
    r = sp.log() - sq.log() - 0.5 * e * e + 0.5 * ((z - mp) / sp) ** 2
    per_b = lambda v: torch.zeros(B, dtype=torch.float64).index_add(0, b_of, (v * live).sum(1))  # noqa: E731
    return per_b(r), per_b(r.abs())


def run(ops6, x_sl, layout, B, Tp, Z, stride, unaligned=False):
    d = [dev_buf(t, unaligned).view(B * Tp, Z) for t in ops6]
    return ops.gauss_log_ratio_sums(*d, x_sl.to(DEV, torch.int32), layout, B, Tp, Z, stride)


CASES = [
    (1, 5, 9, 48, 8, False, False),     # float4 path, time-major
    (0, 5, 9, 48, 8, False, False),     # float4 path, batch-major
    (1, 4, 7, 30, 4, False, False),     # scalar path: Z % 4 != 0
    (0, 4, 7, 48, 4, True, False),      # scalar path: unaligned base
    (1, 2, 250, 256, 1, False, False),  # Z = 256, many steps per wave
    (1, 5, 9, 48, 8, False, True),      # a row of x_sl = 0
]


@pytest.mark.parametrize("layout,B,Tp,Z,stride,unaligned,zero_row", CASES)
def test_logratio_per_row_vs_float64(hs, layout, B, Tp, Z, stride, unaligned, zero_row):
    ops6, x_sl, live, b_of = operands(hs, layout, B, Tp, Z, stride, zero_row)
    tr, sum_abs = truth64(ops6, live, b_of, B)
    got = run(ops6, x_sl, layout, B, Tp, Z, stride, unaligned)
    assert got.dtype == torch.float64 and got.shape == (B,)
    if zero_row:
        assert float(got[1]) == 0.0 and float(sum_abs[1]) == 0.0
    worst = ((got.cpu() - tr).abs() / (64 * U * sum_abs).clamp_min(1e-300)).max()
    print(f"logratio case {(layout, B, Tp, Z, stride, unaligned, zero_row)}: worst err/bar {float(worst):.3g}")
    # (a row without live steps: truth and sum |r| are 0 and so must the result be; 0 / 0 is no margin, so its bar is the tiniest double)
    check_bar("logratio", got, tr, tr, (64 * U * sum_abs).clamp_min(5e-324), lambda i: f"utterance {i}")


def test_logratio_written_not_accumulated_and_repeatable(hs):
    layout, B, Tp, Z, stride = 1, 5, 9, 48, 8
    ops6, x_sl, _, _ = operands(hs, layout, B, Tp, Z, stride, zero_row=True)
    d = [t.to(DEV) for t in ops6]
    xs = x_sl.to(DEV, torch.int32)
    outs = []
    for fill in (float("nan"), 1e30, 0.0):
        out = torch.full((B,), fill, device=DEV, dtype=torch.float64)
        _hip.check(LIB.blvm_gauss_logratio_fwd(*(_hip.ptr(t) for t in d), layout, _hip.ptr(xs), B, Tp, Z, stride, _hip.ptr(out),
                                               _hip.stream_ptr()), "blvm_gauss_logratio_fwd")  # fmt: skip
        outs.append(out.cpu())
    again = ops.gauss_log_ratio_sums(*d, xs, layout, B, Tp, Z, stride).cpu()
    for o in outs + [again]:
        assert torch.equal(o.view(torch.int64), outs[0].view(torch.int64)), (o, outs[0])
    assert bool(torch.isfinite(outs[0]).all())


@pytest.mark.parametrize("layout,Z", [(1, 48), (0, 30)])
def test_logratio_masked_steps_are_not_read(hs, layout, Z):
    B, Tp, stride = 4, 7, 4
    ops6, x_sl, live, b_of = operands(hs, layout, B, Tp, Z, stride, zero_row=True)
    clean = run(ops6, x_sl, layout, B, Tp, Z, stride).cpu()
    dead = (live.squeeze(1) == 0)
    assert bool(dead.any())
    poisoned = []
    for i, t in enumerate(ops6):
        t = t.clone()
        t[dead] = (float("nan"), float("inf"), -float("inf"))[i % 3]
        poisoned.append(t)
    got = run(poisoned, x_sl, layout, B, Tp, Z, stride).cpu()
    assert torch.equal(got.view(torch.int64), clean.view(torch.int64)), (got, clean)


def test_logratio_refuses_bad_arguments():
    t = torch.ones(2, 4, device=DEV)
    xs = torch.full((1,), 2, device=DEV, dtype=torch.int32)
    out = torch.zeros(1, device=DEV, dtype=torch.float64)
    p = _hip.ptr

    def rc(layout=1, B=1, Tp=2, Z=4, stride=1, mq=t, o=out):
        return LIB.blvm_gauss_logratio_fwd(p(mq), p(t), p(t), p(t), p(t), p(t), layout, p(xs), B, Tp, Z, stride, p(o), _hip.stream_ptr())

    einval = _hip.CONSTANTS["BLVM_EINVAL"]
    assert rc() == 0
    for kw in (dict(layout=2), dict(layout=-1), dict(B=0), dict(Tp=0), dict(Z=0), dict(stride=0), dict(mq=None), dict(o=None)):
        assert rc(**kw) == einval, kw
    with pytest.raises(_hip.BlvmHipError):
        ops.gauss_log_ratio_sums(*(torch.ones(2, 4),) * 6, xs, 1, 1, 2, 4, 1)


# ----------------------------------------------------------------------------------------------------------------------
# iw_reduce
# ----------------------------------------------------------------------------------------------------------------------


def columns(K, B, spread, seed):
    """log_w [K, B] float64 at the size of an utterance's log-likelihood, the particles `spread` nats apart at most."""
    g = torch.Generator().manual_seed(seed)
    base = -4000.0 - 500.0 * torch.rand(1, B, generator=g, dtype=torch.float64)
    return base + spread * torch.rand(K, B, generator=g, dtype=torch.float64)


def reference(log_w):
    K = log_w.shape[0]
    bound = torch.logsumexp(log_w, 0) - math.log(K)
    w = (log_w - log_w.max(0).values).exp()
    return bound, w.sum(0) ** 2 / (w * w).sum(0)


@pytest.mark.parametrize("K", [1, 2, 7, 64])
@pytest.mark.parametrize("B", [1, 5])
def test_iw_reduce_vs_logsumexp(K, B):
    for spread in (0.0, 50.0, 2000.0):
        lw = columns(K, B, spread, seed=K * 100 + B + int(spread))
        bound, ess = (t.cpu() for t in ops.iw_reduce(lw.to(DEV)))
        rb, re = reference(lw)
        if K == 1:
            assert torch.equal(bound.view(torch.int64), lw[0].view(torch.int64)) and bool((ess == 1.0).all())
        if spread == 0.0:  # K equal weights: the weight itself and ess = K, exactly
            assert torch.equal(bound.view(torch.int64), lw[0].view(torch.int64)), (bound, lw[0])
            assert bool((ess == float(K)).all()), ess
        tol = 4 * K * 2.0**-53 * rb.abs().clamp_min(1.0)
        err = (bound - rb).abs()
        assert bool((err <= tol).all()), f"K={K} B={B} spread={spread}: err {err.tolist()} tol {tol.tolist()}"
        assert bool(((ess - re).abs() <= 1e-12 * re.abs()).all()), (ess, re)
        assert bool((ess >= 1.0 - 1e-12).all()) and bool((ess <= K + 1e-9).all())


@pytest.mark.parametrize("K", [1, 2, 7, 64])
@pytest.mark.parametrize("B", [1, 5])
def test_iw_reduce_special_columns(K, B):
    lw = columns(K, B, 50.0, seed=K + B)
    clean_b, clean_e = (t.cpu() for t in ops.iw_reduce(lw.to(DEV)))
    lw2 = lw.clone()
    lw2[:, 0] = -float("inf")  # no weight at all
    if B > 1:
        lw2[K // 2, 1] = float("nan")
    bound, ess = (t.cpu() for t in ops.iw_reduce(lw2.to(DEV)))
    assert float(bound[0]) == -float("inf") and float(ess[0]) == 0.0
    if B > 1:
        assert math.isnan(float(bound[1])) and math.isnan(float(ess[1]))
        # the other columns are untouched, bit for bit
        assert torch.equal(bound[2:].view(torch.int64), clean_b[2:].view(torch.int64))
        assert torch.equal(ess[2:].view(torch.int64), clean_e[2:].view(torch.int64))
    # one particle at -inf among finite ones carries no weight
    if K > 1:
        lw3 = lw.clone()
        lw3[0] = -float("inf")
        b3, _ = ops.iw_reduce(lw3.to(DEV))
        rb, _ = reference(lw3)
        assert bool(((b3.cpu() - rb).abs() <= 4 * K * 2.0**-53 * rb.abs().clamp_min(1.0)).all())


def test_iw_reduce_ess_may_be_null_and_repeats_and_refuses_cpu():
    K, B = 7, 5
    lw = columns(K, B, 50.0, seed=3).to(DEV)
    b0, e0 = ops.iw_reduce(lw)
    for fill in (float("nan"), 1e30):
        out = torch.full((B,), fill, device=DEV, dtype=torch.float64)
        _hip.check(LIB.blvm_iw_reduce(_hip.ptr(lw), K, B, _hip.ptr(out), None, _hip.stream_ptr()), "blvm_iw_reduce")
        assert torch.equal(out.view(torch.int64), b0.view(torch.int64))
    b1, e1 = ops.iw_reduce(lw)
    assert torch.equal(b1.view(torch.int64), b0.view(torch.int64)) and torch.equal(e1.view(torch.int64), e0.view(torch.int64))
    with pytest.raises(_hip.BlvmHipError):
        ops.iw_reduce(lw.cpu())
    assert LIB.blvm_iw_reduce(_hip.ptr(lw), 0, B, _hip.ptr(b0), None, _hip.stream_ptr()) == _hip.CONSTANTS["BLVM_EINVAL"]
