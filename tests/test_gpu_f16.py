"""The fp16-operand mode (`blvm_set_operand_dtype(BLVM_DTYPE_F16)`, `--use_amp True --amp_dtype f16`: the reference's fp16 autocast
regime, `experiments/experiment_vrnn_audio.py:198,219-230`): fp16 operands / fp32 accumulation exactly where the bf16 mode has bf16
operands (K6 GEMMs, the persistent recurrent chains, the GRU / LSTM sequence kernels, the WaveNet block kernels), with dynamic loss
scaling in training.

(1) The kernels compute what the mode says: products of fp16-ROUNDED operands (torch's .half(): nearest even, |x| >= 65520 -> inf)
accumulated in fp32.  (2) On the reference's golden inputs the mode stays inside SURVEY A.4's budget (1.2e-3 nats/frame) and is closer
to fp32 than the bf16 mode.  Gradients are taken as GradScaler takes them: backward of loss * 2^16, then divided by the scale."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import blvm_oracle as O
from blvm import _hip, ops
from blvm.models import SRNNAudio, VRNNAudio

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NATS_PER_FRAME_BUDGET = 1.2e-3
SCALE = 2.0**16  # GradScaler's initial scale (the reference's default)
FP16_TINY = 6.1e-5  # smallest normal fp16 number (2^-14)


@pytest.fixture(autouse=True)
def _f16_mode():
    assert torch.cuda.is_available() and _hip.load().blvm_device_ok() == 1
    _hip.set_operand_dtype("f16")
    yield
    _hip.set_operand_dtype("f32")
    _hip.check_async()


def T(a):
    return torch.from_numpy(np.asarray(a))


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def rh(t):  # what the kernels multiply: operands rounded to fp16 (nearest even)
    return t.half().double()


def rb(t):
    return t.to(torch.bfloat16).double()


def _in(mode, fn):
    """fn() in operand mode `mode`, then back to fp16."""
    _hip.set_operand_dtype(mode)
    try:
        return fn()
    finally:
        _hip.set_operand_dtype("f16")


def test_mode_switch_round_trip():
    lib = _hip.load()
    assert _hip.get_operand_dtype() == "f16" and lib.blvm_get_operand_dtype() == 2
    for name, code in (("f32", 0), ("bf16", 1), ("f16", 2)):
        _hip.set_operand_dtype(name)
        assert _hip.get_operand_dtype() == name and lib.blvm_get_operand_dtype() == code
    for bad in (3, 7, -1):
        assert lib.blvm_set_operand_dtype(bad) != 0
        assert b"BLVM_DTYPE_F16" in lib.blvm_last_error()
        assert lib.blvm_get_operand_dtype() == 2  # unchanged
    assert lib.blvm_set_operand_dtype(2) == 0 and _hip.get_operand_dtype() == "f16"
    with pytest.raises(ValueError):
        _hip.set_operand_dtype("fp16")


def _gemm_ref(A, Bm, op_a, op_b, r):
    return (r(A).t() if op_a else r(A)) @ (r(Bm) if op_b else r(Bm).t())


@pytest.mark.parametrize("op_a,op_b", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(64, 64, 32), (130, 70, 50), (256, 1920, 768), (1000, 30, 30), (16, 256, 1003), (384, 192, 517)])
def test_gemm_f16_operands_fp32_accumulate(op_a, op_b, M, N, K):
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K + op_a * 2 + op_b)
    A = torch.randn(*((K, M) if op_a else (M, K)), generator=g)
    Bm = torch.randn(*((K, N) if op_b else (N, K)), generator=g)
    bias = torch.randn(N, generator=g)
    leaky = lambda t: torch.where(t > 0, t, 0.01 * t)  # noqa: E731
    ref = leaky(_gemm_ref(A, Bm, op_a, op_b, rh) + bias.double())
    C = torch.empty(M, N, device=DEV)
    ops.gemm(op_a, op_b, M, N, K, A.to(DEV), A.shape[1], Bm.to(DEV), Bm.shape[1], C, N, bias=bias.to(DEV), act=ops.ACT_LEAKY, slope=0.01)
    assert rel_l2(C, ref) < 2e-6
    # and it is the fp16 product: measurably away from the unrounded product, much closer to it than the bf16-rounded product
    full = leaky(_gemm_ref(A, Bm, op_a, op_b, lambda t: t.double()) + bias.double())
    bf = leaky(_gemm_ref(A, Bm, op_a, op_b, rb) + bias.double())
    e16, ebf = rel_l2(C, full), rel_l2(bf, full)
    assert e16 > 1e-5, e16
    assert e16 < ebf / 4, (e16, ebf)


@pytest.mark.parametrize("op_a,op_b", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(64, 64, 32), (130, 70, 50)])
def test_gemm_f16_subnormal_operands_are_halfs(op_a, op_b, M, N, K):
    """Operands below fp16's smallest normal number (6.1e-5), which randn almost never draws: log-uniform in [1e-7, 6e-5] with a
    random sign.  .half() keeps them as subnormals (multiples of 2^-24); so must the conversion and the fp16 matrix pipe."""
    g = torch.Generator().manual_seed(M + N + K + op_a * 2 + op_b)

    def draw(*shape):
        lo, hi = np.log(1e-7), np.log(6e-5)
        mag = torch.exp(torch.rand(*shape, generator=g) * (hi - lo) + lo)
        return mag * (torch.randint(0, 2, shape, generator=g) * 2 - 1)

    A, Bm = draw(*((K, M) if op_a else (M, K))), draw(*((K, N) if op_b else (N, K)))
    assert float(A.abs().max()) < FP16_TINY and float(Bm.abs().max()) < FP16_TINY
    ref = _gemm_ref(A, Bm, op_a, op_b, rh)
    C = torch.empty(M, N, device=DEV)
    ops.gemm(op_a, op_b, M, N, K, A.to(DEV), A.shape[1], Bm.to(DEV), Bm.shape[1], C, N)
    flushed = _gemm_ref(A, Bm, op_a, op_b, lambda t: torch.where(t.abs() < 2.0**-14, torch.zeros_like(t), t).half().double())
    print(f"subnormal operands: vs .half() {rel_l2(C, ref):.3e}; |C| max {float(C.abs().max()):.3e}, |ref| max {float(ref.abs().max()):.3e}, flushed |ref| max {float(flushed.abs().max()):.3e}")
    assert rel_l2(C, ref) < 2e-6
    assert float(flushed.abs().max()) == 0.0 and float(C.abs().max()) > 1e-9  # flushed operands would give a zero product


@pytest.mark.parametrize("op_a,op_b,M,N,K,split", [(1, 1, 192, 768, 30000, 40), (1, 0, 384, 130, 20001, 24), (0, 1, 16385, 576, 192, 1), (1, 1, 96, 80, 4096, 16)])
def test_gemm_f16_split_k_wide_tiles_accumulate(op_a, op_b, M, N, K, split):
    """Split-K and accumulation with ldc > N.  Of the four shapes only (0, 1, 16385, 576, 192) runs on a wide tile today (128x192:
    the 16-bit modes have no weight-stationary path); the weight-gradient forms and 384 x 130 (144 tiles < 192) run on 64x64
    (`blvm_gemm_arm`).  Every wide tile of this mode, with the launch counters asserted: tests/test_gpu_gemm_arms.py."""
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(*((K, M) if op_a else (M, K)), generator=g)
    Bm = torch.randn(*((K, N) if op_b else (N, K)), generator=g)
    ref = _gemm_ref(A, Bm, op_a, op_b, rh)
    C = torch.full((M, N + 4), 2.0, device=DEV)
    ops.gemm(op_a, op_b, M, N, K, A.to(DEV), A.shape[1], Bm.to(DEV), Bm.shape[1], C, N + 4, accumulate=True, split_k=split)
    assert rel_l2(C[:, :N], ref + 2) < 3e-6
    assert torch.all(C[:, N:] == 2)


def test_wgrad_bias_gradient_stays_fp32_in_f16_mode():
    g = torch.Generator().manual_seed(4)
    N, K, rows = 256, 192, 9000
    D, X = torch.randn(rows, N, generator=g), torch.randn(rows, K, generator=g)
    dW, db = torch.zeros(N, K, device=DEV), torch.zeros(N, device=DEV)
    Dd, Xd = D.to(DEV), X.to(DEV)
    _hip.check(_hip.load().blvm_wgrad_f32(N, K, rows, _hip.ptr(Dd), N, _hip.ptr(Xd), K, _hip.ptr(dW), K, _hip.ptr(db), 0, _hip.stream_ptr()), "wgrad")
    assert rel_l2(dW, rh(D).t() @ rh(X)) < 3e-6
    assert rel_l2(db, D.double().sum(0)) < 3e-6  # NOT the sum of the rounded operands


@pytest.mark.parametrize("op_a,op_b", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_f16_overflow_is_halfs(op_a, op_b):
    """7e4 > 65520 rounds to inf as .half() does (no saturation, no truncation): exactly the outputs that use it are non-finite; 65519
    rounds to 65504 and stays finite; every other entry is exact."""
    M, N, K = 96, 80, 200
    g = torch.Generator().manual_seed(11 + op_a * 2 + op_b)
    A = torch.randn(M, K, generator=g)
    Bm = torch.randn(N, K, generator=g)
    A[5, 17] = 7e4  # row 5 of the output: +-inf
    A[9, 3] = 65519.0  # row 9: finite (65504)
    Bm[40, 100] = -7e4  # column 40: +-inf
    Ad = (A.t().contiguous() if op_a else A)
    Bd = (Bm.t().contiguous() if op_b else Bm)
    ref = rh(A) @ rh(Bm).t()
    C = torch.empty(M, N, device=DEV)
    ops.gemm(op_a, op_b, M, N, K, Ad.to(DEV), Ad.shape[1], Bd.to(DEV), Bd.shape[1], C, N)
    C = C.cpu()
    bad = ~torch.isfinite(ref)
    assert bad[5].all() and bad[:, 40].all() and int(bad.sum()) == M + N - 1
    assert torch.equal(~torch.isfinite(C), bad)
    both = bad & torch.isinf(ref) & torch.isinf(C)
    assert torch.equal(torch.sign(C[both]), torch.sign(ref[both]).float())
    assert rel_l2(C[~bad], ref[~bad]) < 2e-6
    assert torch.isfinite(C[9, torch.arange(N) != 40]).all() and float(rh(A)[9, 3]) == 65504.0


def _run(model, x, x_sl, eps, beta, fn, scale=SCALE):
    """one forward + backward of loss * scale; the gradients are divided by the scale again (GradScaler's unscale)."""
    model.zero_grad()
    loss, metrics, out = model(x.to(DEV), x_sl, beta=beta, free_nats=fn, eps=eps.to(DEV))
    (loss * scale).backward()
    with torch.no_grad():
        for p in model.parameters():
            p.grad /= scale
    return loss, metrics, out


def _flat_grad(model):
    return torch.cat([p.grad.detach().double().flatten().cpu() for p in model.parameters()])


def test_vrnn_full_dims_f16_delta_within_budget_and_below_bf16():
    """C2 dims on the golden inputs of `test_vrnn_full_dims_vs_reference_golden`: per-utterance ELBO / KL of the fp16 mode against the
    REFERENCE's fp32 values, and fp16 vs bf16 on the same inputs: ELBO delta and whole-gradient rel-L2 against the f32 path."""
    g = np.load(os.path.join(GOLDEN, "vrnn_full.npz"))
    torch.manual_seed(0)
    m = VRNNAudio(likelihood="DMoL", input_size=64, hidden_size=256, latent_size=256, residual_posterior=True).to(DEV)
    x, x_sl = O.synth_batch(4, 1280, seed=0, ragged=True)
    torch.manual_seed(123)
    eps = torch.stack([torch.randn(4, 256) for _ in range(20)], 0)
    frames = x_sl.double()
    res = {}
    for mode in ("f32", "bf16", "f16"):
        loss, _, out = _in(mode, lambda: _run(m, x, x_sl, eps, 1.0, 2.0))
        res[mode] = (float(loss), out.elbo.detach().cpu().double(), out.kl.detach().cpu().double(), _flat_grad(m), dict((k, p.grad.double().norm().item()) for k, p in m.named_parameters()))
    _, elbo16, kl16, g16, n16 = res["f16"]
    d_elbo = float(((elbo16 - T(g["elbo"]).double()).abs() / frames).max())
    d_kl = float(((kl16 - T(g["kl"]).double()).abs() / frames).max())
    assert 0.0 < d_elbo < NATS_PER_FRAME_BUDGET, d_elbo
    assert d_kl < NATS_PER_FRAME_BUDGET, d_kl
    assert res["f16"][0] == pytest.approx(float(g["loss"]), rel=1e-4)
    for name, ref in zip(g["grad_names"].tolist(), g["grad_norms"].tolist()):
        assert n16[name] == pytest.approx(ref, rel=3e-2), name
    de = {k: float(((res[k][1] - res["f32"][1]).abs() / frames).max()) for k in ("bf16", "f16")}
    dg = {k: rel_l2(res[k][3], res["f32"][3]) for k in ("bf16", "f16")}
    print(f"C2 vs f32 path: ELBO delta (nats/frame) bf16 {de['bf16']:.3e} f16 {de['f16']:.3e}; gradient rel-L2 bf16 {dg['bf16']:.3e} f16 {dg['f16']:.3e}; "
          f"f16 vs reference ELBO {d_elbo:.3e} KL {d_kl:.3e}")
    assert 0.0 < de["f16"] <= 0.5 * de["bf16"], de
    assert 0.0 < dg["f16"] <= 0.5 * dg["bf16"], dg


def _small(tag, scale):
    g = np.load(os.path.join(GOLDEN, "vrnn_small.npz"))
    m = VRNNAudio(likelihood="DMoL", input_size=8, hidden_size=32, latent_size=16, residual_posterior=True, num_mix=10, num_bins=2**16)
    m.load_state_dict({k[3:]: T(g[k]) for k in g.files if k.startswith("sd.")})
    m.to(DEV)
    beta, fn_ = (1.0, 2.0) if tag == "a" else (0.3, 0.0)
    loss, _, out = _run(m, T(g["x"]), T(g["x_sl"]), T(g[f"{tag}_eps"]), beta, fn_, scale=scale)
    return g, m, loss, out


@pytest.mark.parametrize("tag,worse", [("a", 1.2), ("b", 4.0)])
def test_vrnn_small_f16_against_reference_tensors(tag, worse):
    """Every tensor the small golden holds at fp16-operand distance from the reference's fp32 values, at bars tighter than the bf16
    test's (2e-2 on z / h_n, 0.15 per gradient): 1e-3 and 0.06 (first GPU run: z 1.9e-5, h_n 1.7e-4, worst gradient 3.9e-2).  At loss
    scale 1 the gradients below fp16's smallest normal number come out worse: the backward's operands (~1e-6) fall into fp16's
    subnormal range — the reason the GradScaler exists.  First run, median rel-L2 of those gradients at 2^16 / at 1: (a) 2.1e-2 /
    3.0e-2 (the free-nats case, where the forward's rounding dominates), (b) 6.0e-4 / 1.4e-2."""
    g, m, loss, out = _small(tag, SCALE)
    assert float(loss) == pytest.approx(float(g[f"{tag}_loss"]), rel=1e-3)
    ez, eh = rel_l2(out.z, T(g[f"{tag}_z"])), rel_l2(out.h_n, T(g[f"{tag}_h_n"]))
    assert ez > 1e-7  # not the fp32 path
    errs = {k: rel_l2(p.grad, T(g[f"{tag}_grad.{k}"])) for k, p in m.named_parameters()}
    worst = max(errs, key=errs.get)
    print(f"small {tag}: z {ez:.3e} h_n {eh:.3e} worst gradient {worst} {errs[worst]:.3e}")
    assert ez < 1e-3 and eh < 1e-3, (ez, eh)
    assert errs[worst] < 0.06, (worst, errs[worst])
    tiny = [k for k in errs if float(T(g[f"{tag}_grad.{k}"]).abs().max()) < FP16_TINY]
    assert tiny, "the small golden's gradients are all above fp16's normal range?"
    _, m1, _, _ = _small(tag, 1.0)
    errs1 = {k: rel_l2(p.grad, T(g[f"{tag}_grad.{k}"])) for k, p in m1.named_parameters()}
    scaled = float(np.median([errs[k] for k in tiny]))
    unscaled = float(np.median([errs1[k] for k in tiny]))
    print(f"small {tag}: {len(tiny)} gradients below 6.1e-5, median rel-L2 at scale 2^16 {scaled:.3e}, at scale 1 {unscaled:.3e}")
    assert unscaled > worse * scaled, (unscaled, scaled)


def test_f16_and_f32_steps_agree_on_headline_shape():
    """[16, 16000] at the headline widths: one train step in both modes on the same weights, noise and batch."""
    torch.manual_seed(0)
    m = VRNNAudio(likelihood="DMoL", input_size=64, hidden_size=256, latent_size=256, residual_posterior=True).to(DEV)
    x, x_sl = O.synth_batch(16, 16000, seed=1, ragged=True)
    eps = torch.randn(250, 16, 256, generator=torch.Generator().manual_seed(5))
    _, _, oh = _run(m, x, x_sl, eps, 1.0, 0.0)
    gh = _flat_grad(m)
    _, _, of = _in("f32", lambda: _run(m, x, x_sl, eps, 1.0, 0.0))
    gf = _flat_grad(m)
    d = float(((oh.elbo.cpu().double() - of.elbo.cpu().double()).abs() / x_sl.double()).max())
    cos = float((gh * gf).sum() / (gh.norm() * gf.norm()))
    print(f"headline: ELBO delta {d:.3e} nats/frame, gradient cosine {cos:.6f}")
    assert 0.0 < d < NATS_PER_FRAME_BUDGET, d
    assert cos > 0.999, cos


def test_srnn_f16_delta_within_budget():
    torch.manual_seed(0)
    m = SRNNAudio(likelihood="DMoL", input_size=64, hidden_size=256, latent_size=256, residual_posterior=True, smoothing=True).to(DEV)
    x, x_sl = O.synth_batch(8, 6400, seed=2, ragged=True)
    eps = torch.randn(100, 8, 256, generator=torch.Generator().manual_seed(7))
    _, _, oh = _run(m, x, x_sl, eps, 1.0, 0.0)
    _, _, of = _in("f32", lambda: _run(m, x, x_sl, eps, 1.0, 0.0))
    d = float(((oh.elbo.cpu().double() - of.elbo.cpu().double()).abs() / x_sl.double()).max())
    print(f"SRNN: ELBO delta {d:.3e} nats/frame")
    assert 0.0 < d < NATS_PER_FRAME_BUDGET, d


@pytest.mark.parametrize("tag,ragged", [("full", False), ("ragged", True)])
def test_lstm_c1_f16_against_reference_golden(tag, ragged):
    """BASELINE configs[0] through the register-resident LSTM sequence kernels with fp16 weight packs."""
    from blvm.models import LSTMAudio

    g = np.load(os.path.join(GOLDEN, "lstm.npz"))
    torch.manual_seed(0)
    m = LSTMAudio(stack_size=64, hidden_size=256, num_layers=1, num_mix=10, num_bins=2**16).to(DEV)
    x, x_sl = O.synth_batch(8, 4000, seed=0, ragged=ragged)
    loss, metrics, out = m(x.to(DEV), x_sl)
    (loss * SCALE).backward()
    d = float(((out.ll.detach().cpu().double() - T(g[f"{tag}_ll"]).double()).abs()).max())
    print(f"LSTM {tag}: loss {float(loss)} vs {float(g[f'{tag}_loss'])}, max |ll delta| {d:.3e}")
    assert float(loss) == pytest.approx(float(g[f"{tag}_loss"]), rel=1e-4)
    assert 0.0 < rel_l2(out.ll.detach(), T(g[f"{tag}_ll"])) < 1e-3
    grads = dict(m.named_parameters())
    for name, ref in zip(g["grad_names"].tolist(), g[f"{tag}_grad_norms"].tolist()):
        assert (grads[name].grad.double().norm().item() / SCALE) == pytest.approx(ref, rel=2e-2), name


def test_wavenet_c5_dims_f16_delta_within_budget():
    """C5 dims on the golden inputs of `test_wavenet_c5_dims_vs_reference_golden`, block kernels on the fp16 matrix pipe; gradient
    norms tighter than the bf16 test's 5e-2 (5e-3)."""
    from blvm.models import WaveNet
    from blvm.modules.distributions import DiscretizedLogisticMixtureDense

    g = np.load(os.path.join(GOLDEN, "wavenet.npz"))
    torch.manual_seed(0)
    lik = DiscretizedLogisticMixtureDense(96, 1, num_mix=10, num_bins=2**16)
    m = WaveNet(likelihood=lik, n_layers=10, n_stacks=5, res_channels=96, kernel_size=2, base_dilation=2, n_stack_frames=1).to(DEV)
    x, x_sl = O.synth_batch(2, 1500, seed=0, ragged=True)
    loss, metrics, out = m(x.to(DEV), x_sl)
    (loss * SCALE).backward()
    d = float(((out.log_prob.detach().cpu().double() - T(g["f_log_prob"]).double()).abs() / x_sl.double()).max())
    grads = dict(m.named_parameters())
    worst = max(abs(grads[n].grad.double().norm().item() / SCALE / r - 1) for n, r in zip(g["f_grad_names"].tolist(), g["f_grad_norms"].tolist()))
    print(f"WaveNet C5: log-prob delta {d:.3e} nats/frame, worst gradient-norm deviation {worst:.3e}")
    assert 0.0 < d < NATS_PER_FRAME_BUDGET, d
    assert float(loss) == pytest.approx(float(g["f_loss"]), rel=1e-4)
    assert worst < 5e-3, worst  # first GPU run: 4.2e-4


def _bench_step(name, B, T_, scale):
    sys.path.insert(0, ROOT)
    import bench

    m = bench.build_model(name, DEV)
    x, x_sl = O.synth_batch(B, T_, seed=3, ragged=False)

    def step():
        m.zero_grad()
        torch.manual_seed(9)
        loss, _, out = m(x.to(DEV), x_sl, beta=1.0, free_nats=4.0)
        (loss * scale).backward()
        return float(loss), _flat_grad(m) / scale

    return step


def test_stcn_f16_step_within_budget():
    step = _bench_step("stcn", 4, 8000, SCALE)
    lh, gh = step()
    lf, gf = _in("f32", step)
    print(f"stcn: loss f16 {lh} f32 {lf} (relative {abs(lh - lf) / abs(lf):.3e}), gradient rel-L2 {rel_l2(gh, gf):.3e}")
    assert np.isfinite(lh) and torch.isfinite(gh).all()
    assert 0.0 < abs(lh - lf) < 1e-4 * abs(lf), (lh, lf)  # 1e-4 relative (first GPU run: 1.2e-7)
    assert rel_l2(gh, gf) < 5e-3  # first GPU run: 2.7e-4


def test_cwvae_f16_forward_within_budget():
    """CW-VAE (which the reference does not train under --use_amp): the fp16 forward is within budget of the fp32 one (first GPU run:
    9.2e-5 relative).  Its backward at random init spans more than fp16's range: on the fp32 path the encoder's weight gradients reach
    3.7e5, so the fp16 gradients are non-finite at every scale >= 2^-5 while the loss-facing end underflows below it — GradScaler cannot
    place that span, and the bf16 mode is the one for this model.  Asserted: the forward, and the fp32 gradient range that explains it."""
    step = _bench_step("cwvae", 2, 16384, 1.0)
    m_loss_h, _ = step()
    lf, gf = _in("f32", step)
    print(f"cwvae: loss f16 {m_loss_h} f32 {lf} (relative {abs(m_loss_h - lf) / abs(lf):.3e}), fp32 gradient max {float(gf.abs().max()):.3e}")
    assert np.isfinite(m_loss_h)
    assert 0.0 < abs(m_loss_h - lf) < 1e-4 * abs(lf), (m_loss_h, lf)
    assert float(gf.abs().max()) > 65504.0


def test_one_launch_decoders_in_f16_mode():
    """The sampling programs with fp16 weight packs: finite, in range, and close to the fp32 roll-out on the first stack."""
    B, T_ = 8, 6
    g = torch.Generator().manual_seed(13)
    torch.manual_seed(23)
    v = VRNNAudio(likelihood="DMoL", input_size=16, hidden_size=32, latent_size=16, residual_posterior=True).to(DEV)
    eps = torch.randn(T_, B, 16, generator=g).to(DEV)
    uni = (torch.empty(T_, B, 16, 10).uniform_(1e-5, 1 - 1e-5, generator=g).to(DEV), torch.empty(T_, B, 16).uniform_(1e-8, 1 - 1e-8, generator=g).to(DEV))
    x0 = (torch.rand(B, 16, 1, generator=g) * 0.2 - 0.1).to(DEV)
    (h, _), _ = v.generate(n_samples=B, max_timesteps=T_, x=x0, eps=eps, uniforms=uni, fused=True)
    (a, _), _ = _in("f32", lambda: v.generate(n_samples=B, max_timesteps=T_, x=x0, eps=eps, uniforms=uni, fused=True))
    assert torch.isfinite(h).all() and float(h.abs().max()) <= 1.0
    assert float(((a[:, :2] - h[:, :2]).abs() > 2e-2).float().mean()) < 0.1
    assert not torch.equal(a, h)
    _hip.check_async()


def _vrnn_step(B, Tp, H=256, seed=0):
    S = 64
    torch.manual_seed(seed)
    m = VRNNAudio(likelihood="DMoL", input_size=S, hidden_size=H, latent_size=H, residual_posterior=True).to(DEV)
    g = torch.Generator().manual_seed(seed + 1)
    x = (torch.rand(B, Tp * S, generator=g) * 2 - 1)
    x_sl = torch.randint(Tp * S // 2, Tp * S + 1, (B,), generator=g, dtype=torch.int64)
    x_sl[0] = Tp * S
    eps = torch.randn(Tp, B, H, generator=g)
    return m, x, x_sl, eps


@pytest.mark.timeout(300)
def test_static_walk_selector_is_a_no_op_in_f16_mode():
    """The static-walk kernels decline 16-bit programs: at their shape (B = 16, H = Z = 256) the selector on and off give identical
    results, and no static launch is counted."""
    lib = _hip.load()
    was = lib.blvm_pchain_static(-1)
    m, x, x_sl, eps = _vrnn_step(16, 20)
    res = []
    try:
        for static in (1, 0):
            lib.blvm_pchain_static(static)
            n0 = lib.blvm_pchain_static(-2)
            loss, _, out = _run(m, x, x_sl, eps, 1.0, 2.0)
            torch.cuda.synchronize()
            res.append((lib.blvm_pchain_static(-2) - n0, loss.detach().clone(), out.elbo.detach().clone(), out.z.detach().clone(), out.h_n.detach().clone(), _flat_grad(m)))
    finally:
        lib.blvm_pchain_static(was)
    assert res[0][0] == res[1][0] == 0
    for a, b in zip(res[0][1:5], res[1][1:5]):
        assert torch.equal(a, b)
    assert rel_l2(res[0][5], res[1][5]) < 1e-6  # (float atomics of the weight gradients)
    assert _hip.take_async_errors() == (0, 0)


@pytest.mark.timeout(300)
def test_f16_step_at_b65_within_budget():
    """B = 65: the row-group kernels decline 16-bit operands (fp32 there), the rest of the step is in fp16 mode as in bf16 mode."""
    m, x, x_sl, eps = _vrnn_step(65, 20)
    _, _, oh = _run(m, x, x_sl, eps, 1.0, 2.0)
    gh = _flat_grad(m)
    _, _, of = _in("f32", lambda: _run(m, x, x_sl, eps, 1.0, 2.0))
    gf = _flat_grad(m)
    d = float(((oh.elbo.cpu().double() - of.elbo.cpu().double()).abs() / x_sl.double()).max())
    assert torch.isfinite(gh).all()
    assert 0.0 < d < NATS_PER_FRAME_BUDGET, d
    assert rel_l2(gh, gf) < 2e-2
    assert _hip.take_async_errors() == (0, 0)


@pytest.mark.timeout(300)
def test_grad_scaler_overflow_step_through_the_persistent_chain():
    """Every fp16 run meets this in its first steps: at an excessive scale (2^40) the backward chain's fp16 operands overflow.  NaN /
    inf words are not the hand-off sentinel 0xFFFFFFFF, so no bounded poll trips; GradScaler skips the step (parameters and Adam state
    unchanged) and lowers the scale; the next step at 2^16 is finite and taken."""
    sys.path.insert(0, os.path.join(ROOT, "experiments"))
    import _common as C

    m, x, x_sl, eps = _vrnn_step(16, 25)  # [16, 1600]
    params = list(m.parameters())
    opt = torch.optim.Adam(params, lr=1e-4)
    _hip.take_async_errors()

    def step(scaler):
        opt.zero_grad(set_to_none=True)
        loss, _, _ = m(x.to(DEV), x_sl, beta=1.0, free_nats=2.0, eps=eps.to(DEV))
        scaler.scale(loss).backward()
        torch.cuda.synchronize()
        assert _hip.take_async_errors() == (0, 0)
        return C.clip_and_step(params, opt, 1000.0, 3000.0, False, scaler)

    assert step(torch.amp.GradScaler("cuda", init_scale=SCALE))  # Adam holds moments now
    before = [p.detach().clone() for p in params]
    state = [{k: v.clone() for k, v in opt.state[p].items()} for p in params]
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0**40, growth_interval=2000)
    assert not step(scaler)
    assert not all(torch.isfinite(p.grad).all() for p in params)  # the overflow reached the gradients
    assert scaler.get_scale() == 2.0**39
    for p, b, st in zip(params, before, state):
        assert torch.equal(p.detach(), b)
        for k, v in st.items():
            assert torch.equal(opt.state[p][k], v)
    scaler.update(SCALE)
    assert step(scaler)
    assert all(torch.isfinite(p).all() for p in params)
    assert any(not torch.equal(p.detach(), b) for p, b in zip(params, before))


@pytest.mark.timeout(600)
def test_experiment_vrnn_f16_amp_end_to_end():
    env = dict(os.environ)
    cmd = [sys.executable, os.path.join(ROOT, "experiments", "experiment_vrnn_audio.py"), "--dataset", "synthetic", "--use_amp", "True",
           "--amp_dtype", "f16", "--epochs", "1", "--synthetic_utterances", "16", "--synthetic_length", "6400", "--batch_size", "8",
           "--hidden_size", "256", "--latent_size", "256", "--stack_frames", "64", "--test_every", "1", "--seed", "1"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=540, cwd=ROOT)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    assert "--use_amp: f16 matrix operands" in r.stderr and "GradScaler" in r.stderr
    assert "step(s) skipped: non-finite gradient norm (loss scale" in r.stdout
    line = next(ln for ln in r.stdout.splitlines() if "frames/s" in ln)
    loss = float(line.split("loss ")[1].split(",")[0])
    assert np.isfinite(loss), line
