"""GPU (MI355X): training steps at the frame-stack sizes 1 and 256 of the reference's benchmark table (`experiments/benchmarks.txt`
trains every sequence model at s = 1, 64 and 256; the other model tests stop at 64), and WaveNet / STCN at 128.

What these sizes reach that no other test does: at S = 256 the DMoL rows kernel walks four 64-frame units per stack row (the last
stack of the batch is half padding, so units lie wholly beyond T and beyond the shorter lengths), the decoder's last layer is
7680 wide (forward, data gradient over K = 7680, weight gradient with N = 7680), and stride = ceil(T / T') = 214 is not the stack
size: x_sl = 500 is 3 steps to the KL mask (ceil(500 / 214)) and 2 stacks to the likelihood mask.  At S = 1 the encoder's first layer
is a reduction of length 1 (forward and weight gradient) and the batch holds a one-sample utterance.

VRNNAudio, SRNNAudio(smoothing) and LSTMAudio (hidden 32, latent 16), each at S in {1, 256}:
  * against the reference's own outputs (tests/golden/stack_sizes.npz, oracle/gen_golden.py::gen_stack_sizes; weights from the seed,
    pinned by checksums; tests/test_oracle_golden.py pins the fp32 oracle to the same fixture), at the bars of
    test_vrnn_small_vs_reference_golden / test_vrnn_full_dims_vs_reference_golden: loss 1e-5, elbo / log_prob rtol 1e-5 atol 1e-3,
    kl rtol 1e-5 atol 1e-4, states rtol 1e-4 atol 1e-5, metrics 1e-5, gradient norms 1e-3, stored gradients rel-L2 < 1e-3;
  * every gradient against the float64 oracle: rel-L2 <= max(4 x the fp32 oracle's own rel-L2 to float64, 1e-5)
    (test_dmol_forward_backward_vs_oracle's rule; the three numbers are printed per tensor);
  * VRNN and SRNN on both execution paths (persistent chain programs and one launch per link), which agree at 1e-6 on loss and ELBO.
A VRNN with a non-zero initial state and B = 19 (a partial row tile) against the oracle, as
test_vrnn_vs_oracle_ragged_with_initial_state.  WaveNet (head without a Linear of its own: W = NULL) and STCN at S = 128 against their
oracles at the bars of test_wavenet_on_frame_stacks_vs_reference_golden / test_stcn_small_matches_reference.

Measured on an MI355X (err / bar, <= 1 passes; every case of this file runs in under a second, the file in 3.5 s):
  * gradients against float64, worst tensor per case -- hip vs float64 | fp32 oracle vs float64 (largest over tensors) | worst err / bar:
      VRNN S = 1     6.9e-7 | 7.6e-7 | 0.07   (both paths)      VRNN S = 256   3.4e-6 | 1.7e-6 | 0.34 (engine 0.334, per link 0.339)
      SRNN S = 1     8.6e-7 | 9.7e-7 | 0.09   (both paths)      SRNN S = 256   2.4e-6 | 1.1e-6 | 0.24 (both paths)
      LSTM S = 1     2.0e-7 | 2.2e-7 | 0.02                     LSTM S = 256   8.1e-7 | 4.8e-7 | 0.08
      VRNN S = 256, B = 19, h0 != 0:  2.2e-6 | 1.1e-6 | 0.22
    (the fp32 oracle is within 2e-6 of float64 everywhere, so the floor of 1e-5 is the bar for every tensor);
  * persistent programs against one launch per link: VRNN loss 8.4e-10 / ELBO 2.1e-9 (S = 1), 1.1e-10 / 2.5e-10 (S = 256); SRNN the
    same bits on both paths at both sizes;
  * the per-frame head cases of tests/test_gpu_heads.py::test_dmol_per_frame_vs_float64 with several units per row (S = 128 both
    layouts, 192 without a Linear, 256 at B = 2 and B = 400, 128 unaligned), worst err / bar: ll 0.072 (65536 bins) / 0.099 (256 bins),
    per-utterance sums <= 0.011, d_dec 0.038 / 0.128 -- the figures of the S = 64 rows, as the same frames are evaluated.
"""
import functools

import numpy as np
import pytest
import torch

import blvm_oracle as O
from blvm import _hip

from test_oracle_golden import STACK_SIZES_BETA as BETA, STACK_SIZES_FREE_NATS as FREE_NATS, stack_sizes_oracle, stack_sizes_setup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATHS = {"engine": 128, "per_link": 0}  # blvm_pchain_configure's first argument: largest batch the persistent programs take


@pytest.fixture(scope="module", autouse=True)
def _require_hip():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert _hip.load().blvm_device_ok() == 1, "libblvm_hip: no gfx950 device visible"
    yield
    _hip.load().blvm_pchain_configure(128, -1)


def T(a):
    return torch.from_numpy(np.asarray(a))


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def oracle_grads(fwd, sd, dtype):
    """Gradients of the oracle's loss in `dtype`; fwd(sd) -> the oracle's output dict."""
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    out = fwd(leaves)
    out["loss"].backward()
    return out, {k: v.grad for k, v in leaves.items()}


def check_grads_vs_float64(label, named_grads, g32, g64):
    """rel-L2(hip, f64) <= max(4 rel-L2(oracle32, f64), 1e-5) for every tensor; prints the three numbers, returns the worst err / bar."""
    worst, fails = 0.0, []
    for k, got in named_grads:
        e, e32 = rel_l2(got, g64[k]), rel_l2(g32[k], g64[k])
        bar = max(4 * e32, 1e-5)
        print(f"[{label}] {k}: hip vs float64 {e:.3e}  fp32 oracle vs float64 {e32:.3e}  bar {bar:.3e}")
        worst = max(worst, e / bar)
        if not e <= bar:
            fails.append((k, e, e32, bar))
    print(f"[{label}] worst err / bar over {len(named_grads)} tensors: {worst:.3f}")
    assert not fails, fails
    return worst


@functools.lru_cache(maxsize=None)
def reference_case(kind, S):
    """Set-up and both oracles of one (model, S), computed once for every path."""
    m, x, x_sl, eps, g, tag = stack_sizes_setup(kind, S, cks_rel=1e-6)  # (this host's CPU: the same tensors to float32 rounding)
    sd = m.state_dict()
    run = lambda dt: oracle_grads(lambda leaves: stack_sizes_oracle(kind, S, leaves, x.to(dt), x_sl, None if eps is None else eps.to(dt)), sd, dt)  # noqa: E731
    (_, g32), (_, g64) = run(torch.float32), run(torch.float64)
    return m.to(DEV), x, x_sl, eps, g, tag, g32, g64


def run_model(kind, m, x, x_sl, eps, path):
    for p in m.parameters():
        p.grad = None
    if path is not None:
        _hip.load().blvm_pchain_configure(PATHS[path], -1)
    try:
        if kind == "lstm":
            loss, metrics, out = m(x.to(DEV), x_sl)
        else:
            loss, metrics, out = m(x.to(DEV), x_sl, beta=BETA, free_nats=FREE_NATS, eps=eps.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
        _hip.check_async()
    finally:
        _hip.load().blvm_pchain_configure(128, -1)
    return loss.detach(), metrics, out, [(k, p.grad.clone()) for k, p in m.named_parameters()]


@pytest.mark.parametrize("S", [1, 256])
@pytest.mark.parametrize("kind", ["vrnn", "srnn", "lstm"])
def test_models_at_stack_sizes_vs_reference_and_float64(kind, S):
    m, x, x_sl, eps, g, tag, g32, g64 = reference_case(kind, S)
    B, T_ = x.shape
    Tp = -(-T_ // S)
    stride = -(-T_ // Tp)
    if S == 256 and kind != "lstm":  # the two masks count a whole step apart for one utterance
        assert stride == 214 and any(-(-n // stride) != -(-n // S) for n in x_sl.tolist()), (stride, x_sl)
    results = {}
    for path in ([None] if kind == "lstm" else list(PATHS)):
        label = f"stack_sizes {kind} S={S} path={path or 'only'}"
        loss, metrics, out, grads = run_model(kind, m, x, x_sl, eps, path)
        results[path] = (loss, out)
        assert float(loss) == pytest.approx(float(g[f"{tag}_loss"]), rel=1e-5), label
        if kind == "lstm":
            assert loss.dtype == torch.float32
            torch.testing.assert_close(out.ll.cpu(), T(g[f"{tag}_log_prob"]), rtol=1e-5, atol=1e-3)
            torch.testing.assert_close(out.s_n[0].cpu(), T(g[f"{tag}_h_n"]), rtol=1e-4, atol=1e-5)
            torch.testing.assert_close(out.s_n[1].cpu(), T(g[f"{tag}_c_n"]), rtol=1e-4, atol=1e-5)
            assert out.reconstruction_mode.shape == (B, (Tp - 1) * S, 1)
        else:
            assert loss.dtype == torch.float64
            torch.testing.assert_close(out.elbo.cpu(), T(g[f"{tag}_elbo"]), rtol=1e-5, atol=1e-3)
            torch.testing.assert_close(out.log_prob.cpu(), T(g[f"{tag}_log_prob"]), rtol=1e-5, atol=1e-3)
            torch.testing.assert_close(out.kl.cpu(), T(g[f"{tag}_kl"]), rtol=1e-5, atol=1e-4)
            if kind == "vrnn":
                torch.testing.assert_close(out.h_n.cpu(), T(g[f"{tag}_h_n"]), rtol=1e-4, atol=1e-5)
            else:
                for k in ("d_n", "a_n", "z_n"):
                    torch.testing.assert_close(getattr(out, k).cpu(), T(g[f"{tag}_{k}"]), rtol=1e-4, atol=1e-5)
            assert out.reconstructions_mode.shape == (B, T_, 1)  # S = 256: [3, 640, 1], as the reference
        assert out.z_sl.tolist() == g[f"{tag}_z_sl"].tolist()
        vals = {mm.name: mm.value for mm in metrics}
        for name, val in zip(g[f"{tag}_metric_names"].tolist(), g[f"{tag}_metric_values"].tolist()):
            assert vals[name] == pytest.approx(val, rel=1e-5, abs=1e-7), (label, name)
        gd = dict(grads)
        for name, norm in zip(g[f"{tag}_grad_names"].tolist(), g[f"{tag}_grad_norms"].tolist()):
            assert gd[name].double().norm().item() == pytest.approx(norm, rel=1e-3), (label, name)
        pre = f"{tag}_grad."
        stored = [f[len(pre):] for f in g.files if f.startswith(pre)]
        assert len(stored) >= 2
        for k in stored:
            assert rel_l2(gd[k], T(g[pre + k])) < 1e-3, (label, k)
        check_grads_vs_float64(label, grads, g32, g64)
    if kind != "lstm":
        (l0, o0), (l1, o1) = results["engine"], results["per_link"]
        d_loss = abs(float(l0) - float(l1)) / abs(float(l1))
        d_elbo = float(((o0.elbo - o1.elbo).abs() / o1.elbo.abs()).max())
        print(f"[stack_sizes {kind} S={S}] engine vs per-link: loss rel {d_loss:.3e}, elbo rel {d_elbo:.3e}")
        assert d_loss <= 1e-6 and d_elbo <= 1e-6, (d_loss, d_elbo)


@pytest.mark.parametrize("path", list(PATHS))
def test_vrnn_stack_256_initial_state_partial_row_tile_vs_oracle(path):
    """h0 != 0 and B = 19 (one full 16-row tile and a partial one) at S = 256, ragged: against the oracle only, at the bars of
    test_vrnn_vs_oracle_ragged_with_initial_state plus the float64 rule."""
    from blvm.models import VRNNAudio

    S, B, T_ = 256, 19, 640
    torch.manual_seed(4)
    m = VRNNAudio(likelihood="DMoL", input_size=S, hidden_size=32, latent_size=16, residual_posterior=True)
    x, x_sl = O.synth_batch(B, T_, seed=9, ragged=True)
    assert any(-(-n // 214) != -(-n // S) for n in x_sl.tolist())
    gen = torch.Generator().manual_seed(8)
    eps = torch.randn(3, B, 16, generator=gen)
    h0 = torch.randn(B, m.state_dict()["vrnn.vrnn_cell.gru_cell.weight_hh"].size(1), generator=gen) * 0.3
    fwd = lambda dt: lambda leaves: O.vrnn_audio_forward(leaves, x.to(dt), x_sl, eps.to(dt), beta=0.7, free_nats=1.5, h0=h0.to(dt), stack=S)  # noqa: E731
    (ref, g32), (_, g64) = (oracle_grads(fwd(dt), m.state_dict(), dt) for dt in (torch.float32, torch.float64))
    m.to(DEV)
    _hip.load().blvm_pchain_configure(PATHS[path], -1)
    try:
        loss, _, out = m(x.to(DEV), x_sl, beta=0.7, free_nats=1.5, eps=eps.to(DEV), h0=h0.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
        _hip.check_async()
    finally:
        _hip.load().blvm_pchain_configure(128, -1)
    assert float(loss) == pytest.approx(float(ref["loss"]), rel=1e-5)
    torch.testing.assert_close(out.elbo.cpu(), ref["elbo"].detach(), rtol=1e-5, atol=1e-3)
    grads = [(k, p.grad) for k, p in m.named_parameters()]
    for k, gr in grads:
        assert rel_l2(gr, g32[k]) < 1e-3, k
    check_grads_vs_float64(f"stack_sizes vrnn S=256 B=19 h0 path={path}", grads, g32, g64)


def test_wavenet_stack_128_vs_oracle():
    """WaveNet on 128-sample frames (the head kernel with W = NULL, two units per row), smallest widths, ragged: fp32 oracle at the
    bars of test_wavenet_on_frame_stacks_vs_reference_golden."""
    from blvm.models import WaveNet
    from blvm.modules.distributions import DiscretizedLogisticMixtureDense

    S, B, T_ = 128, 3, 5 * 128 - 64
    torch.manual_seed(12)
    lik = DiscretizedLogisticMixtureDense(16, 1, num_mix=10, num_bins=2**16)
    m = WaveNet(likelihood=lik, n_layers=2, n_stacks=1, res_channels=16, kernel_size=2, base_dilation=2, n_stack_frames=S)
    x, x_sl = O.synth_batch(B, T_, seed=S, ragged=True)
    sd = {k: v.clone().requires_grad_(True) for k, v in m.state_dict().items()}
    xr = x.clone().requires_grad_(True)
    ref = O.wavenet_forward(sd, xr, x_sl, n_layers=2, n_stacks=1, n_stack_frames=S)
    ref["loss"].backward()
    m.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    loss, _, out = m(xd, x_sl)
    loss.backward()
    assert float(loss) == pytest.approx(float(ref["loss"]), rel=1e-5)
    torch.testing.assert_close(out.log_prob.cpu(), ref["log_prob"].detach(), rtol=1e-5, atol=1e-3)
    assert rel_l2(xd.grad, xr.grad) < 1e-3
    for k, p in m.named_parameters():
        assert rel_l2(p.grad, sd[k].grad) < 1e-3, k


def test_stcn_stack_128_vs_oracle():
    """STCN on 128-sample frames (the head after a single up-projection), test_gpu_stcn.py's smallest model, ragged: loss / ELBO /
    log-likelihood 1e-4 against the fp32 oracle, gradients against the float64 oracle no further than max(2 x the fp32 oracle's
    distance, 1e-3) (test_stcn_small_matches_reference's bars, the fp32 oracle standing for the reference it is pinned to)."""
    from blvm.models import STCN

    S, B, T_ = 128, 3, 5 * 128 - 64
    Tp = 5
    lat = [16, 16, 32]
    torch.manual_seed(13)
    m = STCN(likelihood="DMoL", n_layers=3, latent_size=lat, res_channels=16, n_stack_frames=S)
    x, x_sl = O.synth_batch(B, T_, seed=S + 1, ragged=True)
    gen = torch.Generator().manual_seed(14)
    eps = [torch.randn(B, Tp, z, generator=gen) for z in lat]  # [B,T',z] as the reference draws them
    fwd = lambda dt: lambda leaves: O.stcn_forward(leaves, x.to(dt), x_sl, [e.to(dt) for e in eps], n_layers=3, latent_size=lat,  # noqa: E731
                                                   n_stack_frames=S, beta=0.8, free_nats=1.0)
    (ref, g32), (_, g64) = (oracle_grads(fwd(dt), m.state_dict(), dt) for dt in (torch.float32, torch.float64))
    m.to(DEV)
    loss, _, out = m(x.to(DEV), x_sl, beta=0.8, free_nats=1.0, eps=[e.transpose(0, 1).contiguous().to(DEV) for e in eps])
    loss.backward()
    for got, want in ((loss, ref["loss"]), (out.elbo, ref["elbo"]), (out.log_prob, ref["log_prob"])):
        torch.testing.assert_close(got.detach().double().cpu(), want.detach().double(), rtol=1e-4, atol=0)
    for k, p in m.named_parameters():
        if g64[k] is None or float(g64[k].abs().max()) == 0.0:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        e, e32 = rel_l2(p.grad, g64[k]), rel_l2(g32[k], g64[k])
        assert e <= max(2 * e32, 1e-3), (k, e, e32)
