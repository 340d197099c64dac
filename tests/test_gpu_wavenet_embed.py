"""GPU: WaveNet with embedded class input (K10e): the fused front (`blvm_wavenet_embed_tables` / `_fwd` / `_bwd`), the model against
the unmodified reference's golden, and generation on all three paths (`blvm_wavenet_embed_cat_decode` / `_resume`).

References, bounds and the tie rule are in tests/wavenet_embed_cases.py: the front per element against float64 with derived bounds,
generation with EVERY class equal to the float64 restatement (its cases keep every draw MIN_GAP from a CDF boundary, asserted on the
CPU by tests/test_wavenet_embed_cpu.py) and every returned float `dequantize(class)` to the bit."""
import functools
import os

import numpy as np
import pytest
import torch

import wavenet_embed_cases as W
from conftest import GOLDEN
from test_gpu_buffer_contract import poisoned

gpu = pytest.mark.gpu
DEV = "cuda:0"


def _lib():
    from blvm import _hip

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    lib = _hip.load()
    assert lib.blvm_device_ok() == 1, "libblvm_hip: no gfx950 device visible"
    return lib


def _ratio(got, want64, bound):
    """max over elements of |got - want| / bound (0 / 0 counts as 0: an exact value where nothing may be wrong)."""
    err = (got.detach().double().cpu() - want64).abs()
    assert tuple(err.shape) == tuple(bound.shape)
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


# ---- 1: the front, forward ---------------------------------------------------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("shape", W.FRONT_SHAPES)
@pytest.mark.parametrize("pad_causal", [False, True])
def test_front_forward_per_element(shape, pad_causal):
    """out = causal(pad(embedding(k))) per element against float64 within (2m + 2) 2^-24 sum|terms|; leading -1 frames, classes 0 and
    V - 1; the tables' padding row is exact zeros."""
    from blvm import ops

    _lib()
    c, out64, bound = W.front_reference(shape, pad_causal)
    k, emb, cw, bias = (c[n].to(DEV) for n in ("k", "emb", "cw", "bias"))
    P = ops.wavenet_embed_tables(emb, cw)
    assert tuple(P.shape) == (2, c["V"] + 1, c["C"]) and bool((P[:, c["V"]] == 0).all())
    got = ops.wavenet_embed_front(k, emb, cw, bias, pad_causal)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(out64.shape)
    r = _ratio(got, out64, bound)
    print(f"front fwd V={shape[0]} C={shape[1]} m={shape[2]} pad_causal={pad_causal}: largest |err| / bound {r:.3f}")
    assert r <= 1.0
    assert torch.equal(got, ops.wavenet_embed_lookup(P, bias, k, pad_causal))


# ---- 2: the front, backward --------------------------------------------------------------------------------------------------------------

BWD_CASES = [(s, True, None) for s in W.FRONT_SHAPES] + [(W.FRONT_SHAPES[1], False, None), (W.SKEWED, True, 0.9)]


@gpu
@pytest.mark.parametrize("shape,pad_causal,skew", BWD_CASES)
def test_front_backward_per_element_and_bit_identical(shape, pad_causal, skew, monkeypatch):
    """dE, dcw, db per element against float64 autograd within n 2^-24 sum|terms|; a class without a frame has an exactly zero
    gradient; a second call gives the same bits; every output and workspace is pre-filled with NaN words first."""
    from blvm import ops

    _lib()
    c, grads64, bounds, empty = W.grad_reference(shape, pad_causal, skew)
    k, d_out = c["k"].to(DEV), c["d_out"][pad_causal].to(DEV)

    def run():
        params = [c[n].to(DEV).requires_grad_(True) for n in ("emb", "cw", "bias")]
        ops.wavenet_embed_front(k, *params, pad_causal).backward(d_out)
        return [p.grad for p in params]

    with poisoned(monkeypatch, "nan") as h:
        first = run()
    assert h.count >= 7  # tables, out | G, workspace, dE, dcw, db
    second = run()
    for name, a, b, want, bound in zip(("dE", "dcw", "db"), first, second, grads64, bounds):
        assert not bool(torch.isnan(a).any()), name
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name}: two calls differ"
        r = _ratio(a, want, bound)
        print(f"front bwd V={shape[0]} C={shape[1]} m={shape[2]} skew={skew} {name}: largest |err| / bound {r:.3f}")
        assert r <= 1.0, name
    assert bool((first[0].cpu()[empty] == 0).all()), "a class without a frame has a non-zero gradient"


# ---- 3: the model against the reference's golden -------------------------------------------------------------------------------------------


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.double()
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


@gpu
@pytest.mark.parametrize("tag", list(W.FIXTURES))
@pytest.mark.parametrize("float_x", [False, True])
def test_model_vs_reference_golden(tag, float_x):
    """Loss, log_prob, ll and every parameter gradient (embedding.weight included) at the tolerances of
    test_tiny_wavenet_vs_reference_golden; x as classes and as the floats levels[k], which quantise back to k."""
    _lib()
    g = np.load(os.path.join(GOLDEN, "wavenet_embed.npz"))
    T_ = lambda n: torch.from_numpy(g[f"{tag}.{n}"])  # noqa: E731
    m = W.fixture_model(g, tag).to(DEV)
    k = T_("x").to(DEV)
    x = m.levels[k].unsqueeze(-1) if float_x else k  # (the model's table: computed on the host, like `Quantize`'s boundaries)
    loss, metrics, out = m(x, T_("x_sl"), pad_receptive_field=W.FIXTURES[tag][2])
    loss.backward()
    assert float(loss.detach()) == pytest.approx(float(g[f"{tag}.loss"]), rel=1e-5)
    torch.testing.assert_close(out.log_prob.cpu(), T_("log_prob"), rtol=1e-5, atol=1e-3)
    torch.testing.assert_close(out.log_prob_twise.cpu().float(), T_("ll"), rtol=1e-4, atol=1e-4)
    assert torch.equal(out.y.squeeze(-1).cpu(), T_("y"))
    for name, p in m.named_parameters():
        r = rel_l2(p.grad, T_(f"grad.{name}"))
        assert r < 1e-3, (name, r)
    assert len(metrics) == 3


# ---- 4: generation ---------------------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def gpu_model(name):
    return W.build_model(W.SHAPES[name]).to(DEV)


def _dev(uni):
    return [u.to(DEV) for u in uni]


def _check_classes(tag, got, k64, lik):
    """got [B,n,1] floats == dequantize(k64) to the bit: the classes and the table at once."""
    want = lik.dequantize(k64.to(DEV))
    k_got = torch.bucketize(got.squeeze(-1), lik.levels)
    wrong = int((k_got.cpu() != k64).sum())
    print(f"{tag}: classes that differ {wrong} of {k64.numel()}")
    assert got.dtype == torch.float32 and tuple(got.shape) == (*k64.shape, 1)
    assert wrong == 0, f"{tag}: {wrong} of {k64.numel()} classes differ from the float64 restatement"
    assert torch.equal(got.squeeze(-1).view(torch.int32), want.view(torch.int32)), f"{tag}: a value is not dequantize(k) to the bit"


def _forbid_block_steps(monkeypatch):
    from blvm import ops

    def refuse(*a, **k):
        raise AssertionError("the block-by-block path ran")

    monkeypatch.setattr(ops, "wavenet_block_step", refuse)


@gpu
@pytest.mark.parametrize("name,P", W.STARTS)
def test_one_launch_generation_matches_float64(name, P, monkeypatch):
    """generate(cached=True) from the zero start (a past of class 0) and from a prompt of classes, with the block-by-block path's
    kernel wrapper made to raise: every class the float64 restatement's, every value dequantize(k) to the bit."""
    _lib()
    case = W.SHAPES[name]
    _, prompt, uni, r = W.reference(name, P)
    assert r["gap"] >= W.MIN_GAP
    m = gpu_model(name)
    assert m._cat_decode_kernel_applies() is True
    _forbid_block_steps(monkeypatch)
    kw = dict(x=prompt.to(DEV)) if P else {}
    got = m.generate(n_samples=case.B, n_frames=case.n_frames, uniforms=_dev(uni), cached=True, **kw)
    _check_classes(f"{name} P={P} one launch vs float64", got, r["k"], m.likelihood)


@gpu
@pytest.mark.parametrize("name,P", [("e16", 0), ("e16", 11), ("e64m2", 0), ("e64", 77)])
def test_one_launch_window_and_block_by_block_paths_return_equal_tensors(name, P):
    """The three paths on the same draws; a float prompt levels[k] [B,P,1] is quantised back to the classes k."""
    _lib()
    case = W.SHAPES[name]
    _, prompt, uni, r = W.reference(name, P)
    m = gpu_model(name)
    uni = _dev(uni)
    kw = dict(x=prompt.to(DEV)) if P else {}
    one = m.generate(n_samples=case.B, n_frames=case.n_frames, uniforms=uni, cached=True, **kw)
    win = m.generate(n_samples=case.B, n_frames=case.n_frames, uniforms=uni, cached=False, **kw)
    state = m._prime(prompt.to(DEV)) if P else None
    blk = m._generate_cached(case.B, case.n_frames, uni, state=state)
    _check_classes(f"{name} P={P} one launch", one, r["k"], m.likelihood)
    assert torch.equal(one, win), "one launch vs the window path"
    assert torch.equal(one, blk), "one launch vs block by block"
    if P:
        floats = m.likelihood.dequantize(prompt.to(DEV)).unsqueeze(-1)
        assert torch.equal(one, m.generate(n_samples=case.B, n_frames=case.n_frames, uniforms=uni, cached=True, x=floats))


@gpu
@pytest.mark.parametrize("name,P,n", [("e16", 11, 5), ("e16", 0, 7), ("e64m2", 70, 9), ("e64m2", 0, 7), ("e64", 77, 5), ("e64", 0, 7)])
def test_generation_in_two_chunks_is_bit_identical(name, P, n, monkeypatch):
    """2n frames in one call == n frames with return_state=True, then n frames from the state, which keeps the two newest CLASSES."""
    _lib()
    case = W.SHAPES[name]
    assert n % 2 == 1 and n < max(case.dilations) and 2 * n <= case.n_frames
    prompt, uni = W.draws(case, P)
    m = gpu_model(name)
    lik = m.likelihood
    _forbid_block_steps(monkeypatch)
    uni = _dev(uni)[: 2 * n]
    kw = dict(x=prompt.to(DEV)) if P else {}
    whole = m.generate(n_samples=case.B, n_frames=2 * n, uniforms=uni, cached=True, **kw)
    first, state = m.generate(n_samples=case.B, n_frames=n, uniforms=uni[:n], cached=True, return_state=True, **kw)
    assert state.n_frames == P + n and tuple(state.samples.shape) == (case.B, 2) and state.samples.dtype == torch.int32
    assert torch.equal(lik.dequantize(state.samples), first[:, -2:, 0])
    second, state2 = m.generate(n_samples=case.B, n_frames=n, uniforms=uni[n:], cached=True, state=state, return_state=True)
    assert state2.n_frames == P + 2 * n and torch.equal(lik.dequantize(state2.samples[:, 1]), second[:, -1, 0])
    chunks = torch.cat([first, second], 1)
    assert tuple(chunks.shape) == tuple(whole.shape) == (case.B, 2 * n, 1)
    assert torch.equal(whole.view(torch.int32), chunks.view(torch.int32))
    assert len(whole.unique()) >= 4  # (no constant output)


@gpu
def test_sampling_without_given_uniforms_and_the_dmol_refusal():
    from blvm.models import WaveNet
    from blvm.modules.distributions import DiscretizedLogisticMixtureDense

    _lib()
    case = W.SHAPES["e64m2"]
    m = gpu_model("e64m2")
    torch.manual_seed(3)
    free = m.generate(n_samples=case.B, n_frames=case.n_frames, cached=True)
    kf = torch.bucketize(free.squeeze(-1), m.likelihood.levels)
    assert tuple(free.shape) == (case.B, case.n_frames, 1)
    assert torch.equal(m.likelihood.dequantize(kf), free.squeeze(-1)) and len(kf.unique()) >= 8
    dmol = WaveNet(likelihood=DiscretizedLogisticMixtureDense(16, 1, num_mix=10, num_bins=256), embedding_dim=16, num_bins=32, n_layers=2,
                   n_stacks=2, res_channels=16).to(DEV)  # fmt: skip
    for cached in (False, True):
        with pytest.raises(NotImplementedError, match="categorical head"):
            dmol.generate(2, 3, cached=cached)
