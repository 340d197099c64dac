"""Cached WaveNet generation from an audio prompt, resumable in chunks (`WaveNet.generate(x=prompt, cached=True)`,
`return_state` / `state`; `blvm_wavenet_decode_ring_fill`, `blvm_wavenet_decode_resume`).

Reference: `generate_f64`, the loop of `blvm_oracle.wavenet_generate` (pinned to the reference by tests/golden/generate.npz) with
the initial window as an argument, in float64.  `test_restatement_equals_the_oracle_from_a_zero_window` ties the two.

Regime: at default initialisation half the samples clamp to +-1 and a prompt barely moves the output, so every case scales the
residual blocks' weights by 2, the output transform's and the head's by 3 and sets the head's log-scale biases to -5 (a
trained-like network: narrow components, a prompt moves the samples by 0.1 .. 2, fewer than half of the samples clamp).

Comparison rule: a Gumbel-max tie would flip a component and every later sample, so ties are excluded by construction — each
case asserts (on the CPU, `test_cases_have_no_near_ties`) that the smallest float64 gap between the best and the second-best
perturbed logit over all rows and frames is >= 1e-3 — and then EVERY sample must lie within 1e-4 of the float64 restatement
(the threshold of `test_wavenet_decode_kernel_matches_window_generation`), none left out."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import blvm_oracle as O

gpu = pytest.mark.gpu
DEV = "cuda:0"
TOL, MIN_GAP = 1e-4, 1e-3


class Case:
    def __init__(self, name, B, C, layers, stacks, num_mix, n_frames, seed):
        self.name, self.B, self.C, self.layers, self.stacks = name, B, C, layers, stacks
        self.num_mix, self.n_frames, self.seed = num_mix, n_frames, seed
        self.dilations = O.wavenet_dilations(layers, stacks, 2)
        self.rf = sum(self.dilations) + 2


#           B   C  layers stacks K  n_frames seed      rf     kernel
SHAPES = {
    "g16": Case("g16", 3, 16, 4, 2, 10, 24, 8),  # 32      <8,0,0>: every ring (d <= 8) wraps
    "r32": Case("r32", 19, 32, 5, 2, 10, 20, 51),  # 64    <8,32,32>: look-ahead slots, partial group 16 + 3
    "r64": Case("r64", 1, 64, 10, 5, 10, 12, 65),  # 5117  <8,64,64>: 512-deep rings part prompt, part zero pad
    "g128": Case("g128", 40, 128, 3, 1, 10, 12, 168),  # 9  <8,0,0>: three workgroups, last one partial
    "mix11": Case("mix11", 3, 16, 4, 2, 11, 24, 8),  # 32  3 * 11 > 32 head rows: block by block
}
# (shape, prompt length): P < rf zero pad, P == rf exact window, P > rf trimming; none a multiple of the larger dilations
ZERO_STARTS = [("g16", 0), ("r64", 0)]  # P = 0: no prompt
PRIMED = [("g16", 11), ("g16", 32), ("g16", 40), ("r32", 70), ("r64", 601), ("g128", 9), ("mix11", 11), ("mix11", 40)]


def build_model(case):
    """The case's network in the trained-like regime (CPU, fp32)."""
    from blvm.models import WaveNet
    from blvm.modules.distributions import DiscretizedLogisticMixtureDense

    torch.manual_seed(case.seed)
    m = WaveNet(likelihood=DiscretizedLogisticMixtureDense(case.C, 1, num_mix=case.num_mix, num_bins=2**16), n_layers=case.layers,
                n_stacks=case.stacks, res_channels=case.C)  # fmt: skip
    assert m.receptive_field == case.rf and list(m.res_stack.dilations) == list(case.dilations)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith("weight") and k.startswith("res_stack.res_blocks"):
                p.mul_(2.0)
            elif k in ("out_transform.linear.weight", "likelihood.params.weight"):
                p.mul_(3.0)
        m.likelihood.params.bias[2 * case.num_mix :] = -5.0  # the log-scales
    return m


def draws(case, P, n_frames=None, offset=0):
    """-> prompt [B,P,1] uniform in [-0.8, 0.8] and n_frames pairs (u [B,1,K], v [B,1]) of uniform draws."""
    g = torch.Generator().manual_seed(case.seed + offset)
    n = case.n_frames if n_frames is None else n_frames
    prompt = torch.rand(case.B, max(P, 1), 1, generator=g) * 1.6 - 0.8
    uni = [(torch.empty(case.B, 1, case.num_mix).uniform_(1e-5, 1 - 1e-5, generator=g), torch.empty(case.B, 1).uniform_(1e-8, 1 - 1e-8, generator=g))
           for _ in range(n)]  # fmt: skip
    return prompt[:, :P], uni


def window_of(prompt, rf):
    """The last rf samples of prompt [B,P,1], zeros in front of a shorter one -> [B,rf,1]."""
    w = prompt[:, -rf:]
    return F.pad(w, (0, 0, rf - w.size(1), 0))


def generate_f64(sd, window, n_frames, n_layers, n_stacks, uniforms, num_mix=10, base_dilation=2):
    """`O.wavenet_generate` from a given window [B,rf,1] instead of zeros, in the dtype of `sd`.  -> (x [B,n_frames,1], the smallest
    gap between the best and the second-best perturbed logit over all rows and frames)."""
    dil = O.wavenet_dilations(n_layers, n_stacks, base_dilation)
    rf = sum(dil) + 1 + (sd["causal.conv.weight"].size(2) - 1)
    dt = sd["causal.conv.weight"].dtype
    assert tuple(window.shape[1:]) == (rf, 1)
    x = window.to(dt).transpose(1, 2)  # [B,1,rf]
    scale = math.sqrt(n_layers / n_stacks)
    out, gap = [], float("inf")
    for t in range(n_frames):
        h = F.conv1d(x, sd["causal.conv.weight"], sd["causal.conv.bias"])
        skips = sum(O.residual_stack_skips(sd, "res_stack", h, dil, 1)) / scale  # [B,C,1]
        o = F.relu(F.linear(F.relu(skips.transpose(1, 2)), sd["out_transform.linear.weight"], sd["out_transform.linear.bias"]))
        logits, locs, log_scales = O.dmol_head(o, sd["likelihood.params.weight"], sd["likelihood.params.bias"], num_mix)
        u, v = uniforms[t][0].to(dt), uniforms[t][1].to(dt).reshape(-1, 1, 1)
        top = (logits - torch.log(-torch.log(u))).topk(2, dim=-1).values
        gap = min(gap, float((top[..., 0] - top[..., 1]).min()))
        pred = O.dmol_sample(logits, locs, log_scales, u, v)  # [B,1,1]
        out.append(pred)
        x = torch.cat([x[:, :, 1:], pred], dim=2)
    return torch.hstack(out), gap


@functools.lru_cache(maxsize=None)
def reference(name, P):
    """(model on the CPU, prompt, draws, float64 samples [B,n,1], smallest gap) of a primed case — computed once, never changed.
    P == 0: the zero start."""
    case = SHAPES[name]
    m = build_model(case)
    prompt, uni = draws(case, P)
    sd64 = {k: v.detach().double() for k, v in m.state_dict().items()}
    x64, gap = generate_f64(sd64, window_of(prompt, case.rf), case.n_frames, case.layers, case.stacks, uni, case.num_mix)
    return m, prompt, uni, x64, gap


# ---- the decode kernel's arm with a skip width other than the residual width ------------------------------------------
# The model always builds skip_channels = res_channels and an output transform of that width, so this arm is reached with
# hand-made parameters only (`ops.wavenet_decode` takes the tensors as they are).
class SkipCase:
    B, C, S, O, num_mix, n_frames, seed = 19, 32, 16, 48, 10, 12, 9  # one full group of 16 rows and a partial one; S != C != O
    dilations = (1, 2, 4, 1, 2)  # five blocks: an odd count, so the any-width kernel <8,0,0> runs; 12 frames: every ring wraps
    inv_std, skip_scale, log_eps = math.sqrt(0.5), 1.0 / math.sqrt(2.5), -7.0  # (skip_scale: five blocks as if in two stacks)


def skip_case_parameters():
    """Hand-made fp32 parameters at torch's default initialisation (uniform in +-1/sqrt(fan_in)), in the regime of `build_model`:
    the blocks' weights x 2, the output transform's and the head's x 3, the head's log-scale biases -5.
    -> (causal, in_transform, blocks, out_linear, head_linear) as `ops.wavenet_decode` takes them."""
    c = SkipCase
    g = torch.Generator().manual_seed(c.seed)

    def init(fan_in, *shape, gain=1.0):
        return (torch.rand(*shape, generator=g) * 2 - 1) * (gain / math.sqrt(fan_in))

    causal = (init(2, c.C, 1, 2), init(2, c.C))
    in_transform = (init(c.C, c.C, c.C), init(c.C, c.C))
    blocks = [(init(2 * c.C, 2 * c.C, c.C, 2, gain=2.0), init(2 * c.C, 2 * c.C), init(c.C, c.C + c.S, c.C, gain=2.0), init(c.C, c.C + c.S))
              for _ in c.dilations]  # fmt: skip
    out_linear = (init(c.S, c.O, c.S, gain=3.0), init(c.S, c.O))
    head_b = init(c.O, 3 * c.num_mix)
    head_b[2 * c.num_mix :] = -5.0
    return causal, in_transform, blocks, out_linear, (init(c.O, 3 * c.num_mix, c.O, gain=3.0), head_b)


@functools.lru_cache(maxsize=None)
def skip_case_reference():
    """The cached formulation (arXiv:1611.09482) of the hand-made network in float64, restated in plain torch: one ring per block,
    started from the steady state under an all-zero past.  -> (parameters, u [n,B,K], v [n,B], x64 [B,n], the smallest gap between
    the best and the second-best perturbed logit) — computed once, never changed."""
    c = SkipCase
    params = skip_case_parameters()
    g = torch.Generator().manual_seed(c.seed + 1)
    u = torch.empty(c.n_frames, c.B, c.num_mix).uniform_(1e-5, 1 - 1e-5, generator=g)
    v = torch.empty(c.n_frames, c.B).uniform_(1e-8, 1 - 1e-8, generator=g)
    f64 = lambda ts: tuple(t.double() for t in ts)  # noqa: E731
    (cw, cb), (iw, ib), (ow, ob), (hw, hb) = f64(params[0]), f64(params[1]), f64(params[3]), f64(params[4])
    blocks = [f64(b) for b in params[2]]
    C, K = c.C, c.num_mix

    def front(x_prev, x_new):  # causal conv (kernel 2) on the two newest samples -> 1x1 in_transform
        return F.linear(x_prev[:, None] * cw[:, 0, 0] + x_new[:, None] * cw[:, 0, 1] + cb, iw, ib)

    def block(i, old, h):  # -> (the next block's input, the skip half)
        kw, kb, rw, rb = blocks[i]
        pre = F.linear(old, kw[:, :, 0]) + F.linear(h, kw[:, :, 1]) + kb
        rs = F.linear(torch.tanh(pre[:, :C]) * torch.sigmoid(pre[:, C:]), rw, rb)
        return (rs[:, :C] + h) * c.inv_std, rs[:, C:]

    x_prev = x_new = torch.zeros(c.B, dtype=torch.float64)
    h, rings = front(x_prev, x_new), []
    for i, d in enumerate(c.dilations):  # an input constant in time: both taps see it, every slot holds it
        rings.append(h.repeat(d, 1, 1))
        h, _ = block(i, h, h)
    out, gap = [], float("inf")
    for t in range(c.n_frames):
        h, skip = front(x_prev, x_new), 0.0
        for i, d in enumerate(c.dilations):
            old = rings[i][t % d].clone()
            rings[i][t % d] = h
            h, s = block(i, old, h)
            skip = skip + s
        par = F.linear(F.relu(F.linear(F.relu(skip * c.skip_scale), ow, ob)), hw, hb)
        top = (par[:, :K] - torch.log(-torch.log(u[t].double()))).topk(2, dim=-1)
        gap = min(gap, float((top.values[:, 0] - top.values[:, 1]).min()))
        best = top.indices[:, :1]
        loc, raw = par[:, K : 2 * K].gather(1, best)[:, 0], par[:, 2 * K :].gather(1, best)[:, 0]
        vt = v[t].double()
        x = (loc + torch.exp(raw.clamp(min=c.log_eps)) * (torch.log(vt) - torch.log(1 - vt))).clamp(-1, 1)
        out.append(x)
        x_prev, x_new = x_new, x
    return params, u, v, torch.stack(out, 1), gap


# ----------------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------------


def test_restatement_equals_the_oracle_from_a_zero_window():
    case = SHAPES["g16"]
    m = build_model(case)
    _, uni = draws(case, 0)
    for dt in (torch.float32, torch.float64):
        sd = {k: v.detach().to(dt) for k, v in m.state_dict().items()}
        ours, _ = generate_f64(sd, torch.zeros(case.B, case.rf, 1), case.n_frames, case.layers, case.stacks, uni, case.num_mix)
        before = torch.get_default_dtype()
        torch.set_default_dtype(dt)  # (the oracle's zero window takes the default dtype)
        try:
            ref = O.wavenet_generate(sd, case.B, case.n_frames, case.layers, case.stacks, [(u.to(dt), v.to(dt).reshape(-1, 1, 1)) for u, v in uni],
                                     num_mix=case.num_mix)  # fmt: skip
        finally:
            torch.set_default_dtype(before)
        assert ours.dtype == dt and tuple(ours.shape) == (case.B, case.n_frames, 1)
        assert torch.equal(ours, ref)


@pytest.mark.parametrize("name,P", PRIMED + ZERO_STARTS)
def test_cases_have_no_near_ties(name, P):
    """The precondition of the every-sample comparison, and that the regime is what the header says: the prompt matters."""
    case = SHAPES[name]
    _, prompt, uni, x64, gap = reference(name, P)
    assert tuple(x64.shape) == (case.B, case.n_frames, 1) and bool(torch.isfinite(x64).all())
    assert gap >= MIN_GAP, f"{name} P={P}: perturbed-logit gap {gap:.2e}: pick another seed"
    if P and (name, 0) in ZERO_STARTS:
        assert float((x64 - reference(name, 0)[3]).abs().max()) > 0.05
    assert float((x64.abs() >= 1).double().mean()) < 0.5


def test_skip_width_case_has_no_near_ties():
    """The precondition of `test_gpu_parity.py::test_wavenet_decode_kernel_with_a_skip_width_of_its_own`, and its regime."""
    c = SkipCase
    _, _, _, x64, gap = skip_case_reference()
    assert tuple(x64.shape) == (c.B, c.n_frames) and bool(torch.isfinite(x64).all())
    assert gap >= MIN_GAP, f"perturbed-logit gap {gap:.2e}: pick another seed"
    assert float((x64.abs() >= 1).double().mean()) < 0.5
    assert float(x64.std()) > 0.05  # (the samples are no constant)


def test_prime_and_state_arguments_are_checked_without_a_device():
    m = build_model(SHAPES["g16"])
    with pytest.raises(NotImplementedError):
        m.generate(3, 4, cached=False, return_state=True)
    with pytest.raises(ValueError):
        m.generate(3, 4, x=torch.zeros(2, 5, 1), cached=True)
    with pytest.raises(ValueError):
        m.generate(3, 4, x=torch.zeros(3, 5, 1), state=object(), cached=True)


# ----------------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------------


def _lib():
    from blvm import _hip

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    lib = _hip.load()
    assert lib.blvm_device_ok() == 1, "libblvm_hip: no gfx950 device visible"
    return lib


def _dev(uni):
    return [(u.to(DEV), v.to(DEV)) for u, v in uni]


@functools.lru_cache(maxsize=None)
def gpu_model(name):
    return build_model(SHAPES[name]).to(DEV)


def _report(tag, got, want):
    err = (got.detach().cpu().double() - want.double()).abs()
    print(f"{tag}: max |diff| {float(err.max()):.3e}, samples beyond {TOL:g}: {int((err > TOL).sum())} of {err.numel()}")
    return err


@gpu
@pytest.mark.parametrize("name,P", PRIMED)
def test_primed_generation_matches_float64_and_the_window_path(name, P):
    """generate(x=prompt, cached=True): one launch from primed rings (block by block for `mix11`) against the float64 restatement
    and against the window path generate(x=window, cached=False) on the same draws; every sample within 1e-4.
    Measured on an MI355X: max |diff| to float64 2.9e-7 .. 5.7e-7 and to the window path 3.6e-7 .. 7.2e-7 over the six kernel cases."""
    _lib()
    case = SHAPES[name]
    _, prompt, uni, x64, gap = reference(name, P)
    assert gap >= MIN_GAP
    m = gpu_model(name)
    assert m._decode_kernel_applies() == (name != "mix11")
    got = m.generate(n_samples=case.B, n_frames=case.n_frames, x=prompt.to(DEV), uniforms=_dev(uni), cached=True)
    assert tuple(got.shape) == (case.B, case.n_frames, 1) and bool(torch.isfinite(got).all())
    err = _report(f"{name} P={P} primed vs float64", got, x64)
    win = m.generate(n_samples=case.B, n_frames=case.n_frames, x=window_of(prompt, case.rf).to(DEV), uniforms=_dev(uni), cached=False)
    err_w = _report(f"{name} P={P} primed vs window path", got, win.cpu())
    assert float(err.max()) <= TOL
    assert float(err_w.max()) <= TOL
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("P", [11, 40])
def test_block_by_block_path_takes_the_primed_state(P):
    """`_generate_cached` called directly on the g16 shape (num_mix = 10) with the primed rings, in two chunks: the fallback's
    ring phases and sample hand-over at the head width every audio model uses (the `mix11` cases reach it through `generate`)."""
    _lib()
    case = SHAPES["g16"]
    _, prompt, uni, x64, gap = reference("g16", P)
    assert gap >= MIN_GAP
    m = gpu_model("g16")
    uni, n = _dev(uni), 7
    first, state = m._generate_cached(case.B, n, uni[:n], state=m._prime(prompt.to(DEV)), want_state=True)
    assert state.n_frames == P + n
    rest, state = m._generate_cached(case.B, case.n_frames - n, uni[n:], state=state, want_state=True)
    assert state.n_frames == P + case.n_frames
    err = _report(f"g16 P={P} block by block, primed, two chunks vs float64", torch.cat([first, rest], 1), x64)
    assert float(err.max()) <= TOL


@gpu
@pytest.mark.parametrize("name", ["g16", "r64"])
def test_zero_prompt_equals_the_zero_start(name):
    """A prompt of rf zeros is the all-zero past: primed rings == the steady-state fill, within 1e-4 on every sample."""
    _lib()
    case = SHAPES[name]
    _, _, uni, x64, gap = reference(name, 0)
    assert gap >= MIN_GAP
    m = gpu_model(name)
    a = m.generate(n_samples=case.B, n_frames=case.n_frames, uniforms=_dev(uni), cached=True)
    b = m.generate(n_samples=case.B, n_frames=case.n_frames, x=torch.zeros(case.B, case.rf, 1, device=DEV), uniforms=_dev(uni), cached=True)
    err = _report(f"{name} zero prompt vs zero start", b, a.cpu())
    err64 = _report(f"{name} zero prompt vs float64", b, x64)
    assert float(err.max()) <= TOL and float(err64.max()) <= TOL


@gpu
@pytest.mark.parametrize("name,P,n", [("g16", 11, 5), ("g16", 0, 7), ("r32", 70, 9), ("r32", 0, 7), ("r64", 601, 5), ("r64", 0, 3), ("mix11", 11, 5), ("mix11", 0, 7)])
def test_generation_in_two_chunks_is_bit_identical(name, P, n):
    """2n frames in one call == n frames with return_state=True, then n frames from the state: the same kernel and the same order
    of arithmetic.  n is odd and smaller than the largest dilation (8, 16, 512), so the split lands inside the rings; P = 0 is the
    zero start, whose first call is the steady-state entry."""
    _lib()
    case = SHAPES[name]
    assert n % 2 == 1 and n < max(case.dilations) and 2 * n <= case.n_frames
    prompt, uni = draws(case, P)
    m = gpu_model(name)
    uni = _dev(uni)[: 2 * n]
    kw = dict(x=prompt.to(DEV)) if P else {}
    whole = m.generate(n_samples=case.B, n_frames=2 * n, uniforms=uni, cached=True, **kw)
    first, state = m.generate(n_samples=case.B, n_frames=n, uniforms=uni[:n], cached=True, return_state=True, **kw)
    assert state.n_frames == P + n and tuple(state.samples.shape) == (case.B, 2)
    assert torch.equal(state.samples[:, 1], first[:, -1, 0]) and torch.equal(state.samples[:, 0], first[:, -2, 0])
    second, state2 = m.generate(n_samples=case.B, n_frames=n, uniforms=uni[n:], cached=True, state=state, return_state=True)
    assert state2.n_frames == P + 2 * n and torch.equal(state2.samples[:, 1], second[:, -1, 0])
    chunks = torch.cat([first, second], 1)
    assert tuple(chunks.shape) == tuple(whole.shape) == (case.B, 2 * n, 1)
    print(f"{name} P={P} n={n}: max |whole - chunks| {float((whole - chunks).abs().max()):.3e}")
    assert torch.equal(whole, chunks)


@gpu
@pytest.mark.parametrize("d", [1, 3, 8])
def test_ring_fill_places_frame_tau_in_slot_tau_mod_d(d):
    """`blvm_wavenet_decode_ring_fill` alone, B = 19: h[j] is absolute frame t0 - L + j; slot tau mod d holds frame tau for the last
    d frames, and nothing outside the ring is written."""
    from blvm import ops

    _lib()
    B, C = 19, 16
    for t0 in (d, d + 1, 2 * d + 5):
        for L in (d, d + 3):
            h = (torch.arange(L * B * C, dtype=torch.float32).view(L, B, C) + 1).to(DEV)
            buf = torch.full(((d + 2) * B * C,), -7.0, device=DEV)
            ring = buf[B * C : (d + 1) * B * C].view(d, B, C)
            ops.wavenet_ring_fill(h, d, t0, ring)
            torch.cuda.synchronize()
            for tau in range(t0 - d, t0):
                assert torch.equal(ring[tau % d], h[L - (t0 - tau)]), (d, t0, L, tau)
            assert bool((buf[: B * C] == -7.0).all()) and bool((buf[(d + 1) * B * C :] == -7.0).all())


def _pack(m):
    """The packed weight image of `blvm_wavenet_decode` (include/blvm_hip.h) of a model on the device."""
    rs, lik = m.res_stack, m.likelihood
    hw, hb = lik.params.weight, lik.params.bias
    parts = [m.causal.conv.weight, m.causal.conv.bias, rs.in_transform.weight, rs.in_transform.bias]
    for b in rs.res_blocks:
        parts += list(b.kernel_params())
    parts += [m.out_transform.linear.weight, m.out_transform.linear.bias, hw, hw.new_zeros(32 - hw.shape[0], hw.shape[1]), hb, hb.new_zeros(32 - hb.numel())]
    return torch.cat([p.detach().float().reshape(-1) for p in parts])


@gpu
def test_new_exports_do_not_depend_on_what_their_buffers_held():
    """Ring fill + decode-from-a-state through the C ABI, twice: the ring region of the scratch buffer, the weight copies in front
    of it, the [B,2] state output and the samples pre-filled with NaN, then with zeros.  Identical bits; rows >= B of the last
    16-row group of the outputs stay as they were; priming writes every ring slot the decoder reads."""
    from blvm import ops

    lib = _lib()
    name, P = "r32", 70
    case = SHAPES[name]
    B, C, n = case.B, case.C, case.n_frames
    _, prompt, uni, x64, _ = reference(name, P)
    m = gpu_model(name)
    rs = m.res_stack
    dil = (ctypes.c_int * len(case.dilations))(*case.dilations)
    nb = len(case.dilations)
    packed = _pack(m)
    assert packed.numel() == lib.blvm_wavenet_decode_pack_floats(C, C, C, nb)
    u = torch.stack([a.reshape(B, case.num_mix) for a, _ in uni]).to(DEV).contiguous()
    v = torch.stack([b.reshape(B) for _, b in uni]).to(DEV).contiguous()
    # block inputs over the window, from the model's own pieces (every activation kept: the shape is tiny)
    win = window_of(prompt, case.rf)[:, :, 0].t().contiguous().unsqueeze(-1).to(DEV)  # [rf,B,1]
    out = m.causal.forward_tm(win, pad_causal=True)
    L = out.size(0)
    t_in = rs.in_transform
    h0 = ops.linear(out.reshape(L * B, C), t_in.weight.view(C, C), t_in.bias).view(L, B, C)
    samples = window_of(prompt, case.rf)[:, -2:, 0].contiguous().to(DEV)
    total = lib.blvm_wavenet_decode_scratch_floats(dil, nb, B, C, C)
    off = lib.blvm_wavenet_decode_ring_offset_floats(nb, C, C)
    assert off == nb * ((2 * C) ** 2 + (C + C) * C) and total - off == sum(case.dilations) * B * C
    Bp = 16 * ((B + 15) // 16)
    results = []
    for fill in (float("nan"), 0.0):
        scratch = torch.full((total,), fill, device=DEV)
        x_out = torch.full((Bp, n), fill, device=DEV)
        x_state = torch.full((Bp, 2), fill, device=DEV)
        rings = ops.wavenet_ring_views(scratch, case.dilations, B, C, C)
        ops.wavenet_prime_rings(h0, [b.kernel_params() for b in rs.res_blocks], case.dilations, rs.res_blocks[0].inv_std, C, P, rings)
        rc = lib.blvm_wavenet_decode_resume(packed.data_ptr(), dil, nb, B, C, C, C, case.num_mix, n, P, rs.res_blocks[0].inv_std,
                                            1.0 / m.variance_scale, m.likelihood.log_epsilon, u.data_ptr(), v.data_ptr(), samples.data_ptr(),
                                            scratch.data_ptr(), x_out.data_ptr(), x_state.data_ptr(), None)  # fmt: skip
        assert rc == 0
        torch.cuda.synchronize()
        results.append((x_out.cpu(), x_state.cpu(), scratch[off:].cpu()))
    (xa, sa, ra), (xb, sb, rb) = results
    # the outputs are [B,n] / [B,2] inside buffers of Bp rows: what lies behind them keeps its fill
    assert bool(torch.isnan(xa.view(-1)[B * n :]).all()) and bool((xb.view(-1)[B * n :] == 0).all())
    assert bool(torch.isnan(sa.view(-1)[B * 2 :]).all()) and bool((sb.view(-1)[B * 2 :] == 0).all())
    xa, xb, sa, sb = xa.view(-1)[: B * n], xb.view(-1)[: B * n], sa.view(-1)[: B * 2], sb.view(-1)[: B * 2]
    assert bool(torch.isfinite(xa).all()) and bool(torch.isfinite(sa).all()) and bool(torch.isfinite(ra).all())
    assert torch.equal(xa.view(torch.int32), xb.view(torch.int32))
    assert torch.equal(sa.view(torch.int32), sb.view(torch.int32))
    assert torch.equal(ra.view(torch.int32), rb.view(torch.int32))
    assert torch.equal(sa.view(B, 2)[:, 1], xa.view(B, n)[:, -1]) and torch.equal(sa.view(B, 2)[:, 0], xa.view(B, n)[:, -2])
    err = _report("C ABI primed decode vs float64", xa.view(B, n, 1), x64)
    assert float(err.max()) <= TOL
