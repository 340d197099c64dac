"""One-launch generation from VRNN, SRNN and LSTM at frame stacks of any size (`blvm_vrnn_generate`, `blvm_srnn_generate`,
`blvm_lstm_generate_any_stack` with S % 16 != 0: the frame-stack operand and the last decoder layer padded inside the scratch, pchain.h
stack_pad), and roll-outs cut into several launches by a bound on the scratch (`max_scratch_floats`).

Shapes (tests/test_generate_any_stack_cpu.py says what each exercises): S in {1, 5, 8, 24}, B in {1, 5, 17}, H = 32, Z = 16, T from
3 to 7.  tests/test_generate_any_stack_cpu.py replays the padded program on the host and should run first.

Bars, all taken from the tests of the multiples of 16:
  reference fixture (tests/golden/generate.npz, S = 8): VRNN use_mode rtol 1e-4 / atol 2e-5; SRNN sampled: fewer than 2 % of the
    elements off by more than 1e-4 (tests/test_gpu_parity.py)
  one launch against step by step: share of |diff| > 2e-4 below 0.02 (test_vrnn_one_launch_decoder_matches_stepwise_generation); the
    seeds below were chosen so that the observed share (printed) stays at or below 0.005; returned state at rel-L2 2e-5 where nothing flipped
  LSTM against the float64 restatement: 1e-4 on samples, rel-L2 2e-5 on h_n and c_n, both paths within 1e-4 of each other
    (tests/test_gpu_lstm_generate.py)
  chunked against unchunked: torch.equal

Measured on an MI355X (fp32 operands): reference fixture VRNN max |diff| 6.0e-08, SRNN share 0.0000 (max 1.2e-07); one launch against
step by step: share 0.0000 in all 14 cases (max |diff| <= 1.2e-07), rel-L2 of h_n <= 7.9e-08, of d_n <= 9.7e-08; LSTM one launch max
|x - x64| <= 6.2e-07, rel-L2 h_n <= 9.7e-08, c_n <= 7.2e-08, step by step <= 1.8e-07 / 1.1e-07 / 7.0e-08, the two paths within 4.8e-07.
"""
import copy
import functools
import os

import numpy as np
import pytest
import torch

from blvm import _hip, ops
from blvm.models import VRNNAudio

from test_generate_any_stack_cpu import CASES, reference
from test_lstm_generate_cpu import MIN_GAP

gpu = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
X_TOL, S_TOL = 1e-4, 2e-5
HID, LAT = 32, 16
# (S, B, T, use_mode): every S with B = 17, every B with S = 1
SHAPES = [(1, 1, 7, False), (1, 5, 5, False), (1, 17, 7, False), (5, 17, 4, False), (8, 17, 3, False), (24, 17, 3, False), (5, 5, 4, True)]
SHAPE_IDS = [f"S{s}-B{b}{'-mode' if m else ''}" for s, b, _, m in SHAPES]


def T(a):
    return torch.from_numpy(np.asarray(a))


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def share(a, b, tol=2e-4):
    return float(((a - b).abs() > tol).float().mean())


# ---- 1. against the reference's own samples (S = 8) -------------------------------------------------------------------------------


@gpu
def test_vrnn_one_launch_matches_reference_at_stack_8():
    g = np.load(os.path.join(GOLDEN, "generate.npz"))
    m = VRNNAudio(likelihood="DMoL", input_size=8, hidden_size=32, latent_size=16, residual_posterior=True, num_mix=10, num_bins=2**16)
    m.load_state_dict({k[6:]: T(g[k]) for k in g.files if k.startswith("vr_sd.")})
    m = m.to(DEV)
    (x, x_sl), _ = m.generate(n_samples=3, max_timesteps=6, use_mode=True, eps=T(g["vr_eps"]).to(DEV), fused=True)
    assert tuple(x.shape) == tuple(g["vr_x"].shape) and x_sl.tolist() == g["vr_x_sl"].tolist()
    print(f"VRNN S=8 one launch against the reference: max |diff| {float((x.cpu() - T(g['vr_x'])).abs().max()):.2e}")
    torch.testing.assert_close(x.cpu(), T(g["vr_x"]), rtol=1e-4, atol=2e-5)
    _hip.check_async("VRNN.generate")


@gpu
def test_srnn_one_launch_matches_reference_at_stack_8():
    from blvm.models import SRNNAudio

    g = np.load(os.path.join(GOLDEN, "generate.npz"))
    m = SRNNAudio(likelihood="DMoL", input_size=8, hidden_size=32, latent_size=16, residual_posterior=True, smoothing=True)
    m.load_state_dict({k[6:]: T(g[k]) for k in g.files if k.startswith("sr_sd.")})
    m = m.to(DEV)
    uni = [(u.to(DEV), u2.to(DEV)) for u, u2 in zip(T(g["sr_u"]), T(g["sr_u2"]))]
    x0 = torch.zeros(3, 1, 8, device=DEV)
    (x, x_sl), out = m.srnn.generate(x=x0, n_samples=3, max_timesteps=5, eps=T(g["sr_eps"]).to(DEV), uniforms=uni, fused=True)
    assert tuple(x.shape) == tuple(g["sr_x"].shape) and x_sl.tolist() == g["sr_x_sl"].tolist()
    diff = (x.cpu() - T(g["sr_x"])).abs()
    off = float((diff > 1e-4).float().mean())
    print(f"SRNN S=8 one launch against the reference: share of |diff| > 1e-4 {off:.4f}, max {float(diff.max()):.2e}")
    assert off < 0.02, off
    assert tuple(out.h_p.shape) == (3, 64 + 16) and bool(torch.isfinite(out.h_p).all())
    _hip.check_async("SRNN.generate")


# ---- 2. one launch against step by step -------------------------------------------------------------------------------------------


def draws(S, B, T_, seed):
    g = torch.Generator().manual_seed(seed)
    eps = torch.randn(T_, B, LAT, generator=g).to(DEV)
    u = torch.empty(T_, B, S, 10).uniform_(1e-5, 1 - 1e-5, generator=g).to(DEV)
    v = torch.empty(T_, B, S).uniform_(1e-8, 1 - 1e-8, generator=g).to(DEV)
    x0 = (torch.rand(B, S, generator=g) * 0.2 - 0.1).to(DEV)
    return eps, u, v, x0


@functools.lru_cache(maxsize=None)
def vrnn_model(S):
    torch.manual_seed(40 + S)
    return VRNNAudio(likelihood="DMoL", input_size=S, hidden_size=HID, latent_size=LAT, residual_posterior=True).to(DEV)


@functools.lru_cache(maxsize=None)
def srnn_model(S):
    from blvm.models import SRNNAudio

    torch.manual_seed(60 + S)
    return SRNNAudio(likelihood="DMoL", input_size=S, hidden_size=HID, latent_size=LAT, residual_posterior=True, smoothing=True).to(DEV)


def vrnn_step_by_step(m, x0, h0, eps, uniforms, use_mode):
    """The loop of `VRNN.generate(fused=False)` with the state kept: -> (x [B,T,S], h_n [B,R])."""
    v = m.vrnn
    S, enc_lin, dec_lin, lik = v._plan()
    n = x0.size(0)
    x, h, xs = x0, v.vrnn_cell.get_initial_state(n, x0.device) if h0 is None else h0, []
    for t in range(eps.size(0)):
        enc = ops.mlp(x.reshape(n, S).to(torch.float32).contiguous(), enc_lin, ops.ACT_LEAKY, ops.LEAKY_SLOPE)
        h, out = v.vrnn_cell.generate(enc, h.contiguous(), use_mode=False, eps=eps[t])
        dec = ops.mlp(torch.cat([out.phi_z, h], -1).contiguous(), dec_lin, ops.ACT_LEAKY, ops.LEAKY_SLOPE)
        parameters = lik(dec.view(n, S, lik.out_features))
        x = lik.mode(parameters) if use_mode else lik.sample(parameters, uniforms=(uniforms[0][t], uniforms[1][t]))
        xs.append(x.reshape(n, S))
    return torch.stack(xs, 1), h


def vrnn_one_launch(m, x0, h0, eps, u, v, use_mode, **kw):
    vr = m.vrnn
    S, enc_lin, dec_lin, lik = vr._plan()
    c = vr.vrnn_cell
    slope = next(l.negative_slope for l in vr.encoder if isinstance(l, torch.nn.LeakyReLU))
    return ops.vrnn_decode(enc_lin, c.kernel_params(), dec_lin, lik.params, x0, h0, eps, None if use_mode else u, None if use_mode else v, S,
                           c.h_dim, c.z_dim, c.r_dim, lik.num_mix, c.prior[6].epsilon, slope, lik.log_epsilon, whole_chip=True, **kw)  # fmt: skip


@gpu
@pytest.mark.parametrize("S,B,T_,use_mode", SHAPES, ids=SHAPE_IDS)
def test_vrnn_one_launch_matches_step_by_step(S, B, T_, use_mode):
    m = vrnn_model(S)
    eps, u, v, x0 = draws(S, B, T_, 700 + 10 * S + B)
    h0 = 0.5 * torch.randn(B, m.vrnn.vrnn_cell.r_dim, generator=torch.Generator().manual_seed(B)).to(DEV)
    (a, a_sl), _ = m.generate(n_samples=B, max_timesteps=T_, x=x0.view(B, S, 1), h0=h0, eps=eps, uniforms=(u, v), use_mode=use_mode, fused=False)
    (b, b_sl), _ = m.generate(n_samples=B, max_timesteps=T_, x=x0.view(B, S, 1), h0=h0, eps=eps, uniforms=(u, v), use_mode=use_mode, fused=True)
    assert tuple(a.shape) == tuple(b.shape) == (B, T_ + 1, S) and torch.equal(a_sl, b_sl)
    assert bool(torch.isfinite(b).all()) and float(b.abs().max()) <= 1.0
    again = m.generate(n_samples=B, max_timesteps=T_, x=x0.view(B, S, 1), h0=h0, eps=eps, uniforms=(u, v), use_mode=use_mode, fused=False)[0][0]
    assert torch.equal(a, again)  # the step-by-step path against itself
    off = share(a, b)
    print(f"VRNN S={S} B={B} mode={use_mode}: share of |diff| > 2e-4 {off:.4f}, max |diff| {float((a - b).abs().max()):.2e}")
    assert off < 0.02, off
    # the returned state: the op itself against the model's loop restated with the state kept
    xs, hs = vrnn_step_by_step(m, x0, h0, eps, (u, v), use_mode)
    assert torch.equal(xs, a[:, 1:])
    xo, ho = vrnn_one_launch(m, x0, h0, eps, u, v, use_mode)
    assert torch.equal(xo, b[:, 1:]) and tuple(ho.shape) == tuple(hs.shape)
    if off == 0.0:
        e = rel_l2(ho, hs)
        print(f"    rel-L2 of h_n {e:.2e}")
        assert e <= S_TOL, e
    _hip.check_async("VRNN.generate")


@gpu
@pytest.mark.parametrize("S,B,T_,use_mode", SHAPES, ids=SHAPE_IDS)
def test_srnn_one_launch_matches_step_by_step(S, B, T_, use_mode):
    m = srnn_model(S)
    eps, u, v, x0 = draws(S, B, T_, 800 + 10 * S + B)
    R = m.srnn.r_dim
    g = torch.Generator().manual_seed(B + 1)
    d0, z0 = (0.5 * torch.randn(B, R, generator=g)).to(DEV), (0.5 * torch.randn(B, LAT, generator=g)).to(DEV)
    uni = [(u[t], v[t].unsqueeze(-1)) for t in range(T_)]
    kw = dict(x=x0.view(B, 1, S), d_0=d0, z_0=z0, n_samples=B, max_timesteps=T_, eps=eps, uniforms=uni, use_mode=use_mode)
    (a, a_sl), oa = m.srnn.generate(fused=False, **kw)
    (b, b_sl), ob = m.srnn.generate(fused=True, **kw)
    assert tuple(a.shape) == tuple(b.shape) == (B, T_, S, 1) and torch.equal(a_sl, b_sl)
    assert bool(torch.isfinite(b).all()) and float(b.abs().max()) <= 1.0
    assert torch.equal(a, m.srnn.generate(fused=False, **kw)[0][0])  # the step-by-step path against itself
    off, off_h = share(a, b), share(oa.h_p, ob.h_p, 1e-3)
    print(f"SRNN S={S} B={B} mode={use_mode}: share of |diff| > 2e-4 {off:.4f}, max |diff| {float((a - b).abs().max()):.2e}; h_p share > 1e-3 {off_h:.4f}")
    assert off < 0.02, off
    assert tuple(oa.h_p.shape) == tuple(ob.h_p.shape) == (B, R + LAT) and off_h < 0.02, off_h
    if off == 0.0:
        e = rel_l2(ob.h_p[:, :R], oa.h_p[:, :R])
        print(f"    rel-L2 of d_n {e:.2e}")
        assert e <= S_TOL, e
    _hip.check_async("SRNN.generate")


# ---- 3. LSTM against the float64 restatement --------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def lstm_on_device(name):
    m, x0, s0, uni, *_ = reference(name)
    to = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    return copy.deepcopy(m).to(DEV), to(x0), None if s0 is None else (to(s0[0]), to(s0[1])), (to(uni[0]), to(uni[1]))


@functools.lru_cache(maxsize=None)
def lstm_generated(name, fused):
    case = CASES[name]
    m, x0, s0, uni = lstm_on_device(name)
    (x, x_sl), out = m.generate(n_samples=case.B, max_timesteps=case.T, use_mode=case.mode, x=x0, h0=s0, uniforms=None if case.mode else uni,
                                fused=fused)  # fmt: skip
    torch.cuda.synchronize()
    _hip.check_async("LSTMAudio.generate")
    return x, x_sl, out.s_n


@gpu
@pytest.mark.parametrize("fused", [True, False], ids=["one-launch", "step-by-step"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_lstm_matches_float64(name, fused):
    case = CASES[name]
    *_, x64, (h64, c64), gap = reference(name)
    assert gap >= MIN_GAP
    x, x_sl, (h_n, c_n) = lstm_generated(name, fused)
    assert tuple(x.shape) == (case.B, case.T, case.S, 1) and x_sl.tolist() == [case.T] * case.B
    assert tuple(h_n.shape) == tuple(c_n.shape) == (case.L, case.B, case.H)
    dx = float((x[..., 0].double().cpu() - x64).abs().max())
    eh, ec = rel_l2(h_n, h64), rel_l2(c_n, c64)
    print(f"LSTM case {name} fused={fused}: max |x - x64| {dx:.2e}, rel-L2 h_n {eh:.2e}, c_n {ec:.2e}")
    assert dx <= X_TOL and eh <= S_TOL and ec <= S_TOL, (dx, eh, ec)
    d = float((lstm_generated(name, False)[0] - lstm_generated(name, True)[0]).abs().max())
    print(f"    max |step by step - one launch| {d:.2e}")
    assert d <= X_TOL


# ---- 4. the default takes the one-launch path -------------------------------------------------------------------------------------


def counting(monkeypatch, op):
    """-> list that receives one entry per call of `ops.<op>` (the models call it through the module)."""
    seen, real = [], getattr(ops, op)

    def wrapped(*a, **k):
        out = real(*a, **k)
        seen.append(out)
        return out

    monkeypatch.setattr(ops, op, wrapped)
    return seen


@gpu
def test_default_takes_the_one_launch_path_at_stack_1(monkeypatch):
    S, B, T_ = 1, 5, 5
    eps, u, v, x0 = draws(S, B, T_, 31)
    seen = counting(monkeypatch, "vrnn_decode")
    m = vrnn_model(S)
    (x, _), _ = m.generate(n_samples=B, max_timesteps=T_, x=x0.view(B, S, 1), eps=eps, uniforms=(u, v))
    assert len(seen) == 1
    assert torch.equal(x, m.generate(n_samples=B, max_timesteps=T_, x=x0.view(B, S, 1), eps=eps, uniforms=(u, v), fused=True)[0][0])
    seen = counting(monkeypatch, "srnn_generate")
    m = srnn_model(S)
    kw = dict(x=x0.view(B, 1, S), n_samples=B, max_timesteps=T_, eps=eps, uniforms=[(u[t], v[t].unsqueeze(-1)) for t in range(T_)])
    (x, _), _ = m.generate(**kw)
    assert len(seen) == 1
    assert torch.equal(x, m.srnn.generate(fused=True, **kw)[0][0])
    seen = counting(monkeypatch, "lstm_generate")
    case = CASES["s1b5"]
    m, lx0, s0, uni = lstm_on_device("s1b5")
    (x, _), out = m.generate(n_samples=case.B, max_timesteps=case.T, x=lx0, h0=s0, uniforms=uni)
    assert len(seen) == 1
    ref = lstm_generated("s1b5", True)
    assert torch.equal(x, ref[0]) and torch.equal(out.s_n[0], ref[2][0]) and torch.equal(out.s_n[1], ref[2][1])
    _hip.check_async("generate")


# ---- 5. / 6. chunked equals unchunked; multiples of 16 unchanged ------------------------------------------------------------------


def launches(monkeypatch):
    """-> list of the names of the library calls `ops` checks."""
    seen, real = [], ops.check

    def wrapped(code, name, *a, **k):
        seen.append(name)
        return real(code, name, *a, **k)

    monkeypatch.setattr(ops, "check", wrapped)
    return seen


def lstm_args(S, B, T_, L, seed):
    from blvm.models import LSTMAudio

    torch.manual_seed(seed)
    m = LSTMAudio(stack_size=S, hidden_size=HID, num_layers=L, num_mix=10).to(DEV)
    _, u, v, x0 = draws(S, B, T_, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    h0, c0 = (0.3 * torch.randn(L, B, HID, generator=g)).to(DEV), (0.3 * torch.randn(L, B, HID, generator=g)).to(DEV)
    emb = [l for l in m.embedding if isinstance(l, torch.nn.Linear)]
    dec = [l for l in m.decoder if isinstance(l, torch.nn.Linear)]
    return (emb, m.lstm, dec, m.likelihood.params, x0, h0, c0, u, v, S, HID, 10, m.likelihood.log_epsilon), m


@gpu
@pytest.mark.parametrize("S", [1, 16])
def test_chunked_roll_out_equals_the_single_launch(S, monkeypatch):
    """S = 1, B = 17, T = 7 with a bound that holds 3 steps: launches of 3, 3 and 1 steps give the single launch's samples and states
    bit for bit; S = 16: the same with nothing padded."""
    B, T_ = 17, 7
    lib = ops.load()
    seen = launches(monkeypatch)
    # VRNN
    m = vrnn_model(S)
    c = m.vrnn.vrnn_cell
    eps, u, v, x0 = draws(S, B, T_, 900 + S)
    h0 = 0.5 * torch.randn(B, c.r_dim, generator=torch.Generator().manual_seed(5)).to(DEV)
    bound = lib.blvm_vrnn_generate_scratch_floats(3, B, S, c.h_dim, c.z_dim, c.r_dim)
    assert bound < lib.blvm_vrnn_generate_scratch_floats(4, B, S, c.h_dim, c.z_dim, c.r_dim)
    x1, h1 = vrnn_one_launch(m, x0, h0, eps, u, v, False)
    assert seen.count("blvm_vrnn_generate") == 1
    x3, h3 = vrnn_one_launch(m, x0, h0, eps, u, v, False, max_scratch_floats=bound)
    assert seen.count("blvm_vrnn_generate") == 1 + 3
    assert torch.equal(x1, x3) and torch.equal(h1, h3) and bool(torch.isfinite(x1).all())
    # SRNN
    m = srnn_model(S).srnn
    Sx, enc_lin, dec_lin, lik = m._plan()
    H, Z, R = m.h_dim, m.z_dim, m.r_dim
    g = torch.Generator().manual_seed(6)
    d0, z0 = (0.5 * torch.randn(B, R, generator=g)).to(DEV), (0.5 * torch.randn(B, Z, generator=g)).to(DEV)
    slope = next(l.negative_slope for l in m.encoder if isinstance(l, torch.nn.LeakyReLU))
    args = (enc_lin, m.d_forward_recurrent, m._chain_params(), dec_lin, lik.params, x0, d0, z0, eps, u, v, S, H, Z, R, lik.num_mix, m.prior[6].epsilon,
            slope, lik.log_epsilon)  # fmt: skip
    bound = lib.blvm_srnn_generate_scratch_floats(3, B, S, H, Z, R)
    assert Sx == S and bound < lib.blvm_srnn_generate_scratch_floats(4, B, S, H, Z, R)
    x1, d1, z1 = ops.srnn_generate(*args)
    assert seen.count("blvm_srnn_generate") == 1
    x3, d3, z3 = ops.srnn_generate(*args, max_scratch_floats=bound)
    assert seen.count("blvm_srnn_generate") == 1 + 3
    assert torch.equal(x1, x3) and torch.equal(d1, d3) and torch.equal(z1, z3) and bool(torch.isfinite(x1).all())
    # LSTM, two layers
    args, _ = lstm_args(S, B, T_, 2, 910 + S)
    bound = lib.blvm_lstm_generate_scratch_floats(3, B, S, HID, 2)
    assert bound < lib.blvm_lstm_generate_scratch_floats(4, B, S, HID, 2)
    x1, h1, c1 = ops.lstm_generate(*args)
    assert seen.count("blvm_lstm_generate_any_stack") == 1
    x3, h3, c3 = ops.lstm_generate(*args, max_scratch_floats=bound)
    assert seen.count("blvm_lstm_generate_any_stack") == 1 + 3
    assert torch.equal(x1, x3) and torch.equal(h1, h3) and torch.equal(c1, c3) and bool(torch.isfinite(x1).all())
    with pytest.raises(ValueError):  # not even one step fits
        ops.lstm_generate(*args, max_scratch_floats=lib.blvm_lstm_generate_scratch_floats(1, B, S, HID, 2) - 1)
    torch.cuda.synchronize()
    _hip.check_async("chunked generate")


@gpu
def test_ops_still_refuse_other_widths_and_heads():
    """Any S, but H a multiple of 16 and 10 components: the library refuses the rest before it launches (S = 24 was refused before)."""
    for H, K in ((40, 10), (32, 5)):
        from blvm.models import LSTMAudio

        torch.manual_seed(3)
        m = LSTMAudio(stack_size=24, hidden_size=H, num_layers=1, num_mix=K).to(DEV)
        with pytest.raises(_hip.BlvmHipError):
            m.generate(n_samples=3, max_timesteps=2, fused=True)
    (x, _), _ = LSTMAudio(stack_size=24, hidden_size=32, num_layers=1, num_mix=10).to(DEV).generate(n_samples=3, max_timesteps=2, fused=True)
    assert tuple(x.shape) == (3, 2, 24, 1) and bool(torch.isfinite(x).all())
    _hip.check_async("LSTMAudio.generate")


@gpu
def test_scratch_sizes_at_multiples_of_16_are_the_unpadded_layouts():
    """S = 16: the scratch sizes are the closed forms of the layouts in vrnn_decode.hip, srnn_decode.hip and lstm_decode.h (every piece
    is a multiple of 4 floats at these shapes, so the arena's rounding adds nothing); at S = 5 they are those of the padded widths."""
    lib = ops.load()
    H, Z, R, L, F = HID, LAT, 2 * HID, 2, 30
    for S, B, T_ in ((16, 17, 7), (16, 5, 3), (32, 128, 2), (5, 17, 4), (1, 1, 1)):
        Sp = -(-S // 16) * 16
        Np, pad = (S * F, 0) if Sp == S else (-(-S * F // 16) * 16, None)
        if pad is None:  # the staged zero-padded copies: first layer's weight, last layer's weight and bias
            pad = H * Sp + Np * H + Np
        rows = -(-B // 16) * 16
        m = T_ * rows
        vr = (H * Sp + 2 * H * H) + (H * R + 2 * H * H) + 2 * Z * H + (H * Z + 3 * H * H) + 3 * R * 2 * H + 3 * R * R + (H * (H + R) + H * H + Np * H) + pad
        vr += (m + rows) * Sp + 2 * m * H + m * 2 * H + (m + rows) * R + (T_ + 1) * B * R + 3 * m * H + T_ * B * 3 * R + m * Z + 3 * m * H + m * (H + R)
        vr += 2 * m * H + T_ * B * Np + B * Z + B * R
        assert lib.blvm_vrnn_generate_scratch_floats(T_, B, S, H, Z, R) == vr, (S, B, T_)
        sr = (H * Sp + 2 * H * H) + 3 * R * H + 3 * R * R + (H * (R + Z) + 2 * H * H) + 2 * Z * H + (H * (Z + R) + H * H + Np * H) + pad
        sr += (m + rows) * Sp + 3 * m * H + (m + 2 * rows) * (R + Z) + (T_ + 1) * B * R + T_ * B * 3 * R + 3 * m * H + m * (Z + R) + 2 * m * H
        sr += T_ * B * Np + T_ * B * Z + B * Z + B * R
        assert lib.blvm_srnn_generate_scratch_floats(T_, B, S, H, Z, R) == sr, (S, B, T_)
        ls = (H * Sp + 2 * H * H) + L * 8 * H * H + (2 * H * H + Np * H) + pad
        ls += (m + rows) * Sp + 3 * m * H + L * ((m + rows) * H + m * H + T_ * B * 4 * H) + 2 * m * H + T_ * B * Np + L * (T_ * B * H + (T_ + 1) * B * H)
        assert lib.blvm_lstm_generate_scratch_floats(T_, B, S, H, L) == ls, (S, B, T_)
