"""`LSTMAudio.generate` on the device: the one-launch roll-out (`blvm_lstm_generate`, csrc/lstm_decode.hip) and the step-by-step path
against the float64 restatement of tests/test_lstm_generate_cpu.py, which also defines the cases, their seeds and the comparison
rule (no near ties: every case's smallest perturbed-logit gap is >= 1e-3, asserted there on the CPU).

Bars: every sample within 1e-4 of the restatement (the bar of tests/test_wavenet_prompt.py for the same kind of free-running
comparison), `s_n` at rel-L2 2e-5 per tensor (the project's LSTM bar), the two paths within 1e-4 of each other.

Measured on an MI355X (fp32 operands), max |x - x64| / rel-L2 of h_n / of c_n:
  one launch   a 1.6e-07 / 9.1e-08 / 8.1e-08   b 3.0e-07 / 8.1e-08 / 6.4e-08   c 4.5e-07 / 8.6e-08 / 6.5e-08
               d 3.4e-07 / 8.7e-08 / 6.4e-08   e 3.9e-07 / 9.2e-08 / 7.4e-08   f 2.0e-08 / 8.7e-08 / 5.8e-08
  step by step a 5.7e-08 / 8.0e-08 / 6.9e-08   b 1.0e-07 / 8.3e-08 / 6.8e-08   c 1.5e-07 / 8.5e-08 / 6.3e-08
               d 1.3e-07 / 8.8e-08 / 6.6e-08   e 2.1e-07 / 1.0e-07 / 8.7e-08   f 1.6e-08 / 8.0e-08 / 6.9e-08
  max |step by step - one launch|: a 1.2e-07, b 2.7e-07, c 5.4e-07, d 3.0e-07, e 3.6e-07, f 3.0e-08
  other structures (step by step): H = 40 1.6e-07 / 8.9e-08 / 6.7e-08, num_mix = 5 1.8e-07 / 9.5e-08 / 7.3e-08, H = 40 with two
  layers 2.5e-07 / 9.9e-08 / 7.5e-08;  teacher forcing: h_n 6.0e-08, c_n 5.7e-08, max |resampled - generated| 4.5e-07
"""
import copy
import ctypes
import functools

import pytest
import torch

from blvm import _hip, ops

from test_lstm_generate_cpu import CASES, MIN_GAP, NUM_MIX, lstm_audio_generate_f64, reference

gpu = pytest.mark.gpu
DEV = "cuda:0"
X_TOL, S_TOL = 1e-4, 2e-5


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@functools.lru_cache(maxsize=None)
def on_device(name):
    """(model on the device, x0, s0, uniforms on the device) of a case."""
    m, x0, s0, uni, *_ = reference(name)
    to = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    return copy.deepcopy(m).to(DEV), to(x0), None if s0 is None else (to(s0[0]), to(s0[1])), (to(uni[0]), to(uni[1]))


@functools.lru_cache(maxsize=None)
def generated(name, fused):
    """(x [B,T,S,1], x_sl, (h_n, c_n)) of a case on one path — computed once."""
    case = CASES[name]
    m, x0, s0, uni = on_device(name)
    (x, x_sl), out = m.generate(n_samples=case.B, max_timesteps=case.T, use_mode=case.mode, x=x0, h0=s0, uniforms=None if case.mode else uni,
                                fused=fused)  # fmt: skip
    torch.cuda.synchronize()
    _hip.check_async("LSTMAudio.generate")
    return x, x_sl, out.s_n


def check_against_f64(name, fused):
    case = CASES[name]
    *_, x64, (h64, c64), gap = reference(name)
    assert gap >= MIN_GAP
    x, x_sl, (h_n, c_n) = generated(name, fused)
    assert tuple(x.shape) == (case.B, case.T, case.S, 1) and x_sl.tolist() == [case.T] * case.B
    assert tuple(h_n.shape) == tuple(c_n.shape) == (case.L, case.B, case.H)
    dx = float((x[..., 0].double().cpu() - x64).abs().max())
    eh, ec = rel_l2(h_n, h64), rel_l2(c_n, c64)
    print(f"case {name} fused={fused}: max |x - x64| {dx:.2e}, rel-L2 h_n {eh:.2e}, c_n {ec:.2e}")
    assert dx <= X_TOL and eh <= S_TOL and ec <= S_TOL, (dx, eh, ec)


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_one_launch_matches_float64(name):
    check_against_f64(name, True)


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_step_by_step_matches_float64_and_the_one_launch_path(name):
    check_against_f64(name, False)
    d = float((generated(name, False)[0] - generated(name, True)[0]).abs().max())
    print(f"case {name}: max |step by step - one launch| {d:.2e}")
    assert d <= X_TOL


def counting(monkeypatch):
    """-> list that receives one entry per `ops.lstm_generate` call (the model calls it as `ops.lstm_generate`)."""
    seen, real = [], ops.lstm_generate

    def wrapped(*a, **k):
        out = real(*a, **k)
        seen.append(out)
        return out

    monkeypatch.setattr(ops, "lstm_generate", wrapped)
    return seen


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_default_takes_the_one_launch_path(name, monkeypatch):
    case = CASES[name]
    m, x0, s0, uni = on_device(name)
    seen = counting(monkeypatch)
    (x, _), out = m.generate(n_samples=case.B, max_timesteps=case.T, use_mode=case.mode, x=x0, h0=s0, uniforms=None if case.mode else uni)
    assert len(seen) == 1
    ref = generated(name, True)
    assert torch.equal(x, ref[0]) and torch.equal(out.s_n[0], ref[2][0]) and torch.equal(out.s_n[1], ref[2][1])


@gpu
@pytest.mark.parametrize("kw", [dict(hidden_size=40), dict(num_mix=5), dict(hidden_size=40, num_layers=2)], ids=["H40", "K5", "H40x2"])
def test_other_structures_run_step_by_step(kw, monkeypatch):
    """A hidden size that is no multiple of 16 (the step-by-step path pads it) and a head of 5 components: the default takes the
    step-by-step path, the samples are finite, inside [-1, 1] and the restatement's; an explicit fused=True raises."""
    from blvm.models import LSTMAudio

    n, T, S = 3, 4, 16
    torch.manual_seed(11)
    m = LSTMAudio(**{**dict(stack_size=S, hidden_size=48, num_layers=1, num_mix=NUM_MIX), **kw})
    H, L, K = m.hidden_size, m.num_layers, m.num_mix
    g = torch.Generator().manual_seed(13)
    u = torch.empty(T, n, S, K).uniform_(1e-5, 1.0 - 1e-5, generator=g)
    v = torch.empty(T, n, S).uniform_(1e-8, 1.0 - 1e-8, generator=g)
    s0 = (0.3 * torch.randn(L, n, H, generator=g), 0.3 * torch.randn(L, n, H, generator=g))
    sd64 = {k: t.detach().double() for k, t in m.state_dict().items()}
    x64, (h64, c64), gap = lstm_audio_generate_f64(sd64, None, s0, (u, v), T, n, S, H, L, num_mix=K)
    assert gap >= MIN_GAP  # no near tie: a flipped component would show as a large difference below
    m = m.to(DEV)
    seen = counting(monkeypatch)
    (x, x_sl), out = m.generate(n_samples=n, max_timesteps=T, h0=(s0[0].to(DEV), s0[1].to(DEV)), uniforms=(u.to(DEV), v.to(DEV)))
    assert len(seen) == 0
    assert tuple(x.shape) == (n, T, S, 1) and bool(torch.isfinite(x).all()) and float(x.abs().max()) <= 1.0
    assert tuple(out.s_n[0].shape) == tuple(out.s_n[1].shape) == (L, n, H)
    dx = float((x[..., 0].double().cpu() - x64).abs().max())
    print(f"{kw}: max |x - x64| {dx:.2e}, rel-L2 h_n {rel_l2(out.s_n[0], h64):.2e}, c_n {rel_l2(out.s_n[1], c64):.2e}")
    assert dx <= X_TOL and rel_l2(out.s_n[0], h64) <= S_TOL and rel_l2(out.s_n[1], c64) <= S_TOL
    with pytest.raises(_hip.BlvmHipError):  # an explicit fused=True insists
        m.generate(n_samples=n, max_timesteps=T, fused=True)


@gpu
def test_teacher_forcing_reproduces_the_roll_out():
    """`forward` on cat[x0, generated] (zero initial state, case b's shape) ends in `generate`'s state, and its head parameters with the
    replayed draws give the generated stacks back."""
    case = CASES["b"]
    m, x0, _, (u, v) = on_device("b")
    B, T, S = case.B, case.T, case.S
    (x, _), out = m.generate(n_samples=B, max_timesteps=T, x=x0, uniforms=(u, v), fused=True)
    seq = torch.cat([x0.view(B, 1, S), x[..., 0]], 1).flatten(1)
    _, _, fwd = m(seq, torch.full((B,), seq.size(1)))
    eh, ec = rel_l2(fwd.s_n[0], out.s_n[0]), rel_l2(fwd.s_n[1], out.s_n[1])
    ub, vb = u.permute(1, 0, 2, 3).reshape(B, T * S, NUM_MIX), v.permute(1, 0, 2).reshape(B, T * S)
    again = m.likelihood.sample(fwd._parameters, uniforms=(ub, vb)).view(B, T, S)
    dx = float((again - x[..., 0]).abs().max())
    print(f"teacher forcing: rel-L2 h_n {eh:.2e}, c_n {ec:.2e}, max |resampled - generated| {dx:.2e}")
    assert eh <= S_TOL and ec <= S_TOL and dx <= X_TOL


@gpu
@pytest.mark.parametrize("name", ["b", "c"])
def test_one_launch_path_is_resumable_bit_for_bit(name):
    case = CASES[name]
    m, x0, s0, (u, v) = on_device(name)
    T1 = 3
    (xa, _), oa = m.generate(n_samples=case.B, max_timesteps=T1, x=x0, h0=s0, uniforms=(u[:T1], v[:T1]), fused=True)
    (xb, _), ob = m.generate(n_samples=case.B, max_timesteps=case.T - T1, x=xa[:, -1, :, 0], h0=oa.s_n, uniforms=(u[T1:], v[T1:]), fused=True)
    x, _, s_n = generated(name, True)
    assert torch.equal(torch.cat([xa, xb], 1), x)
    assert torch.equal(ob.s_n[0], s_n[0]) and torch.equal(ob.s_n[1], s_n[1])


@gpu
def test_device_rng_draws():
    m = on_device("b")[0]
    (a, x_sl), _ = m.generate(n_samples=4, max_timesteps=6)
    (b, _), _ = m.generate(n_samples=4, max_timesteps=6)
    assert tuple(a.shape) == (4, 6, 16, 1) and x_sl.tolist() == [6] * 4
    for x in (a, b):
        assert bool(torch.isfinite(x).all()) and float(x.abs().max()) <= 1.0
    assert not torch.equal(a, b)


def call_c_abi(name, fill, B=None, S=None, num_mix=NUM_MIX, x_fill=None):
    """`blvm_lstm_generate` called directly on a case's tensors with scratch and outputs prefilled with `fill`.  -> (rc, x, h, c)."""
    case = CASES[name]
    m, x0, s0, (u, v) = on_device(name)
    B, S = case.B if B is None else B, case.S if S is None else S
    T, H, L = case.T, case.H, case.L
    lib = ops.load()
    emb = [l for l in m.embedding if isinstance(l, torch.nn.Linear)]
    dec = [l for l in m.decoder if isinstance(l, torch.nn.Linear)]
    w, keep = ops.lstm_decode_weights(emb, m.lstm, dec, m.likelihood.params)
    f32 = dict(device=DEV, dtype=torch.float32)
    n = max(int(lib.blvm_lstm_generate_scratch_floats(T, B, S, H, L)), 16)
    scratch = torch.full((n,), fill, **f32)
    x = torch.full((B, T, S), fill if x_fill is None else x_fill, **f32)
    h, c = torch.full((L, B, H), fill, **f32), torch.full((L, B, H), fill, **f32)
    p = ops.ptr
    rc = lib.blvm_lstm_generate(ctypes.byref(w), p(x0), p(None if s0 is None else s0[0]), p(None if s0 is None else s0[1]), p(u), p(v), T, B, S, H, L,
                                num_mix, m.likelihood.log_epsilon, p(x), p(h), p(c), p(scratch), ops.stream_ptr())  # fmt: skip
    torch.cuda.synchronize()
    del keep
    return rc, x, h, c


@gpu
@pytest.mark.parametrize("name", ["c", "e"])
def test_c_abi_results_do_not_depend_on_prior_buffer_contents(name):
    rc0, x0_, h0_, c0_ = call_c_abi(name, float("nan"))
    rc1, x1_, h1_, c1_ = call_c_abi(name, 0.0)
    assert rc0 == 0 and rc1 == 0
    _hip.check_async("blvm_lstm_generate")
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    assert torch.equal(bits(x0_), bits(x1_)) and torch.equal(bits(h0_), bits(h1_)) and torch.equal(bits(c0_), bits(c1_))
    assert torch.equal(x0_, generated(name, True)[0][..., 0])


@gpu
@pytest.mark.parametrize("kw", [dict(B=129), dict(S=24), dict(num_mix=11)], ids=["B129", "S24", "K11"])
def test_c_abi_refuses_bad_arguments_before_touching_anything(kw):
    rc, x, _, _ = call_c_abi("b", 0.0, x_fill=7.0, **kw)
    assert rc != 0
    assert bool((x == 7.0).all())
