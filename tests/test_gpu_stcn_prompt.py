"""`STCN.generate` from a prompt and in chunks, on the device: the resume entry of the one-launch kernel (`blvm_stcn_generate_resume`,
csrc/stcn_decode.hip), the priming of its rings from a state's windows, and the step-by-step path continuing from the same state —
against the float64 restatement of tests/test_stcn_prompt_cpu.py, which also defines the prompt cases, their seeds and the
comparison rule (no near ties, asserted there on the CPU).

Bars, those of tests/test_gpu_stcn_generate.py: every sample within X_TOL = 1e-4 of the restatement, z / prior_mus / prior_sds (and
the prompt's z) at rel-L2 S_TOL = 2e-5 per level, the two paths within 1e-4 of each other.  Chunked generation through the one-launch
kernel is compared bit for bit: a resumed call does the arithmetic of the long call on the same ring contents.

Measured on an MI355X (fp32 operands).  Prompt cases, posterior latents unless marked, max |x - x64| / largest rel-L2 over the levels
of z / of prior_mus / of prior_sds / of prompt_z:
  one launch   b P'=1 6.0e-08 / 1.0e-07 / 5.2e-08 / 9.9e-08 / 8.2e-08    b P'=3 5.3e-08 / 9.8e-08 / 5.2e-08 / 9.7e-08 / 8.0e-08
               b P'=3 prior 4.7e-08 / 1.0e-07 / 5.4e-08 / 9.7e-08 / 1.0e-07   b P'=30 5.9e-08 / 9.9e-08 / 4.9e-08 / 9.9e-08 / 7.8e-08
               c P'=5 1.5e-07 / 1.0e-07 / 6.8e-08 / 1.0e-07 / 8.0e-08    c P'=5 prior 2.1e-07 / 1.0e-07 / 7.2e-08 / 1.0e-07 / 1.0e-07
               d P'=5 2.6e-08 / 1.1e-07 / 7.5e-08 / 1.0e-07 / 8.3e-08    e P'=2 2.0e-07 / 1.1e-07 / 2.8e-07 / 9.9e-08 / 8.6e-08
               f P'=5 9.8e-08 / 1.1e-07 / 6.7e-08 / 1.0e-07 / 8.2e-08    g P'=5 1.1e-07 / 1.0e-07 / 7.6e-08 / 1.0e-07 / 8.0e-08
  step by step b P'=1 5.3e-08 / 1.0e-07 / 4.8e-08 / 9.8e-08 / 8.2e-08    b P'=3 5.3e-08 / 9.9e-08 / 5.1e-08 / 9.7e-08 / 8.0e-08
               b P'=3 prior 4.7e-08 / 1.0e-07 / 4.7e-08 / 9.8e-08 / 1.0e-07   b P'=30 7.4e-08 / 1.0e-07 / 4.7e-08 / 9.9e-08 / 7.8e-08
               c P'=5 1.5e-07 / 1.0e-07 / 7.3e-08 / 1.0e-07 / 8.0e-08    c P'=5 prior 2.1e-07 / 1.0e-07 / 7.7e-08 / 1.0e-07 / 1.0e-07
               d P'=5 2.8e-08 / 1.1e-07 / 7.0e-08 / 1.0e-07 / 8.3e-08    e P'=2 2.0e-07 / 1.1e-07 / 2.8e-07 / 1.0e-07 / 8.6e-08
               f P'=5 9.8e-08 / 1.0e-07 / 6.1e-08 / 1.0e-07 / 8.2e-08    g P'=5 1.1e-07 / 1.0e-07 / 7.0e-08 / 1.0e-07 / 8.0e-08
  max |step by step - one launch| over the prompt cases: 1.2e-07 (e P'=2)
Chunks against the long call: bit for bit on the one-launch path (asserted) and, as measured, on the step-by-step path too (every
case: all differences 0, bit-exact).  A free run's first steps as a prior-mode prompt, continuation against the run's tail, max |dx| /
rel-L2 z / prior_mus / prior_sds / prompt_z: b T1=5 one launch 3.0e-08 / 2.1e-08 / 3.5e-08 / 1.6e-08 / 4.2e-08, step by step
3.0e-08 / 4.0e-08 / 5.8e-08 / 2.6e-08 / 4.2e-08; c T1=4 one launch 1.8e-07 / 2.9e-08 / 4.5e-08 / 1.8e-08 / 5.2e-08, step by step
8.9e-08 / 4.4e-08 / 7.8e-08 / 2.8e-08 / 5.2e-08.  A step-by-step state (b, 5 steps) primed and continued in one launch: 3.0e-08 from
the long one-launch call.
"""
import ctypes
import functools
import math

import pytest
import torch

from blvm import _hip, ops

from test_gpu_stcn_generate import DEV, S_TOL, X_TOL, generated, on_device, rel_l2
from test_stcn_generate_cpu import CASES, MIN_GAP, NUM_MIX
from test_stcn_prompt_cpu import PROMPT_RUNS, prompt_reference

gpu = pytest.mark.gpu


def gen(m, case, T, eps, uni, **kw):
    """One `generate` call of T steps; eps / uniforms are the call's own (indexed from 0).  -> (x [B,T*S,1], namespace)."""
    (x, x_sl), out = m.generate(n_samples=case.B, max_timesteps=T * case.S, use_mode_observations=case.mode, eps=eps,
                                uniforms=None if case.mode else uni, **kw)  # fmt: skip
    torch.cuda.synchronize()
    _hip.check_async("STCN.generate")
    assert tuple(x.shape) == (case.B, T * case.S, 1) and x_sl.tolist() == [T * case.S] * case.B
    return x, out


def cut(eps, uni, lo, hi):
    return [e[lo:hi] for e in eps], (uni[0][lo:hi], uni[1][lo:hi])


def in_chunks(name, chunks, fused):
    """The case's draws spent in `chunks` calls chained through return_state / state.
    -> (x, z, prior_mus, prior_sds concatenated over the calls, the last state, the states' n_steps)."""
    case = CASES[name]
    m, eps, uni = on_device(name)
    xs, outs, steps, lo, state = [], [], [], 0, None
    for i, T in enumerate(chunks):
        kw = dict(return_state=True, fused=fused)
        if state is not None:
            kw["state"] = state
        x, out = gen(m, case, T, *cut(eps, uni, lo, lo + T), **kw)
        state, lo = out.state, lo + T
        xs.append(x)
        outs.append(out)
        steps.append(state.n_steps)
    cat = lambda f: [torch.cat([f(o)[l] for o in outs], 1) for l in range(len(case.latents))]  # noqa: E731
    return torch.cat(xs, 1), cat(lambda o: o.z), cat(lambda o: o.prior_mus), cat(lambda o: o.prior_sds), state, steps


def all_equal(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


CHUNKS = [("b", (5, 7)), ("b", (1, 4, 7)), ("c", (4, 5)), ("d", (2, 4)), ("f", (3, 3)), ("g", (3, 3))]
CHUNK_IDS = [f"{n}-{'+'.join(map(str, c))}" for n, c in CHUNKS]


@gpu
@pytest.mark.parametrize("name,chunks", CHUNKS, ids=CHUNK_IDS)
def test_chunks_are_the_long_call_bit_for_bit_in_one_launch(name, chunks):
    x, _, out = generated(name, True)
    cx, cz, cmu, csd, state, steps = in_chunks(name, chunks, True)
    assert steps == [sum(chunks[: i + 1]) for i in range(len(chunks))]
    assert state.scratch is not None
    assert torch.equal(cx, x)
    assert all_equal(cz, out.z) and all_equal(cmu, out.prior_mus) and all_equal(csd, out.prior_sds)


@gpu
@pytest.mark.parametrize("name,chunks", CHUNKS, ids=CHUNK_IDS)
def test_chunks_are_the_long_call_step_by_step(name, chunks):
    x, _, out = generated(name, False)
    cx, cz, cmu, csd, state, steps = in_chunks(name, chunks, False)
    assert steps == [sum(chunks[: i + 1]) for i in range(len(chunks))] and state.scratch is None
    dx = float((cx - x).abs().max())
    errs = [max(rel_l2(g, w) for g, w in zip(got, want)) for got, want in ((cz, out.z), (cmu, out.prior_mus), (csd, out.prior_sds))]
    exact = torch.equal(cx, x) and all_equal(cz, out.z) and all_equal(cmu, out.prior_mus) and all_equal(csd, out.prior_sds)
    print(f"case {name} chunks {chunks} step by step: max |dx| {dx:.2e}, rel-L2 z {errs[0]:.2e}, mus {errs[1]:.2e}, sds {errs[2]:.2e}, bit-exact {exact}")
    assert dx <= X_TOL and max(errs) <= S_TOL


@gpu
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", ["b", "c"])
def test_return_state_changes_nothing(name, fused):
    case = CASES[name]
    m, eps, uni = on_device(name)
    x, out = gen(m, case, case.T, eps, uni, fused=fused, return_state=True)
    rx, _, rout = generated(name, fused)
    assert torch.equal(x, rx) and all_equal(out.z, rout.z) and all_equal(out.prior_mus, rout.prior_mus) and all_equal(out.prior_sds, rout.prior_sds)
    st = out.state
    assert st.n_steps == case.T and tuple(st.x_window.shape) == (m.receptive_field, case.B, case.S)
    assert (st.scratch is not None) == fused
    tail = min(case.T, m.receptive_field)
    assert torch.equal(st.x_window[-tail:], rx[..., 0].view(case.B, case.T, case.S).transpose(0, 1)[-tail:])
    assert not bool(st.x_window[: m.receptive_field - tail].any())


def prompt_kw(r, mode):
    return dict(x=r["prompt"].to(DEV), prompt_eps=[e.to(DEV) for e in r["prompt_eps"]], prompt_latents=mode)


@functools.lru_cache(maxsize=None)
def prompted(name, Pp, mode, fused):
    """(x, namespace) of a prompt case on one path — computed once."""
    case = CASES[name]
    r = prompt_reference(name, Pp, mode)
    m = on_device(name)[0]
    eps, uni = [e.to(DEV) for e in r["eps"]], tuple(t.to(DEV) for t in r["uniforms"])
    return gen(m, case, r["T"], eps, uni, fused=fused, **prompt_kw(r, mode))


def check_prompt_against_f64(name, Pp, mode, fused):
    case = CASES[name]
    r = prompt_reference(name, Pp, mode)
    assert r["gap"] >= MIN_GAP
    x, out = prompted(name, Pp, mode, fused)
    dx = float((x[..., 0].double().cpu() - r["x"]).abs().max())
    errs = []
    for got, want in ((out.z, r["z"]), (out.prior_mus, r["mu"]), (out.prior_sds, r["sd"]), (out.prompt_z, r["prompt_z"])):
        assert len(got) == len(case.latents)
        errs.append(max(rel_l2(got[l], want[l].transpose(0, 1)) for l in range(len(case.latents))))
    assert [tuple(t.shape) for t in out.prompt_z] == [(case.B, Pp, Z) for Z in case.latents]
    print(f"case {name} P'={Pp} {mode} fused={fused}: max |x - x64| {dx:.2e}, rel-L2 z {errs[0]:.2e}, prior_mus {errs[1]:.2e}, "
          f"prior_sds {errs[2]:.2e}, prompt_z {errs[3]:.2e}")  # fmt: skip
    assert dx <= X_TOL and max(errs) <= S_TOL, (dx, errs)


@gpu
@pytest.mark.parametrize("name,Pp,mode", PROMPT_RUNS)
def test_prompt_in_one_launch_matches_float64(name, Pp, mode):
    check_prompt_against_f64(name, Pp, mode, True)


@gpu
@pytest.mark.parametrize("name,Pp,mode", PROMPT_RUNS)
def test_prompt_step_by_step_matches_float64_and_the_one_launch_path(name, Pp, mode):
    check_prompt_against_f64(name, Pp, mode, False)
    d = float((prompted(name, Pp, mode, False)[0] - prompted(name, Pp, mode, True)[0]).abs().max())
    print(f"case {name} P'={Pp} {mode}: max |step by step - one launch| {d:.2e}")
    assert d <= X_TOL


@gpu
@pytest.mark.parametrize("name,Pp", [("b", 1), ("c", 5), ("f", 5), ("g", 5)])
def test_posterior_priming_is_forward(name, Pp):
    case = CASES[name]
    r = prompt_reference(name, Pp, "posterior")
    m = on_device(name)[0]
    kw = prompt_kw(r, "posterior")
    _, _, fwd = m.forward(kw["x"], torch.full((case.B,), Pp * case.S), eps=kw["prompt_eps"])
    out = prompted(name, Pp, "posterior", True)[1]
    state, pz = m._prime(kw["x"], kw["prompt_eps"], "posterior")
    torch.cuda.synchronize()
    _hip.check_async("STCN._prime")
    for l in range(len(case.latents)):
        assert torch.equal(out.prompt_z[l], fwd.z[l]) and torch.equal(pz[l], fwd.z[l])
    zin = (torch.cat(fwd.z, -1) if case.dense else fwd.z[0]).transpose(0, 1)  # [P',B,Zin]
    n_out = case.n_layers
    want = torch.cat([torch.zeros(n_out, case.B, zin.size(-1), device=DEV), zin], 0)[-n_out:]
    assert state.n_steps == Pp and state.scratch is None and torch.equal(state.z_window, want)
    xw = torch.cat([torch.zeros(m.receptive_field, case.B, case.S, device=DEV), kw["x"].view(case.B, Pp, case.S).transpose(0, 1)], 0)
    assert torch.equal(state.x_window, xw[-m.receptive_field :])


@gpu
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name,T1", [("b", 5), ("c", 4)])
def test_prior_mode_continues_a_free_run(name, T1, fused):
    """No oracle: the first T1 steps of the free run as a prior-mode prompt under the run's own eps, then the run's remaining draws."""
    case = CASES[name]
    m, eps, uni = on_device(name)
    x, _, out = generated(name, True)
    S, T = case.S, case.T
    cx, cout = gen(m, case, T - T1, *cut(eps, uni, T1, T), fused=fused, x=x[:, : T1 * S], prompt_eps=[e[:T1] for e in eps],
                   prompt_latents="prior")  # fmt: skip
    dx = float((cx - x[:, T1 * S :]).abs().max())
    errs = [max(rel_l2(g, w[:, T1:]) for g, w in zip(got, want))
            for got, want in ((cout.z, out.z), (cout.prior_mus, out.prior_mus), (cout.prior_sds, out.prior_sds))]  # fmt: skip
    ez = max(rel_l2(g, w[:, :T1]) for g, w in zip(cout.prompt_z, out.z))
    print(f"case {name} T1={T1} fused={fused}: max |dx| {dx:.2e}, rel-L2 z {errs[0]:.2e}, mus {errs[1]:.2e}, sds {errs[2]:.2e}, prompt_z {ez:.2e}")
    assert dx <= X_TOL and max(errs) <= S_TOL and ez <= S_TOL


@gpu
@pytest.mark.parametrize("name,Pp,chunks", [("b", 3, (2, 4)), ("c", 5, (1, 5))])
def test_prompt_then_chunks_is_prompt_then_all(name, Pp, chunks):
    case = CASES[name]
    r = prompt_reference(name, Pp, "posterior")
    m = on_device(name)[0]
    eps, uni = [e.to(DEV) for e in r["eps"]], tuple(t.to(DEV) for t in r["uniforms"])
    x, out = prompted(name, Pp, "posterior", True)
    xs, outs, state, lo = [], [], None, 0
    for i, T in enumerate(chunks):
        kw = prompt_kw(r, "posterior") if i == 0 else dict(state=state)
        cx, cout = gen(m, case, T, *cut(eps, uni, lo, lo + T), fused=True, return_state=True, **kw)
        state, lo = cout.state, lo + T
        xs.append(cx)
        outs.append(cout)
        assert state.n_steps == Pp + lo and ("prompt_z" in vars(cout)) == (i == 0)
    assert torch.equal(torch.cat(xs, 1), x)
    for f in (lambda o: o.z, lambda o: o.prior_mus, lambda o: o.prior_sds):
        assert all_equal([torch.cat([f(o)[l] for o in outs], 1) for l in range(len(case.latents))], f(out))


def counting(monkeypatch, name, resumed=False):
    """-> list that receives one entry per `ops.<name>` call (the model calls it as `ops.<name>`); resumed=True: per call that
    continues from a state (the model gives `resume=` by keyword)."""
    seen, real = [], getattr(ops, name)

    def wrapped(*a, **k):
        out = real(*a, **k)
        if not resumed or k.get("resume") is not None:
            seen.append(out)
        return out

    monkeypatch.setattr(ops, name, wrapped)
    return seen


@gpu
def test_default_takes_the_resume_entry_with_a_prompt(monkeypatch):
    name, Pp = "c", 5
    case, r, m = CASES[name], prompt_reference(name, Pp, "posterior"), on_device(name)[0]
    assert m._one_launch_applies()
    seen = counting(monkeypatch, "stcn_generate", resumed=True)
    eps, uni = [e.to(DEV) for e in r["eps"]], tuple(t.to(DEV) for t in r["uniforms"])
    x, _ = gen(m, case, r["T"], eps, uni, fused=None, **prompt_kw(r, "posterior"))
    assert len(seen) == 1
    assert torch.equal(x, prompted(name, Pp, "posterior", True)[0])


@gpu
def test_a_step_by_step_state_is_primed_for_the_one_launch_kernel(monkeypatch):
    name, T1 = "b", 5
    case = CASES[name]
    m, eps, uni = on_device(name)
    _, first = gen(m, case, T1, *cut(eps, uni, 0, T1), fused=False, return_state=True)
    assert first.state.scratch is None
    seen, primed = counting(monkeypatch, "stcn_generate", resumed=True), counting(monkeypatch, "wavenet_prime_rings")
    x, out = gen(m, case, case.T - T1, *cut(eps, uni, T1, case.T), fused=True, state=first.state, return_state=True)
    assert len(seen) == 1 and len(primed) == 2  # the dilated stack's rings and the output stack's
    assert out.state.scratch is not None and out.state.n_steps == case.T
    d = float((x - generated(name, True)[0][:, T1 * case.S :]).abs().max())
    print(f"case {name}: step-by-step state continued in one launch, max |dx| to the long call {d:.2e}")
    assert d <= X_TOL


@gpu
def test_another_head_continues_a_prompt_step_by_step(monkeypatch):
    from blvm.models.stcn.stcn import STCN

    B, S, latents = 3, 8, [16, 16, 32]
    torch.manual_seed(21)
    m = STCN(likelihood="GMM", n_layers=3, latent_size=latents, res_channels=16, n_stack_frames=S).to(DEV)
    seen = counting(monkeypatch, "stcn_generate", resumed=True)
    prompt = 0.5 * torch.tanh(torch.randn(B, 4 * S, device=DEV))
    (x, x_sl), out = m.generate(n_samples=B, max_timesteps=2 * S, x=prompt, return_state=True)
    (x2, _), out2 = m.generate(n_samples=B, max_timesteps=S, state=out.state)
    torch.cuda.synchronize()
    _hip.check_async("STCN.generate")
    assert len(seen) == 0
    assert tuple(x.shape) == (B, 2 * S, 1) and tuple(x2.shape) == (B, S, 1) and bool(torch.isfinite(x).all()) and bool(torch.isfinite(x2).all())
    assert out.state.n_steps == 6 and out.state.scratch is None and not hasattr(out2, "state")
    assert [tuple(t.shape) for t in out.prompt_z] == [(B, 4, Z) for Z in latents]
    with pytest.raises(_hip.BlvmHipError):  # an explicit fused=True insists
        m.generate(n_samples=B, max_timesteps=S, x=prompt, fused=True)


# ---- the C ABI of blvm_stcn_generate_resume
def resume_abi(name, T1, fill=None, sentinel=None, t0=None, null_in=False, null_state=False, latent24=False, T=None):
    """The state after T1 steps of the case (`ops.stcn_generate` from the zero start), then `blvm_stcn_generate_resume` through ctypes for the
    remaining steps.  fill: what the outputs, the operand copies below the ring offset and the selected-skips tail hold before the
    call.  sentinel = (scratch, x_out, x_state) values planted everywhere instead (refusals).
    -> (rc, x, z, mu, sd, x_state, scratch, ring region bounds, x_in, error message)."""
    case = CASES[name]
    m, eps, (u, v) = on_device(name)
    B, S = case.B, case.S
    T2 = case.T - T1 if T is None else T
    p0, lik, blk = m.prior[0], m.likelihood_module, m.res_stack.res_blocks[0]
    f32 = dict(device=DEV, dtype=torch.float32)
    x1, _, _, _, scratch, _ = ops.stcn_generate(m._one_launch_parts(), B, T1, S, blk.inv_std, m.inv_std, p0.softplus_beta, p0.epsilon,
                                                p0.transform_mu[1].negative_slope, NUM_MIX, lik.log_epsilon, [e[:T1] for e in eps],
                                                None if case.mode else u[:T1], None if case.mode else v[:T1])  # fmt: skip
    p = ops.stcn_generate_pack(m._one_launch_parts(), S, NUM_MIX)
    lib = p.lib
    lo = int(lib.blvm_stcn_generate_ring_offset_floats(p.C, S, p.n_blocks, p.n_out, p.latent, p.order, p.n, p.dense, NUM_MIX))
    hi = lo + (sum(m.res_stack.dilations) + p.n_out) * B * p.C
    assert lo == p.packed.numel() and hi + p.n * B * p.C == scratch.numel()
    x_in = torch.cat([torch.zeros(B, 2, S, **f32), x1], 1)[:, -2:].contiguous()
    of = fill
    if sentinel is not None:
        scratch.fill_(sentinel[0])
        of = sentinel[1]
    else:
        scratch[:lo] = fill
        scratch[hi:] = fill
    Ta = max(T2, 1)  # (a call of zero steps still takes real buffers)
    x = torch.full((B, Ta, S), of, **f32)
    zs, mus, sds = ([torch.full((Ta, B, Z), of, **f32) for Z in case.latents] for _ in range(3))
    x_state = torch.full((B, 2, S), of if sentinel is None else sentinel[2], **f32)
    e2 = [e[T1 : T1 + Ta].contiguous() for e in eps]
    u2, v2 = (None, None) if case.mode else (u[T1 : T1 + Ta].contiguous(), v[T1 : T1 + Ta].contiguous())
    ptrs = lambda ts: (ctypes.c_void_p * len(ts))(*[ops.ptr(t) for t in ts])  # noqa: E731
    latent = (ctypes.c_int * p.n)(*[24 if latent24 and l == 1 else z for l, z in enumerate(case.latents)])
    rc = lib.blvm_stcn_generate_resume(ops.ptr(p.packed), p.dil, p.groups, p.n_blocks, p.n_out, latent, p.order, p.n, p.dense, B, p.C, S, NUM_MIX,
                                       T2, blk.inv_std, m.inv_std, p0.softplus_beta, p0.epsilon, p0.transform_mu[1].negative_slope,
                                       lik.log_epsilon, ptrs(e2), ops.ptr(u2), ops.ptr(v2), ops.ptr(x), ptrs(zs), ptrs(mus), ptrs(sds),
                                       ops.ptr(scratch), T1 % math.lcm(*m.res_stack.dilations) if t0 is None else t0,
                                       None if null_in else ops.ptr(x_in), None if null_state else ops.ptr(x_state), ops.stream_ptr())  # fmt: skip
    msg = lib.blvm_last_error().decode(errors="replace") if rc != 0 else ""
    torch.cuda.synchronize()
    return rc, x, zs, mus, sds, x_state, scratch, (lo, hi), x_in, msg


@gpu
@pytest.mark.parametrize("name,T1", [("c", 4), ("b", 5)])
def test_c_abi_resume_does_not_depend_on_prior_buffer_contents(name, T1):
    case = CASES[name]
    r_nan = resume_abi(name, T1, fill=float("nan"))
    r_big = resume_abi(name, T1, fill=1e30)
    assert r_nan[0] == 0 and r_big[0] == 0
    _hip.check_async("blvm_stcn_generate_resume")
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    for i in (1, 5):
        assert torch.equal(bits(r_nan[i]), bits(r_big[i]))
    for i in (2, 3, 4):
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(r_nan[i], r_big[i]))
    lo, hi = r_nan[7]
    assert torch.equal(bits(r_nan[6][lo:hi]), bits(r_big[6][lo:hi]))  # the state after the call
    rx, _, rout = generated(name, True)
    assert torch.equal(r_nan[1].view(case.B, -1), rx[:, T1 * case.S :, 0])
    assert all(torch.equal(g.transpose(0, 1), w[:, T1:]) for g, w in zip(r_nan[2], rout.z))
    assert torch.equal(r_nan[5], r_nan[1][:, -2:])  # x_state: the last two stacks


@gpu
@pytest.mark.parametrize("kw", [dict(t0=-1), dict(null_in=True), dict(null_state=True), dict(latent24=True)],
                         ids=["t0-negative", "x_in-NULL", "x_state-NULL", "latent-24"])  # fmt: skip
def test_c_abi_resume_refuses_before_touching_anything(kw):
    rc, x, zs, mus, sds, x_state, scratch, _, _, msg = resume_abi("b", 5, sentinel=(5.0, 7.0, 9.0), **kw)
    assert rc < 0 and len(msg) > 0
    assert bool((x == 7.0).all()) and bool((x_state == 9.0).all()) and bool((scratch == 5.0).all())
    assert all(bool((t == 7.0).all()) for ts in (zs, mus, sds) for t in ts)
    _hip.check_async("blvm_stcn_generate_resume")


@gpu
def test_c_abi_resume_of_zero_steps_hands_the_stacks_back():
    rc, x, zs, mus, sds, x_state, scratch, _, x_in, _ = resume_abi("b", 5, sentinel=(5.0, 7.0, 9.0), T=0)
    assert rc == 0
    _hip.check_async("blvm_stcn_generate_resume")
    assert torch.equal(x_state, x_in) and bool((scratch == 5.0).all()) and bool((x == 7.0).all())


# ---- a state that does not fit
@gpu
def test_a_mismatched_state_is_refused_and_left_alone():
    case = CASES["b"]
    m, eps, uni = on_device("b")
    _, out = gen(m, case, 2, *cut(eps, uni, 0, 2), fused=True, return_state=True)
    st = out.state
    before = (st.n_steps, st.x_window.clone(), st.z_window.clone(), st.scratch.clone())
    with pytest.raises(ValueError):  # made at B = 5
        m.generate(n_samples=4, max_timesteps=case.S, state=st)
    other = on_device("h")[0]  # C = 256: the same windows, another scratch size
    assert other.receptive_field == m.receptive_field and other.latent_size == m.latent_size
    with pytest.raises(ValueError, match="scratch"):
        other.generate(n_samples=case.B, max_timesteps=case.S, state=st)
    with pytest.raises(ValueError):  # S = 8: other windows
        on_device("c")[0].generate(n_samples=case.B, max_timesteps=8, state=st)
    torch.cuda.synchronize()
    assert st.n_steps == before[0] and torch.equal(st.x_window, before[1]) and torch.equal(st.z_window, before[2])
    assert torch.equal(st.scratch.view(torch.int32), before[3].view(torch.int32))
