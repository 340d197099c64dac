"""`STCN.generate` on the device: the one-launch kernel (`blvm_stcn_generate`, csrc/stcn_decode.hip) and the step-by-step path against
the float64 restatement of tests/test_stcn_generate_cpu.py, which also defines the cases, their seeds and the comparison rule (no near
ties: every case's smallest perturbed-logit gap is >= 1e-3, asserted there on the CPU).

Bars: every sample within 1e-4 of the restatement (the bar of tests/test_wavenet_prompt.py and tests/test_gpu_lstm_generate.py for the
same kind of free-running comparison), z / prior_mus / prior_sds at rel-L2 2e-5 per level (the project's state bar), the two paths
within 1e-4 of each other.  The same restatement in fp32 on the CPU differs from float64 by <= 1.5e-7 in x and <= 8.7e-8 rel-L2 in z
on cases a-g, so the bars have two to three orders of margin.

Measured on an MI355X (fp32 operands), max |x - x64| / largest rel-L2 over the levels of z / of prior_mus / of prior_sds:
  one launch   a 1.1e-09 / 1.1e-07 / 5.1e-08 / 1.1e-07   b 5.3e-08 / 9.8e-08 / 5.1e-08 / 9.9e-08   c 2.1e-07 / 1.0e-07 / 7.0e-08 / 1.0e-07
               d 2.7e-08 / 1.0e-07 / 7.6e-08 / 1.0e-07   e 1.6e-07 / 1.1e-07 / 2.8e-07 / 1.0e-07   f 1.1e-07 / 1.0e-07 / 6.4e-08 / 9.9e-08
               g 1.1e-07 / 1.0e-07 / 8.1e-08 / 1.0e-07   h 6.0e-08 / 1.0e-07 / 2.5e-07 / 1.0e-07
  step by step a 6.4e-09 / 8.7e-08 / 5.4e-08 / 1.0e-07   b 6.2e-08 / 1.0e-07 / 4.7e-08 / 1.0e-07   c 2.1e-07 / 1.0e-07 / 7.0e-08 / 1.0e-07
               d 3.1e-08 / 1.1e-07 / 7.1e-08 / 9.9e-08   e 1.6e-07 / 1.1e-07 / 2.8e-07 / 1.0e-07   f 1.1e-07 / 1.0e-07 / 6.5e-08 / 1.0e-07
               g 1.1e-07 / 9.8e-08 / 7.5e-08 / 1.0e-07   h 6.0e-08 / 1.1e-07 / 2.5e-07 / 9.9e-08
  max |step by step - one launch|: a 7.5e-09, b 6.0e-08, c 1.8e-07, d 3.0e-08, e 7.5e-08, f 1.2e-07, g 1.2e-07, h 3.0e-08
"""
import copy
import ctypes
import functools

import pytest
import torch

from blvm import _hip, ops

from test_stcn_generate_cpu import CASES, MIN_GAP, NUM_MIX, reference

gpu = pytest.mark.gpu
DEV = "cuda:0"
X_TOL, S_TOL = 1e-4, 2e-5


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@functools.lru_cache(maxsize=None)
def on_device(name):
    """(model, eps, uniforms) of a case on the device."""
    m, eps, uni, *_ = reference(name)
    return copy.deepcopy(m).to(DEV), [e.to(DEV) for e in eps], (uni[0].to(DEV), uni[1].to(DEV))


def run(name, fused, max_timesteps=None):
    case = CASES[name]
    m, eps, uni = on_device(name)
    N = case.T * case.S if max_timesteps is None else max_timesteps
    (x, x_sl), out = m.generate(n_samples=case.B, max_timesteps=N, use_mode_observations=case.mode, eps=eps,
                                uniforms=None if case.mode else uni, fused=fused)  # fmt: skip
    torch.cuda.synchronize()
    _hip.check_async("STCN.generate")
    return x, x_sl, out


@functools.lru_cache(maxsize=None)
def generated(name, fused):
    """(x [B,T'*S,1], x_sl, ns(z, prior_mus, prior_sds)) of a case on one path — computed once."""
    return run(name, fused)


def check_against_f64(name, fused):
    case = CASES[name]
    *_, x64, z64, mu64, sd64, gap = reference(name)
    assert gap >= MIN_GAP
    x, x_sl, out = generated(name, fused)
    N = case.T * case.S
    assert tuple(x.shape) == (case.B, N, 1) and x_sl.tolist() == [N] * case.B
    dx = float((x[..., 0].double().cpu() - x64).abs().max())
    errs = []
    for got, want in ((out.z, z64), (out.prior_mus, mu64), (out.prior_sds, sd64)):
        assert len(got) == len(case.latents)
        for l, Z in enumerate(case.latents):
            assert tuple(got[l].shape) == (case.B, case.T, Z)
        errs.append(max(rel_l2(got[l], want[l].transpose(0, 1)) for l in range(len(case.latents))))
    print(f"case {name} fused={fused}: max |x - x64| {dx:.2e}, rel-L2 z {errs[0]:.2e}, prior_mus {errs[1]:.2e}, prior_sds {errs[2]:.2e}")
    assert dx <= X_TOL and max(errs) <= S_TOL, (dx, errs)


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
    """-> list that receives one entry per `ops.stcn_generate` call from the zero start (the model calls it as `ops.stcn_generate`,
    with `resume=` by keyword)."""
    seen, real = [], ops.stcn_generate

    def wrapped(*a, **k):
        out = real(*a, **k)
        if k.get("resume") is None:
            seen.append(out)
        return out

    monkeypatch.setattr(ops, "stcn_generate", wrapped)
    return seen


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_default_takes_the_one_launch_path(name, monkeypatch):
    seen = counting(monkeypatch)
    x, _, out = run(name, None)
    assert len(seen) == 1
    rx, _, rout = generated(name, True)
    assert torch.equal(x, rx)
    for got, want in ((out.z, rout.z), (out.prior_mus, rout.prior_mus), (out.prior_sds, rout.prior_sds)):
        assert all(torch.equal(g, w) for g, w in zip(got, want))


@gpu
@pytest.mark.parametrize("likelihood", ["GMM", "Gaussian"])
def test_other_heads_run_step_by_step(likelihood, monkeypatch):
    from blvm.models.stcn.stcn import STCN

    B, S, N, latents = 3, 8, 20, [16, 16, 32]
    torch.manual_seed(21)
    m = STCN(likelihood=likelihood, n_layers=3, latent_size=latents, res_channels=16, n_stack_frames=S).to(DEV)
    seen = counting(monkeypatch)
    for mode in (False, True):
        (x, x_sl), out = m.generate(n_samples=B, max_timesteps=N, use_mode_observations=mode)
        torch.cuda.synchronize()
        assert len(seen) == 0
        assert tuple(x.shape) == (B, N, 1) and x_sl.tolist() == [N] * B and bool(torch.isfinite(x).all())
        for ts in (out.z, out.prior_mus, out.prior_sds):
            assert [tuple(t.shape) for t in ts] == [(B, 3, Z) for Z in latents] and all(bool(torch.isfinite(t).all()) for t in ts)
    with pytest.raises(_hip.BlvmHipError):  # an explicit fused=True insists
        m.generate(n_samples=B, max_timesteps=N, fused=True)
    _hip.check_async("STCN.generate")


@gpu
def test_device_rng_draws():
    m = on_device("c")[0]
    (a, x_sl), oa = m.generate(n_samples=4, max_timesteps=24)
    (b, _), _ = m.generate(n_samples=4, max_timesteps=24)
    torch.cuda.synchronize()
    _hip.check_async("STCN.generate")
    assert tuple(a.shape) == (4, 24, 1) and x_sl.tolist() == [24] * 4
    assert [tuple(t.shape) for t in oa.z] == [(4, 3, Z) for Z in CASES["c"].latents]
    for x in (a, b):
        assert bool(torch.isfinite(x).all()) and float(x.abs().max()) <= 1.0
    assert not torch.equal(a, b)


@gpu
@pytest.mark.parametrize("fused", [True, False])
def test_output_is_cut_to_max_timesteps(fused):
    """20 samples at S = 8 run three steps and return the first 20 samples of the 24-sample run with the same draws."""
    case = CASES["f"]
    m, eps, uni = on_device("f")
    (x, x_sl), out = m.generate(n_samples=case.B, max_timesteps=20, eps=[e[:3] for e in eps], uniforms=(uni[0][:3], uni[1][:3]), fused=fused)
    (full, _), _ = m.generate(n_samples=case.B, max_timesteps=24, eps=[e[:3] for e in eps], uniforms=(uni[0][:3], uni[1][:3]), fused=fused)
    torch.cuda.synchronize()
    _hip.check_async("STCN.generate")
    assert tuple(x.shape) == (case.B, 20, 1) and x_sl.tolist() == [20] * case.B and tuple(out.z[0].shape) == (case.B, 3, case.latents[0])
    assert torch.equal(x, full[:, :20])
    assert torch.equal(full, generated("f", fused)[0][:, :24])


def call_c_abi(name, fill, C=None, num_mix=NUM_MIX, n=None, out_fill=None):
    """`blvm_stcn_generate` called directly on a case's tensors with scratch and outputs prefilled.  -> (rc, x, z, mu, sd, scratch)."""
    case = CASES[name]
    m, eps, (u, v) = on_device(name)
    p = ops.stcn_generate_pack(m._one_launch_parts(), case.S, NUM_MIX)
    lib, T, B, S = p.lib, case.T, case.B, case.S
    f32 = dict(device=DEV, dtype=torch.float32)
    n_scratch = int(lib.blvm_stcn_generate_scratch_floats(p.dil, p.C, S, p.n_blocks, p.n_out, p.latent, p.order, p.n, p.dense, NUM_MIX, B))
    assert n_scratch > 0
    scratch = torch.full((n_scratch,), fill, **f32)
    of = fill if out_fill is None else out_fill
    x = torch.full((B, T, S), of, **f32)
    zs, mus, sds = ([torch.full((T, B, Z), of, **f32) for Z in case.latents] for _ in range(3))
    ptrs = lambda ts: (ctypes.c_void_p * 9)(*([ops.ptr(t) for t in ts] + [None] * (9 - len(ts))))  # noqa: E731
    ints9 = lambda a: (ctypes.c_int * 9)(*(list(a) + [16] * (9 - len(a))))  # noqa: E731
    p0, lik, blk = m.prior[0], m.likelihood_module, m.res_stack.res_blocks[0]
    rc = lib.blvm_stcn_generate(ops.ptr(p.packed), p.dil, p.groups, p.n_blocks, p.n_out, ints9(p.latent), ints9(p.order), p.n if n is None else n,
                                p.dense, B, p.C if C is None else C, S, num_mix, T, blk.inv_std, m.inv_std, p0.softplus_beta, p0.epsilon,
                                p0.transform_mu[1].negative_slope, lik.log_epsilon, ptrs(eps), ops.ptr(u), ops.ptr(v), ops.ptr(x), ptrs(zs),
                                ptrs(mus), ptrs(sds), ops.ptr(scratch), ops.stream_ptr())  # fmt: skip
    torch.cuda.synchronize()
    return rc, x, zs, mus, sds, scratch


@gpu
@pytest.mark.parametrize("name", ["c", "h"])
def test_c_abi_results_do_not_depend_on_prior_buffer_contents(name):
    r_nan = call_c_abi(name, float("nan"))
    r_big = call_c_abi(name, 1e30)
    assert r_nan[0] == 0 and r_big[0] == 0
    _hip.check_async("blvm_stcn_generate")
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    assert torch.equal(bits(r_nan[1]), bits(r_big[1]))
    for i in (2, 3, 4):
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(r_nan[i], r_big[i]))
    case = CASES[name]
    assert torch.equal(r_nan[1].view(case.B, -1), generated(name, True)[0][..., 0])


@gpu
@pytest.mark.parametrize("kw", [dict(C=24), dict(num_mix=11), dict(n=9)], ids=["C24", "K11", "n9"])
def test_c_abi_refuses_bad_arguments_before_touching_anything(kw):
    rc, x, zs, mus, sds, scratch = call_c_abi("b", 5.0, out_fill=7.0, **kw)
    assert rc != 0
    assert bool((x == 7.0).all()) and bool((scratch == 5.0).all())
    assert all(bool((t == 7.0).all()) for ts in (zs, mus, sds) for t in ts)
