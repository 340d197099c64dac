"""`STCN.generate` on the CPU: the float64 restatement the GPU tests (tests/test_gpu_stcn_generate.py) compare against, the properties
that make that comparison meaningful, its consistency with the model's own `forward`, and the argument checks.

The reference cannot sample from its STCN (its `generate` raises), so there are no reference samples to pin against.  The oracle is
`stcn_generate_f64` below: per step it re-evaluates the zero-padded receptive-field window with `blvm_oracle`'s
`residual_stack_skips`, `stcn_gaussian`, `dmol_head`, `dmol_sample` and `dmol_mode` — no ring buffers, no steady state —, and
`test_restatement_is_consistent_with_teacher_forcing` ties it to the time-parallel pass of `blvm_oracle.stcn_forward`.

Case recipe: `torch.manual_seed(wseed)`, `STCN(likelihood="DMoL", ...)` on the CPU, the head's log-scale biases lowered by 2 so that
most draws stay inside (-1, 1); one `torch.Generator(dseed)` draws eps[l] = randn(T',B,z_l) for l = 0 .. n-1 in index order, then u,
then v.  All in fp32, widened exactly.

Comparison rule (as tests/test_lstm_generate_cpu.py): a Gumbel-max tie would flip a component and everything after it, so ties are
excluded by construction — `test_cases_have_no_near_ties` asserts for every case that the smallest float64 gap between the best and
the second-best perturbed logit (plain logit for the mode) over all rows, steps and samples is >= 1e-3.  The seeds were picked so that
it holds; if a shape or the draw recipe changes they must be picked again.
"""
import collections
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import blvm_oracle as O

MIN_GAP = 1e-3
NUM_MIX = 10

# S = n_stack_frames, C = res_channels, T = model steps T'; seeds: (weights, draws)
Case = collections.namedtuple("Case", "S C n_layers latents B T mode top_down dense seeds")
CASES = {
    "a": Case(1, 16, 2, (16, 16), 1, 1, False, True, True, (0, 100)),                  # the smallest: prologue only
    "b": Case(1, 16, 3, (16, 16, 32), 5, 12, False, True, True, (1, 101)),             # dilation-4 ring wraps three times, partial row group
    "c": Case(8, 16, 3, (16, 16, 32), 17, 9, False, True, True, (2, 105)),             # two workgroups, stacked head
    "d": Case(8, 16, 3, (16, 16, 32), 5, 6, True, True, True, (9, 1009)),              # use_mode_observations=True
    "e": Case(64, 256, 5, (256, 128, 64, 32, 16), 16, 2, False, True, True, (4, 112)),  # the default widths: LDS map, chunked head
    "f": Case(8, 16, 3, (16, 16, 32), 5, 6, False, False, True, (5, 105)),             # top_down=False
    "g": Case(8, 16, 3, (16, 16, 32), 5, 6, False, True, False, (6, 106)),             # dense=False
    "h": Case(1, 256, 3, (16, 16, 32), 3, 9, False, True, True, (12, 112)),             # full width with ring wrap
}


def build_model(case):
    from blvm.models.stcn.stcn import STCN

    torch.manual_seed(case.seeds[0])
    m = STCN(likelihood="DMoL", n_layers=case.n_layers, latent_size=list(case.latents), res_channels=case.C, n_stack_frames=case.S,
             dense=case.dense, top_down=case.top_down)  # fmt: skip
    with torch.no_grad():
        m.likelihood_module.params.bias[2 * NUM_MIX :] -= 2.0
    return m.eval()


def inputs(case):
    """(eps: per level [T',B,z_l], (u [T',B,S,K], v [T',B,S])) in fp32 from the case's draw seed."""
    g = torch.Generator().manual_seed(case.seeds[1])
    eps = [torch.randn(case.T, case.B, z, generator=g) for z in case.latents]
    u = torch.empty(case.T, case.B, case.S, NUM_MIX).uniform_(1e-5, 1.0 - 1e-5, generator=g)
    v = torch.empty(case.T, case.B, case.S).uniform_(1e-8, 1.0 - 1e-8, generator=g)
    return eps, (u, v)


def visiting_order(n, top_down):
    return list(reversed(range(n))) if top_down else list(range(n))


def observe(sd, zin_window, n_layers, n, B, S, num_mix):
    """Output stack on a window [B,Zin,n_layers + frames] -> head parameters of `frames` steps: (logits, locs, log_scales) [B,frames*S,..]."""
    frames = zin_window.size(2) - n_layers
    logits = sum(O.residual_stack_skips(sd, "out_transform", zin_window, [1] * n_layers, frames)) * (1 / math.sqrt(n))
    up = F.relu(F.linear(logits.permute(0, 2, 1), sd["out_upsample.0.weight"], sd["out_upsample.0.bias"]))  # [B,frames,S*3K]
    up = up.reshape(B, frames * S, 3 * num_mix)
    return O.dmol_head(up, sd["likelihood_module.params.weight"], sd["likelihood_module.params.bias"], num_mix)


def stcn_generate_f64(sd, eps, uniforms, T, B, S, n_layers, latent_size, top_down=True, dense=True, use_mode=False, base_dilation=2,
                      num_mix=NUM_MIX):
    """STCN.generate restated naively in the dtype of `sd` (float64 here).  For t = 0 .. T-1: the dilated stack on the window of the
    last receptive_field stacks (zeros before the start) gives d_t[l]; z_t[l] = mu + sd * eps[l][t] with (mu, sd) = prior[l](cat[d_t[l],
    z_t[level visited before]]); the output stack on the window (n_layers zero frames, then z_0 .. z_t) gives the head parameters of x_t.
    -> (x [B,T*S], z, mu, sd: per level [T,B,z_l], smallest gap between the best and the second-best (perturbed) logit)."""
    dt = sd["causal.conv.weight"].dtype
    n = len(latent_size)
    dil = O.wavenet_dilations(n_layers, n, base_dilation)
    rf = sum(dil) + 1 + (sd["causal.conv.weight"].size(2) - 1)
    order = visiting_order(n, top_down)
    x = torch.zeros(B, S, rf + T, dtype=dt)  # [B,channels,frames]
    zin = torch.zeros(B, sum(latent_size) if dense else latent_size[0], n_layers + T, dtype=dt)
    zs, mus, sds = ([torch.zeros(T, B, z, dtype=dt) for z in latent_size] for _ in range(3))
    gap = float("inf")
    for t in range(T):
        h = F.conv1d(x[:, :, t : t + rf], sd["causal.conv.weight"], sd["causal.conv.bias"])
        d = O.residual_stack_skips(sd, "res_stack", h, dil, 1)[n - 1 :: n]
        for i, l in enumerate(order):
            inp = d[l][..., 0] if i == 0 else torch.cat([d[l][..., 0], zs[order[i - 1]][t]], -1)
            mus[l][t], sds[l][t] = O.stcn_gaussian(sd, f"prior.{l}", inp, 0.5)
            zs[l][t] = mus[l][t] + sds[l][t] * eps[l][t].to(dt)
        zin[:, :, n_layers + t] = torch.cat([z[t] for z in zs], -1) if dense else zs[0][t]
        logits, locs, log_scales = observe(sd, zin[:, :, t : t + n_layers + 1], n_layers, n, B, S, num_mix)
        if use_mode:
            score = logits
            xs = O.dmol_mode(logits, locs)
        else:
            u, v = uniforms[0][t].to(dt), uniforms[1][t].to(dt).unsqueeze(-1)
            score = logits - torch.log(-torch.log(u))
            xs = O.dmol_sample(logits, locs, log_scales, u, v)
        top = score.topk(2, dim=-1).values
        gap = min(gap, float((top[..., 0] - top[..., 1]).min()))
        x[:, :, rf + t] = xs.squeeze(-1)
    return x[:, :, rf:].permute(0, 2, 1).reshape(B, T * S), zs, mus, sds, gap


def run_restatement(case, m, eps, uni, dtype):
    sd = {k: v.detach().to(dtype) for k, v in m.state_dict().items()}
    return stcn_generate_f64(sd, eps, uni, case.T, case.B, case.S, case.n_layers, list(case.latents), case.top_down, case.dense, case.mode)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(model on the CPU, eps, uniforms, float64 x [B,T'*S], z, mu, sd per level [T',B,z_l], smallest gap) of a case — computed once,
    never changed."""
    case = CASES[name]
    m = build_model(case)
    eps, uni = inputs(case)
    return (m, eps, uni, *run_restatement(case, m, eps, uni, torch.float64))


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_have_no_near_ties(name):
    gap = reference(name)[7]
    print(f"case {name}: smallest (perturbed-)logit gap {gap:.2e}")
    assert gap >= MIN_GAP, f"case {name}: (perturbed-)logit gap {gap:.2e}: pick another seed"


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_are_not_vacuous(name):
    """At least half of the samples lie strictly inside (-1, 1): a comparison of clamped values would show nothing."""
    x64 = reference(name)[3]
    assert float((x64.abs() < 1).double().mean()) >= 0.5


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "f", "g"])
def test_restatement_is_consistent_with_teacher_forcing(name):
    """On the generated x, in float64 to 1e-12: ONE time-parallel pass (the padded sequence through the dilated stack, each level's
    prior given the generated z of its conditioning level, the output stack on the generated z, `dmol_sample` with the same draws)
    reproduces every mu, sd, z and x itself; and `blvm_oracle.stcn_forward` on the generated x gives the same prior mean for the first
    level visited, which depends on x only."""
    case = CASES[name]
    m, eps, (u, v), x64, z64, mu64, sd64, _ = reference(name)
    B, T, S, n, nl = case.B, case.T, case.S, len(case.latents), case.n_layers
    sd = {k: t.detach().double() for k, t in m.state_dict().items()}
    dil = O.wavenet_dilations(nl, n, 2)
    rf = sum(dil) + 2
    order = visiting_order(n, case.top_down)
    h = F.pad(x64.view(B, T, S).transpose(1, 2), (rf, 0))
    h = F.conv1d(h, sd["causal.conv.weight"], sd["causal.conv.bias"])
    d = O.residual_stack_skips(sd, "res_stack", h, dil, T + 1)[n - 1 :: n]
    for i, l in enumerate(order):
        inp = d[l][..., :-1].permute(2, 0, 1)  # [T,B,C]: d_p
        if i > 0:
            inp = torch.cat([inp, z64[order[i - 1]]], -1)
        mu, sdv = O.stcn_gaussian(sd, f"prior.{l}", inp, 0.5)
        assert float((mu - mu64[l]).abs().max()) <= 1e-12 and float((sdv - sd64[l]).abs().max()) <= 1e-12
        assert float((mu + sdv * eps[l].double() - z64[l]).abs().max()) <= 1e-12
    zin = torch.cat(z64, -1) if case.dense else z64[0]
    logits, locs, log_scales = observe(sd, F.pad(zin.permute(1, 2, 0), (nl, 0)), nl, n, B, S, NUM_MIX)
    if case.mode:
        again = O.dmol_mode(logits, locs)
    else:
        ub = u.double().permute(1, 0, 2, 3).reshape(B, T * S, NUM_MIX)
        vb = v.double().permute(1, 0, 2).reshape(B, T * S, 1)
        again = O.dmol_sample(logits, locs, log_scales, ub, vb)
    assert float((again.view(B, T * S) - x64).abs().max()) <= 1e-12

    fwd = O.stcn_forward(sd, x64, torch.full((B,), T * S), [e.double().transpose(0, 1) for e in eps], nl, list(case.latents), n_stack_frames=S,
                         dense=case.dense, top_down=case.top_down)  # fmt: skip
    first = order[0]
    assert float((fwd["mu_p"][first] - mu64[first].transpose(0, 1)).abs().max()) <= 1e-12


def test_generate_checks_its_arguments_without_a_device():
    """Wrong shapes of eps / uniforms and non-positive n_samples / max_timesteps raise ValueError, a prompt NotImplementedError with a
    message — all before any device call (the model sits on the CPU here: a device call would fail differently)."""
    case = CASES["c"]
    m = build_model(case)
    B, S, N = 3, case.S, 20  # T' = 3
    Tp = 3
    ok_eps = [torch.zeros(Tp, B, z) for z in case.latents]
    ok_u = (torch.rand(Tp, B, S, NUM_MIX), torch.rand(Tp, B, S))
    bad = [
        dict(eps=ok_eps[:-1]),
        dict(eps=[e[:2] for e in ok_eps]),
        dict(eps=[e[:, :2] for e in ok_eps]),
        dict(eps=[ok_eps[0], ok_eps[1], ok_eps[2][..., :16]]),
        dict(eps=ok_eps[0]),
        dict(uniforms=(ok_u[0],)),
        dict(uniforms=(ok_u[0][:2], ok_u[1][:2])),
        dict(uniforms=(ok_u[0][..., :5], ok_u[1])),
        dict(uniforms=(ok_u[0], ok_u[1][..., :-1])),
        dict(uniforms=(ok_u[0][:, :2], ok_u[1][:, :2])),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            m.generate(n_samples=B, max_timesteps=N, **kw)
    with pytest.raises(ValueError):
        m.generate(n_samples=0, max_timesteps=N)
    with pytest.raises(ValueError):
        m.generate(n_samples=B, max_timesteps=0)
    with pytest.raises(NotImplementedError, match="prompt"):
        m.generate(n_samples=B, max_timesteps=N, x=torch.zeros(B, 16))


def test_generate_is_implemented():
    """The default call no longer raises NotImplementedError: on a CPU model it gets as far as the device check."""
    from blvm._hip import BlvmHipError
    from blvm.models.stcn.stcn import STCN

    torch.manual_seed(0)
    m = STCN(likelihood="DMoL", n_layers=2, latent_size=[16, 16], res_channels=16)
    with pytest.raises(BlvmHipError):
        m.generate()
