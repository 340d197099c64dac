"""`STCN.generate` from a prompt or a state, on the CPU: the float64 restatement the GPU tests (tests/test_gpu_stcn_prompt.py) compare
against, the properties that make that comparison meaningful, and the argument checks.

`stcn_generate_from_f64` is `stcn_generate_f64` (tests/test_stcn_generate_cpu.py) with its two zero-initialised buffers — the stacks
and the output stack's input — pre-filled with a past: per step it re-evaluates the naive windows, no rings, no state.
`prompt_latents_f64` gives the latents over a prompt: "posterior" takes the z of `blvm_oracle.stcn_forward` on the prompt, "prior" runs
one time-parallel prior pass (`residual_stack_skips`, `stcn_gaussian`), which `test_prior_latents_of_a_free_run_are_its_own` ties to
free generation.

Prompt recipe: the model and the generation draws (eps, uniforms, cut to the T generated steps) are those of the case in
tests/test_stcn_generate_cpu.py; one `torch.Generator(seed)` draws prompt = 0.8 * tanh(randn(B, P'*S)), then prompt_eps[l] =
randn(P',B,z_l) for l = 0 .. n-1 in index order.  All in fp32, widened exactly.

Comparison rule of that file: no near ties — every prompt case's smallest float64 gap between the best and the second-best perturbed
logit is >= 1e-3 and at least half of its generated samples lie strictly inside (-1, 1), asserted below.  The prompt seeds in
PROMPTS were picked on the CPU so that both hold (for both latent modes where both are used); if a shape or the recipe changes they
must be picked again.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import blvm_oracle as O

from test_stcn_generate_cpu import CASES, MIN_GAP, NUM_MIX, build_model, inputs, observe, reference, stcn_generate_f64, visiting_order

# (case, prompt steps P'): (prompt seed, generated steps T, latent modes compared on the device)
PROMPTS = {
    ("b", 1): (301, 6, ("posterior",)),              # every ring must equal the zero-past steady state
    ("b", 3): (302, 6, ("posterior", "prior")),      # shorter than rf = 23: zero left padding, the dilation-4 ring at a non-zero phase
    ("b", 30): (303, 6, ("posterior",)),             # longer than the window
    ("c", 5): (304, 6, ("posterior", "prior")),      # two workgroups, partial row group, stacked head
    ("f", 5): (305, 6, ("posterior",)),              # top_down=False
    ("g", 5): (306, 6, ("posterior",)),              # dense=False
    ("d", 5): (307, 6, ("posterior",)),              # the mode
    ("e", 2): (317, 2, ("posterior",)),              # the default widths
}
PROMPT_RUNS = [(name, Pp, mode) for (name, Pp), (_, _, modes) in sorted(PROMPTS.items()) for mode in modes]


def state_dict64(m):
    return {k: v.detach().double() for k, v in m.state_dict().items()}


def receptive_field(sd, n_layers, n, base_dilation=2):
    return sum(O.wavenet_dilations(n_layers, n, base_dilation)) + 1 + (sd["causal.conv.weight"].size(2) - 1)


def stcn_generate_from_f64(sd, x_past, zin_past, eps, uniforms, T, B, S, n_layers, latent_size, top_down=True, dense=True, use_mode=False,
                           base_dilation=2, num_mix=NUM_MIX):
    """`stcn_generate_f64` continuing a past: x_past [B,S,P'] the stacks of steps 0 .. P'-1, zin_past [B,Zin,P'] the output stack's
    input over them (zeros stand in front of step 0, as there); T steps P', P'+1, ... are drawn with eps[l][t], uniforms[.][t]
    indexed from 0.  -> (x [B,T*S], z, mu, sd: per level [T,B,z_l], smallest gap between the best and the second-best (perturbed) logit)."""
    dt = sd["causal.conv.weight"].dtype
    n = len(latent_size)
    dil = O.wavenet_dilations(n_layers, n, base_dilation)
    rf = receptive_field(sd, n_layers, n, base_dilation)
    order = visiting_order(n, top_down)
    P = x_past.size(2)
    x = torch.zeros(B, S, rf + P + T, dtype=dt)
    x[:, :, rf : rf + P] = x_past
    zin = torch.zeros(B, sum(latent_size) if dense else latent_size[0], n_layers + P + T, dtype=dt)
    zin[:, :, n_layers : n_layers + P] = zin_past
    zs, mus, sds = ([torch.zeros(T, B, z, dtype=dt) for z in latent_size] for _ in range(3))
    gap = float("inf")
    for t in range(T):
        a = P + t
        h = F.conv1d(x[:, :, a : a + rf], sd["causal.conv.weight"], sd["causal.conv.bias"])
        d = O.residual_stack_skips(sd, "res_stack", h, dil, 1)[n - 1 :: n]
        for i, l in enumerate(order):
            inp = d[l][..., 0] if i == 0 else torch.cat([d[l][..., 0], zs[order[i - 1]][t]], -1)
            mus[l][t], sds[l][t] = O.stcn_gaussian(sd, f"prior.{l}", inp, 0.5)
            zs[l][t] = mus[l][t] + sds[l][t] * eps[l][t].to(dt)
        zin[:, :, n_layers + a] = torch.cat([z[t] for z in zs], -1) if dense else zs[0][t]
        logits, locs, log_scales = observe(sd, zin[:, :, a : a + n_layers + 1], n_layers, n, B, S, num_mix)
        if use_mode:
            score = logits
            xs = O.dmol_mode(logits, locs)
        else:
            u, v = uniforms[0][t].to(dt), uniforms[1][t].to(dt).unsqueeze(-1)
            score = logits - torch.log(-torch.log(u))
            xs = O.dmol_sample(logits, locs, log_scales, u, v)
        top = score.topk(2, dim=-1).values
        gap = min(gap, float((top[..., 0] - top[..., 1]).min()))
        x[:, :, rf + a] = xs.squeeze(-1)
    return x[:, :, rf + P :].permute(0, 2, 1).reshape(B, T * S), zs, mus, sds, gap


def prompt_latents_f64(sd, prompt, prompt_eps, mode, S, n_layers, latent_size, top_down=True, dense=True, base_dilation=2):
    """z per level [P',B,z_l] over prompt [B,P'*S] with the draws prompt_eps[l] [P',B,z_l]: the posterior's (`blvm_oracle.stcn_forward`
    on the prompt) or, mode "prior", each level from its prior given x[<t] in one time-parallel pass."""
    dt = sd["causal.conv.weight"].dtype
    B, n = prompt.size(0), len(latent_size)
    Pp = prompt.size(1) // S
    prompt, prompt_eps = prompt.to(dt), [e.to(dt) for e in prompt_eps]
    if mode == "posterior":
        fwd = O.stcn_forward(sd, prompt, torch.full((B,), Pp * S), [e.transpose(0, 1) for e in prompt_eps], n_layers, list(latent_size),
                             n_stack_frames=S, base_dilation=base_dilation, dense=dense, top_down=top_down)  # fmt: skip
        return [z.transpose(0, 1) for z in fwd["z"]]
    assert mode == "prior"
    dil = O.wavenet_dilations(n_layers, n, base_dilation)
    rf = receptive_field(sd, n_layers, n, base_dilation)
    h = F.pad(prompt.view(B, Pp, S).transpose(1, 2), (rf, 0))
    h = F.conv1d(h, sd["causal.conv.weight"], sd["causal.conv.bias"])
    d = O.residual_stack_skips(sd, "res_stack", h, dil, Pp + 1)[n - 1 :: n]
    order = visiting_order(n, top_down)
    z = [None] * n
    for i, l in enumerate(order):
        inp = d[l][..., :-1].permute(2, 0, 1)  # [P',B,C]: the features that have seen x[<t]
        if i > 0:
            inp = torch.cat([inp, z[order[i - 1]]], -1)
        mu, sdv = O.stcn_gaussian(sd, f"prior.{l}", inp, 0.5)
        z[l] = mu + sdv * prompt_eps[l]
    return z


def past_of(x, z, B, S, dense):
    """(x_past [B,S,P'], zin_past [B,Zin,P']) from samples x [B,P'*S] and z per level [P',B,z_l]."""
    Pp = x.size(1) // S
    zin = torch.cat(z, -1) if dense else z[0]
    return x.view(B, Pp, S).transpose(1, 2), zin.permute(1, 2, 0)


def prompt_inputs(name, Pp):
    """(prompt [B,P'*S], prompt_eps per level [P',B,z_l]) in fp32 from the prompt seed of (case, P')."""
    case = CASES[name]
    g = torch.Generator().manual_seed(PROMPTS[(name, Pp)][0])
    prompt = 0.8 * torch.tanh(torch.randn(case.B, Pp * case.S, generator=g))
    return prompt, [torch.randn(Pp, case.B, z, generator=g) for z in case.latents]


def continue_f64(case, sd, x_past, zin_past, eps, uni, T):
    return stcn_generate_from_f64(sd, x_past, zin_past, eps, uni, T, case.B, case.S, case.n_layers, list(case.latents), case.top_down,
                                  case.dense, case.mode)  # fmt: skip


@functools.lru_cache(maxsize=None)
def prompt_reference(name, Pp, mode):
    """ns-like dict of a prompt run — computed once, never changed: model (CPU), prompt, prompt_eps, eps / uniforms of the T generated
    steps, prompt_z (float64, per level [P',B,z_l]) and the float64 x [B,T*S], z, mu, sd (per level [T,B,z_l]), gap."""
    case = CASES[name]
    T = PROMPTS[(name, Pp)][1]
    m = build_model(case)
    eps, (u, v) = inputs(case)
    eps, uni = [e[:T] for e in eps], (u[:T], v[:T])
    prompt, prompt_eps = prompt_inputs(name, Pp)
    sd = state_dict64(m)
    pz = prompt_latents_f64(sd, prompt, prompt_eps, mode, case.S, case.n_layers, list(case.latents), case.top_down, case.dense)
    x64, z64, mu64, sd64, gap = continue_f64(case, sd, *past_of(prompt.double(), pz, case.B, case.S, case.dense), eps, uni, T)
    return dict(model=m, prompt=prompt, prompt_eps=prompt_eps, eps=eps, uniforms=uni, T=T, prompt_z=pz, x=x64, z=z64, mu=mu64, sd=sd64, gap=gap)


def same(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "f", "g"])
def test_an_empty_past_is_the_zero_start(name):
    case = CASES[name]
    m, eps, uni, x64, z64, mu64, sd64, gap = reference(name)
    sd = state_dict64(m)
    Zin = sum(case.latents) if case.dense else case.latents[0]
    x, z, mu, sdv, g = continue_f64(case, sd, torch.zeros(case.B, case.S, 0, dtype=torch.float64), torch.zeros(case.B, Zin, 0, dtype=torch.float64),
                                    eps, uni, case.T)  # fmt: skip
    assert torch.equal(x, x64) and same(z, z64) and same(mu, mu64) and same(sdv, sd64) and g == gap


@pytest.mark.parametrize("name,T1", [("b", 5), ("b", 1), ("c", 4), ("d", 2), ("f", 3), ("g", 3)])
def test_two_chunks_are_the_long_run(name, T1):
    """T1 steps, then the rest from the first run's past, equal one run exactly in float64."""
    case = CASES[name]
    m, eps, (u, v), x64, z64, mu64, sd64, _ = reference(name)
    sd = state_dict64(m)
    first = stcn_generate_f64(sd, [e[:T1] for e in eps], (u[:T1], v[:T1]), T1, case.B, case.S, case.n_layers, list(case.latents), case.top_down,
                              case.dense, case.mode)  # fmt: skip
    assert torch.equal(first[0], x64[:, : T1 * case.S]) and same(first[1], [z[:T1] for z in z64])
    x, z, mu, sdv, _ = continue_f64(case, sd, *past_of(first[0], first[1], case.B, case.S, case.dense), [e[T1:] for e in eps],
                                    (u[T1:], v[T1:]), case.T - T1)  # fmt: skip
    assert torch.equal(x, x64[:, T1 * case.S :])
    assert same(z, [t[T1:] for t in z64]) and same(mu, [t[T1:] for t in mu64]) and same(sdv, [t[T1:] for t in sd64])


@pytest.mark.parametrize("name,T1", [("b", 5), ("c", 4), ("d", 2), ("f", 3), ("g", 3)])
def test_prior_latents_of_a_free_run_are_its_own(name, T1):
    """To 1e-12: the "prior" latents of a free run's own x under the same eps are that run's z, and the continuation from that past is
    the run's tail."""
    case = CASES[name]
    m, eps, (u, v), x64, z64, mu64, sd64, _ = reference(name)
    sd = state_dict64(m)
    S = case.S
    pz = prompt_latents_f64(sd, x64[:, : T1 * S], [e[:T1] for e in eps], "prior", S, case.n_layers, list(case.latents), case.top_down, case.dense)
    for l in range(len(case.latents)):
        assert float((pz[l] - z64[l][:T1]).abs().max()) <= 1e-12
    x, z, mu, sdv, _ = continue_f64(case, sd, *past_of(x64[:, : T1 * S], pz, case.B, S, case.dense), [e[T1:] for e in eps], (u[T1:], v[T1:]),
                                    case.T - T1)  # fmt: skip
    assert float((x - x64[:, T1 * S :]).abs().max()) <= 1e-12
    for got, want in ((z, z64), (mu, mu64), (sdv, sd64)):
        assert all(float((g - w[T1:]).abs().max()) <= 1e-12 for g, w in zip(got, want))


@pytest.mark.parametrize("name,Pp,mode", PROMPT_RUNS)
def test_prompt_cases_have_no_near_ties_and_are_not_vacuous(name, Pp, mode):
    r = prompt_reference(name, Pp, mode)
    inside = float((r["x"].abs() < 1).double().mean())
    print(f"case {name} P'={Pp} {mode}: smallest (perturbed-)logit gap {r['gap']:.2e}, {inside:.2f} of the samples inside (-1, 1)")
    assert r["gap"] >= MIN_GAP, f"case {name} P'={Pp} {mode}: (perturbed-)logit gap {r['gap']:.2e}: pick another prompt seed"
    assert inside >= 0.5


def test_posterior_prompt_latents_differ_from_prior_ones():
    """The two modes are different pasts (otherwise comparing both would show nothing)."""
    a, b = prompt_reference("c", 5, "posterior"), prompt_reference("c", 5, "prior")
    assert float((a["prompt_z"][0] - b["prompt_z"][0]).abs().max()) > 1e-2


# ---- the argument checks of `STCN.generate`, all before the device check: the model sits on the CPU, a device call would fail differently
def check_model():
    case = CASES["c"]  # S = 8, latents (16, 16, 32), rf = 23, n_layers = 3
    return case, build_model(case)


def good_state(m, case, B):
    from blvm.models.stcn.stcn import STCNDecodeState

    return STCNDecodeState(4, torch.zeros(m.receptive_field, B, case.S), torch.zeros(case.n_layers, B, sum(case.latents)), None)


def test_a_valid_prompt_or_state_reaches_the_device_check():
    """On a CPU model every valid call ends at the device check (BlvmHipError).  With a prompt that error is also the
    NotImplementedError that `generate(x=...)` has always raised where a prompt cannot be continued."""
    from blvm._hip import BlvmHipError

    case, m = check_model()
    B, S = 3, case.S
    with pytest.raises(BlvmHipError):
        m.generate(n_samples=B, max_timesteps=2 * S, x=torch.zeros(B, 2 * S))
    with pytest.raises(BlvmHipError):
        m.generate(n_samples=B, max_timesteps=2 * S, x=torch.zeros(B, 2 * S, 1), prompt_latents="prior",
                   prompt_eps=[torch.zeros(2, B, z) for z in case.latents], return_state=True)
    with pytest.raises(BlvmHipError):
        m.generate(n_samples=B, max_timesteps=2 * S, state=good_state(m, case, B))
    with pytest.raises(NotImplementedError, match="prompt"):
        m.generate(n_samples=B, max_timesteps=2 * S, x=torch.zeros(B, 2 * S))
    with pytest.raises(BlvmHipError) as info:
        m.generate(n_samples=B, max_timesteps=2 * S, state=good_state(m, case, B))
    assert not isinstance(info.value, NotImplementedError)


def test_prompt_arguments_are_checked_without_a_device():
    case, m = check_model()
    B, S = 3, case.S
    ok_x = torch.zeros(B, 2 * S)
    ok_pe = [torch.zeros(2, B, z) for z in case.latents]
    bad = [
        dict(x=ok_x, state=good_state(m, case, B)),               # both
        dict(x=torch.zeros(B + 1, 2 * S)),                        # rows != n_samples
        dict(x=torch.zeros(B, S - 1)),                            # P < S
        dict(x=torch.zeros(B, 2 * S + 3)),                        # P % S != 0
        dict(x=torch.zeros(B, 0)),                                # empty
        dict(x=torch.zeros(B)),                                   # 1-D
        dict(x=torch.zeros(B, 2 * S, 1, 1)),                      # 4-D
        dict(x=torch.zeros(B, 2 * S, 2)),                         # last dim != 1
        dict(x=ok_x, prompt_latents="both"),
        dict(prompt_latents=None),
        dict(x=ok_x, prompt_eps=ok_pe[:-1]),
        dict(x=ok_x, prompt_eps=[e[:1] for e in ok_pe]),          # wrong P'
        dict(x=ok_x, prompt_eps=[e[:, :2] for e in ok_pe]),       # wrong rows
        dict(x=ok_x, prompt_eps=[ok_pe[0], ok_pe[1], ok_pe[2][..., :16]]),
        dict(x=ok_x, prompt_eps=ok_pe[0]),
        dict(prompt_eps=ok_pe),                                   # without a prompt
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            m.generate(n_samples=B, max_timesteps=2 * S, **kw)


def test_state_arguments_are_checked_without_a_device():
    from blvm.models.stcn.stcn import STCNDecodeState

    case, m = check_model()
    B, S, rf, nl, Zin = 3, case.S, m.receptive_field, case.n_layers, sum(case.latents)
    with pytest.raises(ValueError, match="multiple"):
        m.generate(n_samples=B, max_timesteps=2 * S + 1, return_state=True)
    with pytest.raises(ValueError, match="multiple"):
        m.generate(n_samples=B, max_timesteps=2 * S - 1, state=good_state(m, case, B))
    bad_states = [
        good_state(m, case, B + 1),                                                  # another batch size
        STCNDecodeState(4, torch.zeros(rf - 1, B, S), torch.zeros(nl, B, Zin)),     # another receptive field
        STCNDecodeState(4, torch.zeros(rf, B, S + 1), torch.zeros(nl, B, Zin)),     # another stack size
        STCNDecodeState(4, torch.zeros(rf, B, S), torch.zeros(nl, B, Zin - 16)),    # other latent widths
        STCNDecodeState(4, torch.zeros(rf, B, S), torch.zeros(nl + 1, B, Zin)),     # another output stack
        STCNDecodeState(4, torch.zeros(rf, B, S), torch.zeros(nl, B, Zin), torch.zeros(8)),  # a scratch buffer of another size
        "state",
    ]
    for st in bad_states:
        with pytest.raises(ValueError):
            m.generate(n_samples=B, max_timesteps=2 * S, state=st)
    st = bad_states[5]
    assert st.n_steps == 4 and st.scratch.numel() == 8 and tuple(st.x_window.shape) == (rf, B, S)
