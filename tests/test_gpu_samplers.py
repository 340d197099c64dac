"""GPU (MI355X): the mixture samplers draw by draw in trained-model regimes.  Every generator ends in mix_pick / logistic_draw
(csrc/decode_tiles.h); here each draw is compared with the float64 oracle (blvm_oracle.mix_draw_detail) on the inputs of
tests/golden/samplers.npz under the rule of tests/draw_cases.py: an undecided pick (float64 score gap below the fp32 evaluation
error of two scores) may go either way, a decided draw is held to 16 u (|loc| + sd (|log v| + |log(1 - v)|)), a value beyond the
clamp must be exactly +-1.0f, a mode is the location bit for bit.  tests/test_draw_cases_cpu.py asserts that the inputs reach the
regimes they are named after; tests/test_oracle_golden.py pins the oracle to the reference's own draws and samples.

  a. blvm_mix_sample directly: every regime, kind 0 and 1, K = 10 (unrolled) and 1, 3, 5, 32 (generic), the four NULL combinations of
     (u, v), n = 1, 255, 256, 257, 1000 with a sentinel behind the output, n = 0, twice for bit-identical results, and once through
     the two heads' sample / mode (the _pack layout, the sd_beta = 0 hand-off) against the reference's recorded samples.
  b. the in-kernel draw sites with the network taken out of the loop: the layer in front of the head has zero weight and the wanted
     parameters in its bias (>= 0, so ReLU / LeakyReLU pass them), the head Linear is a signed diagonal, so every position s of the
     frame stack draws from its own row whatever was fed back, and a wrong u / v index shows as one wrong draw at a known (t, b, s).

Measured on an MI355X (every test prints its figures: draws, undecided, worst err / bar; <= 1 passes).  No draw of the committed
inputs is undecided (share 0 % everywhere; tests/test_draw_cases_cpu.py::test_the_rule_itself walks that branch of the rule).
  blvm_mix_sample, worst err / bar over K = 10, 1, 3, 5, 32 and kind 1 (draws): floor 0.108 (1 536), saturation 0.110 (1 536),
    dominated 0.171 (4 608), ties 0.064 (1 152), ends 0.088 (1 440), trained 0.062 (1 536), gmm_sd0 0.058 (768), gmm_beta 0.148 (768);
    NULL combinations <= 0.089 (v set) and 0 (v NULL: bit-equal); the heads on the reference's draws 0.110 (DMoL, 1 968) / 0.055 (GMM, 512)
  draw sites, worst err / bar floor | saturation | dominated | ties | ends | trained (draws per regime), the mode bit-equal at each:
    blvm_vrnn_decode S 16 B 17          0.122 | 0.090 | 0.064 | 0.086 | 0.051 | 0.072  (816)
    blvm_vrnn_generate S 8, 16 B 5      0.122 | 0.080 | 0.064 | 0.086 | 0.051 | 0.094  (360)
    blvm_srnn_generate S 8, 16 B 5      0.122 | 0.080 | 0.064 | 0.086 | 0.051 | 0.094  (360)
    blvm_lstm_generate_any_stack S 1,24 0.107 | 0.066 | 0.080 | 0.069 | 0.050 | 0.067  (375; ends 360)
    blvm_stcn_generate S 8 B 3          0.068 | 0.057 | 0.048 | 0.049 | 0.050 | 0.094  (72)
    blvm_wavenet_decode B 19, 24 frames 0.060 | 0.068 | 0.071 | 0.041 |   -   | 0.052  (456 per launch, two trained rows)
  The float32 oracle on the CPU (torch) stays below 0.11 on the same inputs and the reference's own samples below 0.104, so the factor
  16 of the bar was left as the arithmetic gives it.
Two scratch builds of the library, each run against the whole GPU suite: without the fmaxf(raw, log_eps) of logistic_draw 19 of the
tests here fail (every regime test whose rows go below -7, the block-edge tests of kind 0, all nine draw-site tests) and nothing else
does; with `s > bv` turned into `s >= bv` in mix_pick_from 14 fail (ties and ends of the direct tests, the heads' modes, all nine
draw-site tests) and nothing else does.
"""
import pytest
import torch

import draw_cases as DC
from blvm import _hip, ops

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 12345.0


@pytest.fixture(scope="module", autouse=True)
def _require_hip():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert _hip.load().blvm_device_ok() == 1, "libblvm_hip: no gfx950 device visible"


@pytest.fixture(scope="module")
def loaded():
    return DC.load(GOLDEN)


def dev(t):
    return None if t is None else t.to(DEV)


def run_direct(reg, kind, consts, u=True, v=True):
    """ops.mix_sample on a regime, twice (bit-identical), judged by the rule."""
    log_eps, sd_beta, sd_eps = consts
    uu, vv = (reg["u"] if u else None), (DC.noise(reg, kind) if v else None)
    args = (dev(reg["par"]), dev(uu), dev(vv), kind, log_eps, sd_beta if sd_beta > 0 else 0.0, sd_eps)
    got = ops.mix_sample(*args)
    again = ops.mix_sample(*args)
    torch.cuda.synchronize()
    _hip.check_async()
    assert torch.equal(got, again), f"{reg['name']}: two launches on the same inputs differ"
    return DC.judge(reg["name"], got, reg["par"], uu, vv, kind, log_eps, sd_beta, sd_eps)


# ----------------------------------------------------------------------------------------------------------------------
# a. blvm_mix_sample
# ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", DC.DMOL_REGIMES + DC.GMM_REGIMES)
def test_mix_sample_regime(loaded, name):
    regs, fx = loaded
    cases = [c for c in DC.direct_cases(regs, fx) if c[0].split("-")[0] == name]
    assert len(cases) >= 3
    for cid, reg, kind, consts in cases:
        res = run_direct(reg, kind, consts)
        DC.report(f"mix_sample {cid}", res)


@pytest.mark.parametrize("name,kind", [("trained", 0), ("ties", 0), ("saturation", 0), ("ends", 0), ("gmm_beta", 1), ("gmm_sd0", 1), ("ties", 1)])
def test_mix_sample_null_combinations(loaded, name, kind):
    """u NULL: the arg-max-logit component (first maximum); v NULL: the location of the pick, not clamped; both: the mode."""
    regs, fx = loaded
    for K in (DC.K0, 3):
        reg = DC.with_K(regs[name], K)
        for u, v in ((False, True), (True, False), (False, False)):
            res = run_direct(reg, kind, DC.head_constants(name, kind, fx), u=u, v=v)
            DC.report(f"mix_sample {name}-kind{kind}-K{K} u={'set' if u else 'NULL'} v={'set' if v else 'NULL'}", res)
    if name == "saturation":  # the mode leaves |loc| > 1 as it is, like the reference's
        got = ops.mix_sample(dev(regs[name]["par"]), None, None, 0)
        assert torch.equal(got.cpu(), torch.from_numpy(fx["saturation_ref_mode"])) and int((got.abs() > 1).sum()) > 100


@pytest.mark.parametrize("kind,K", [(0, 10), (0, 3), (1, 10), (1, 3)])
def test_mix_sample_block_edge(loaded, kind, K):
    """n around the 256-thread block and over several blocks; the output's tail and the n = 0 call write nothing."""
    regs, fx = loaded
    name = "trained" if kind == 0 else "gmm_beta"
    base = DC.with_K(regs[name], K)
    log_eps, sd_beta, sd_eps = DC.head_constants(name, kind, fx)
    lib = _hip.load()
    for n in (1, 255, 256, 257, 1000):
        reg = DC.take(base, (torch.arange(n) * 7 + 3) % base["par"].shape[0])
        par, u, v = dev(reg["par"]), dev(reg["u"]), dev(DC.noise(reg, kind))
        outs = []
        for _ in range(2):
            out = torch.full((n + 300,), SENTINEL, device=DEV)
            _hip.check(lib.blvm_mix_sample(_hip.ptr(par), _hip.ptr(u), _hip.ptr(v), n, K, kind, log_eps, sd_beta, sd_eps, _hip.ptr(out),
                                           _hip.stream_ptr()), "blvm_mix_sample")
            torch.cuda.synchronize()
            outs.append(out.cpu())
        assert torch.equal(outs[0], outs[1])
        assert bool((outs[0][n:] == SENTINEL).all()), f"n = {n}: wrote past the output"
        DC.judge(f"{name}/n{n}", outs[0][:n], reg["par"], reg["u"], DC.noise(reg, kind), kind, log_eps, sd_beta, sd_eps)
    out = torch.full((64,), SENTINEL, device=DEV)
    rc = lib.blvm_mix_sample(_hip.ptr(dev(base["par"])), None, None, 0, K, kind, log_eps, sd_beta, sd_eps, _hip.ptr(out), _hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and bool((out == SENTINEL).all())
    _hip.check_async()


def test_heads_sample_and_mode_match_reference_draws(loaded):
    """DiscretizedLogisticMixtureDense / DiagonalGaussianMixtureDense .sample / .mode on (logits [N,K], a [N,1,K], b [N,1,K]) as their
    forward returns them, with the reference's recorded draws: the reference's recorded samples under the rule, its modes exactly."""
    from blvm.modules.distributions import DiagonalGaussianMixtureDense, DiscretizedLogisticMixtureDense

    regs, fx = loaded
    T = lambda k: torch.from_numpy(fx[k])  # noqa: E731
    dmol = DiscretizedLogisticMixtureDense(4, 1, num_mix=10, num_bins=2**16).to(DEV)
    for name in DC.DMOL_REGIMES:
        par = regs[name]["par"]
        u, v = (T(f"{name}_ref_{k}") if f"{name}_ref_{k}" in fx else T(f"{name}_{k}") for k in ("u", "v"))
        params = (dev(par[:, :10]), dev(par[:, 10:20].unsqueeze(1)), dev(par[:, 20:].unsqueeze(1).clamp(min=dmol.log_epsilon)))
        x = dmol.sample(params, uniforms=(dev(u), dev(v.unsqueeze(1))))
        assert x.shape == (par.shape[0], 1)
        res = DC.judge(name, x, par, u, v, 0)
        DC.report(f"DMoL head sample, reference draws, {name}", res)
        ref = T(f"{name}_ref_x").double()
        far = (x.cpu().squeeze(1).double() - ref).abs() > 2 * res["detail"]["bar"]  # both are within one bar of the float64 value
        assert int((far & ~res["detail"]["undecided"]).sum()) == 0
        assert torch.equal(dmol.mode(params).cpu().squeeze(1), T(f"{name}_ref_mode")), name
    gmm = DiagonalGaussianMixtureDense(4, 1, num_mix=10).to(DEV)
    beta, eps = float(fx["gmm_beta"]), float(fx["gmm_sd_eps"])
    for name in DC.GMM_REGIMES:
        par, u, n = regs[name]["par"], regs[name]["u"], regs[name]["n"]
        raw = par[:, 20:].unsqueeze(1)
        sd = raw if name == "gmm_sd0" else (torch.nn.functional.softplus(raw.double(), beta=beta) + eps).float()  # what forward hands on
        params = (dev(par[:, :10]), dev(par[:, 10:20].unsqueeze(1)), dev(sd))
        x = gmm.sample(params, noise=(dev(u), dev(n.unsqueeze(1))))
        packed = torch.cat([par[:, :20], sd.squeeze(1)], 1)
        res = DC.judge(name, x, packed, u, n, 1)
        DC.report(f"GMM head sample, reference draws, {name}", res)
        if name == "gmm_sd0":
            ref = T(f"{name}_ref_x").double()
            assert int(((x.cpu().squeeze(1).double() - ref).abs() > 2 * res["detail"]["bar"]).sum()) == 0
        assert torch.equal(gmm.mode(params).cpu().squeeze(1), T(f"{name}_ref_mode")), name
    _hip.check_async()


# ----------------------------------------------------------------------------------------------------------------------
# b. the in-kernel draw sites, the network taken out of the loop
# ----------------------------------------------------------------------------------------------------------------------


def rig(last, head, case):
    """Zero weight and bias a (>= 0) on the layer in front of the head, the signed diagonal and zero bias on the head Linear; returns
    the head parameters [S,30] computed in float64 from these fp32 weights through the same two layers (they are exact in fp32)."""
    a = case["a"].reshape(-1)
    with torch.no_grad():
        last.weight.zero_()
        last.bias.zero_()
        last.bias[: a.numel()] = a.to(last.bias.device)
        head.weight.zero_()
        head.bias.zero_()
        head.weight[torch.arange(30), torch.arange(30)] = DC.SIGNS.to(head.weight.device)
    act = torch.relu(last.bias.detach().cpu().double())
    S = case["S"]
    act = act.view(S, -1) if act.numel() == S * 30 else act.view(1, -1)
    rows = torch.nn.functional.linear(act, head.weight.detach().cpu().double(), head.bias.detach().cpu().double())
    assert torch.equal(rows.float().double(), rows) and torch.equal(rows.float(), case["rows"])
    return rows.float()


def site_draws(case):
    f, (S, B, T) = case["flat"], (case["S"], case["B"], case["T"])
    return f["u"].view(T, B, S, 10).to(DEV), f["v"].view(T, B, S).to(DEV)


def judge_site(site, case, x_bts, mode=False):
    """x_bts [B,T,S] from a launch -> the rule on its T*B*S draws in the order [t, b, s]; a failure names (t, b, s)."""
    torch.cuda.synchronize()
    _hip.check_async(site)
    f, (S, B, T) = case["flat"], (case["S"], case["B"], case["T"])
    assert tuple(x_bts.shape) == (B, T, S), (site, tuple(x_bts.shape))
    got = x_bts.permute(1, 0, 2).reshape(-1)
    res = DC.judge(f["name"], got, f["par"], None if mode else f["u"], None if mode else f["v"], 0, where=lambda i: f"{site} {DC.site_index(case, i)}")
    DC.report(f"{site} S={S} B={B} T={T} {f['name']}{' mode' if mode else ''}", res)
    return res


def site_cases(regs, site, S):
    B, T = next((b, t) for name, s, b, t in DC.SITE_SHAPES if name == site and s == S)
    todo = [(name, None) for name in DC.DMOL_REGIMES] if S > 1 else list(DC.SINGLE_ROWS)
    return [(name, DC.site_case(regs[name], S, B, T, first)) for name, first in todo]


@pytest.mark.parametrize("whole_chip,S", [(False, 16), (True, 8), (True, 16)], ids=["vrnn_decode-S16", "vrnn_generate-S8", "vrnn_generate-S16"])
def test_vrnn_draw_site(loaded, whole_chip, S):
    """blvm_vrnn_decode (mix_pick_from<VD_K> on registers; B = 17: a second, ragged group of rows) and blvm_vrnn_generate (the
    K_DMOLS tile; S = 8 is the padded Sp = 16 layout)."""
    import copy

    from test_gpu_generate_any_stack import draws, vrnn_model

    regs, _ = loaded
    site = "vrnn_generate" if whole_chip else "vrnn_decode"
    m = copy.deepcopy(vrnn_model(S))
    vr = m.vrnn
    _, enc_lin, dec_lin, lik = vr._plan()
    c = vr.vrnn_cell
    slope = next(l.negative_slope for l in vr.encoder if isinstance(l, torch.nn.LeakyReLU))
    for i, (name, case) in enumerate(site_cases(regs, site, S)):
        rig(dec_lin[-1], lik.params, case)
        B, T_ = case["B"], case["T"]
        eps, _, _, x0 = draws(S, B, T_, 900 + S)
        u, v = site_draws(case)
        for uu, vv in ((u, v),) + (((None, None),) if i == 0 else ()):
            x, _ = ops.vrnn_decode(enc_lin, c.kernel_params(), dec_lin, lik.params, x0, None, eps, uu, vv, S, c.h_dim, c.z_dim, c.r_dim, lik.num_mix,
                                   c.prior[6].epsilon, slope, lik.log_epsilon, whole_chip=whole_chip)  # fmt: skip
            judge_site(site, case, x, mode=uu is None)


@pytest.mark.parametrize("S", [8, 16])
def test_srnn_draw_site(loaded, S):
    import copy

    from test_gpu_generate_any_stack import draws, srnn_model

    regs, _ = loaded
    m = copy.deepcopy(srnn_model(S))
    sr = m.srnn
    _, enc_lin, dec_lin, lik = sr._plan()
    slope = next(l.negative_slope for l in sr.encoder if isinstance(l, torch.nn.LeakyReLU))
    for i, (name, case) in enumerate(site_cases(regs, "srnn_generate", S)):
        rig(dec_lin[-1], lik.params, case)
        eps, _, _, x0 = draws(S, case["B"], case["T"], 950 + S)
        u, v = site_draws(case)
        for uu, vv in ((u, v),) + (((None, None),) if i == 0 else ()):
            x, _, _ = ops.srnn_generate(enc_lin, sr.d_forward_recurrent, sr._chain_params(), dec_lin, lik.params, x0, None, None, eps, uu, vv, S,
                                        sr.h_dim, sr.z_dim, sr.r_dim, lik.num_mix, sr.prior[6].epsilon, slope, lik.log_epsilon)  # fmt: skip
            judge_site("srnn_generate", case, x, mode=uu is None)


@pytest.mark.parametrize("S", [1, 24])
def test_lstm_draw_site(loaded, S):
    from test_lstm_generate_cpu import Case, build_model

    regs, _ = loaded
    m = build_model(Case(S, 32, 1, 5, 3, "zeros", False, (70 + S, 0))).to(DEV)
    dec_last = [l for l in m.decoder if isinstance(l, torch.nn.Linear)][-1]
    for i, (name, case) in enumerate(site_cases(regs, "lstm_generate", S)):
        rig(dec_last, m.likelihood.params, case)
        u, v = site_draws(case)
        for mode in (False,) + ((True,) if i == 0 else ()):
            (x, _), _ = m.generate(n_samples=case["B"], max_timesteps=case["T"], use_mode=mode, uniforms=None if mode else (u, v), fused=True)
            judge_site("lstm_generate_any_stack", case, x[..., 0], mode=mode)


def test_stcn_draw_site(loaded):
    from test_stcn_generate_cpu import CASES, build_model, inputs

    regs, _ = loaded
    cfg = CASES["c"]._replace(B=3, T=3)
    m = build_model(cfg).to(DEV)
    eps, _ = inputs(cfg)
    S = cfg.S
    for i, (name, case) in enumerate(site_cases(regs, "stcn_generate", S)):
        rig(m.out_upsample[0], m.likelihood_module.params, case)
        u, v = site_draws(case)
        for mode in (False,) + ((True,) if i == 0 else ()):
            (x, _), _ = m.generate(n_samples=cfg.B, max_timesteps=cfg.T * S, use_mode_observations=mode, eps=eps, uniforms=None if mode else (u, v), fused=True)
            judge_site("stcn_generate", case, x.view(cfg.B, cfg.T, S), mode=mode)


def test_wavenet_draw_site(loaded):
    """No frame stack: one parameter row per launch, six launches (floor, saturation, dominated, ties, two trained rows) of B = 19
    utterances (a second, ragged group of rows) over 24 frames, dilations (1, 2), C = S = O = 32."""
    from blvm.models import WaveNet
    from blvm.modules.distributions import DiscretizedLogisticMixtureDense

    regs, _ = loaded
    torch.manual_seed(31)
    m = WaveNet(likelihood=DiscretizedLogisticMixtureDense(32, 1, num_mix=10, num_bins=2**16), n_layers=2, n_stacks=1, res_channels=32).to(DEV)
    assert m._decode_kernel_applies() and tuple(m.res_stack.dilations) == (1, 2)
    lik, rs = m.likelihood, m.res_stack
    for i, (name, case) in enumerate(site_cases(regs, "wavenet_decode", 1)):
        rig(m.out_transform.linear, lik.params, case)
        B, T_ = case["B"], case["T"]
        u, v = site_draws(case)
        x = m.generate(n_samples=B, n_frames=T_, uniforms=[(u[t, :, 0], v[t, :, 0]) for t in range(T_)], cached=True)
        judge_site("wavenet_decode", case, x.view(B, T_, 1))
        if i == 0:
            x = ops.wavenet_decode(m._one_launch_parts(), ops.DmolHead(lik.num_mix, lik.log_epsilon), B, T_, rs.res_blocks[0].inv_std,
                                   1.0 / m.variance_scale).x  # fmt: skip
            judge_site("wavenet_decode", case, x.view(B, T_, 1), mode=True)
