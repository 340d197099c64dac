"""Cases and float64 restatements for WaveNet with the Gaussian heads (tests/test_wavenet_gauss_cpu.py, tests/test_gpu_wavenet_gauss.py).

Heads, in the reference experiment's spellings: `Gaussian` = DiagonalGaussianDense(C, 1, initial_sd=1, epsilon=1e-4), `GMM-<n>` =
DiagonalGaussianMixtureDense(C, 1, num_mix=n, initial_sd=1, epsilon=1e-4).

Training: `forward_restated` is `O.wavenet_forward`'s stack with these heads (composed of `O.residual_stack_skips`, `O.gaussian_head`,
`O.gaussian_ll`, `O.gaussian_mixture_ll`); tests/golden/wavenet_gauss.npz ties it to the reference.

Generation: the shapes g16, r32, r64, g128 of tests/test_wavenet_prompt.py in its trained-like regime — the residual blocks' weights
x 2, the output transform's and the head's x 3 — with the head's raw-sd biases at -6.2, where sd = softplus_beta(raw) + 1e-4 with
beta = ln 2 is about 0.01 .. 0.05 (softplus_beta(-6.2) = 0.0195; the head's weights move raw by about +-1).  `generate_f64` is
`test_wavenet_prompt.generate_f64` with the draw of these heads (`O.gmm_sample`, or mu + sd n), unclamped.
The seeds below were chosen on the CPU so that every mixture case's smallest float64 gap between the best and the second-best
perturbed logit is >= MIN_GAP (test_wavenet_gauss_cpu.py asserts it): no Gumbel-max tie can flip a component, so every sample is
compared."""
import functools
import math

import torch
import torch.nn.functional as F

import blvm_oracle as O

from test_wavenet_prompt import SHAPES, Case, window_of

EPS = 1e-4  # the experiment's epsilon
RAW_SD_BIAS = -6.2


class Head:
    def __init__(self, name):
        self.name = name
        self.num_mix = 0 if name == "Gaussian" else int(name.split("-")[1])  # 0: the plain Gaussian
        self.F = 3 * self.num_mix if self.num_mix else 2
        # DiagonalGaussianDense: beta = ln 2 / (initial_sd - epsilon); the mixture: ln 2 / initial_sd (distributions.py:120-125, :168-171)
        self.beta = O.LN2 / (1.0 - EPS) if self.num_mix == 0 else O.LN2

    def module(self, C):
        from blvm.modules.distributions import DiagonalGaussianDense, DiagonalGaussianMixtureDense

        if self.num_mix == 0:
            return DiagonalGaussianDense(C, 1, initial_sd=1, epsilon=EPS)
        return DiagonalGaussianMixtureDense(C, 1, num_mix=self.num_mix, initial_sd=1, epsilon=EPS)


HEADS = {n: Head(n) for n in ("GMM-10", "GMM-3", "GMM-1", "Gaussian", "GMM-11")}
# (shape of test_wavenet_prompt.SHAPES, head) -> the seed of the case's parameters and draws (chosen for the no-near-ties rule)
SEEDS = {
    ("g16", "GMM-10"): 9, ("g16", "GMM-3"): 8, ("g16", "GMM-1"): 8, ("g16", "Gaussian"): 8, ("g16", "GMM-11"): 9,
    ("r32", "GMM-10"): 51, ("r32", "GMM-3"): 51, ("r32", "Gaussian"): 51,
    ("r64", "GMM-10"): 65, ("r64", "GMM-3"): 65, ("r64", "Gaussian"): 65,
    ("g128", "GMM-10"): 174, ("g128", "GMM-3"): 168, ("g128", "GMM-1"): 168, ("g128", "Gaussian"): 168,
}  # fmt: skip
# (shape, head, prompt length): P = 0 the zero start, P < rf zero pad, P == rf the exact window, P > rf trimming
ONE_LAUNCH = [
    ("g16", "GMM-10", 0), ("g16", "GMM-10", 11), ("g16", "GMM-10", 32), ("g16", "GMM-10", 40),
    ("g16", "GMM-3", 0), ("g16", "GMM-3", 11), ("g16", "GMM-1", 11), ("g16", "Gaussian", 0), ("g16", "Gaussian", 40),
    ("r32", "GMM-10", 70), ("r32", "GMM-3", 0), ("r32", "Gaussian", 70),
    ("r64", "GMM-10", 601), ("r64", "GMM-3", 0), ("r64", "Gaussian", 601),
    ("g128", "GMM-10", 9), ("g128", "GMM-3", 9), ("g128", "GMM-1", 0), ("g128", "Gaussian", 9),
]  # fmt: skip
BLOCK_BY_BLOCK = [("g16", "GMM-11", 0), ("g16", "GMM-11", 11), ("g16", "GMM-11", 40)]
ALL_CASES = ONE_LAUNCH + BLOCK_BY_BLOCK


def case_of(shape, head):
    s = SHAPES[shape]
    return Case(f"{shape}/{head}", s.B, s.C, s.layers, s.stacks, HEADS[head].num_mix, s.n_frames, SEEDS[(shape, head)])


def build_model(shape, head):
    """The case's network in the trained-like regime (CPU, fp32)."""
    from blvm.models import WaveNet

    case, hd = case_of(shape, head), HEADS[head]
    torch.manual_seed(case.seed)
    m = WaveNet(likelihood=hd.module(case.C), n_layers=case.layers, n_stacks=case.stacks, res_channels=case.C)
    assert m.receptive_field == case.rf and list(m.res_stack.dilations) == list(case.dilations)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith("weight") and k.startswith("res_stack.res_blocks"):
                p.mul_(2.0)
            elif k in ("out_transform.linear.weight", "likelihood.params.weight"):
                p.mul_(3.0)
        m.likelihood.params.bias[-max(hd.num_mix, 1) :] = RAW_SD_BIAS  # the raw sds: the last n head outputs (the last one of two)
    return m


def draws(shape, head, P, n_frames=None, offset=0):
    """-> prompt [B,P,1] uniform in [-0.8, 0.8] and n_frames draws in the form `WaveNet.generate(uniforms=)` takes: (u [B,1,n] in
    (1e-6, 1 - 1e-6), n [B,1] standard normal) for a mixture, (None, n [B,1]) for the Gaussian head."""
    case, hd = case_of(shape, head), HEADS[head]
    g = torch.Generator().manual_seed(case.seed + offset)
    n = case.n_frames if n_frames is None else n_frames
    prompt = torch.rand(case.B, max(P, 1), 1, generator=g) * 1.6 - 0.8
    uni = []
    for _ in range(n):
        u = torch.empty(case.B, 1, hd.num_mix).uniform_(1e-6, 1 - 1e-6, generator=g) if hd.num_mix else None
        uni.append((u, torch.randn(case.B, 1, generator=g)))
    return prompt[:, :P], uni


def _softplus(raw, beta):
    return O.softplus_beta64(raw, beta) if raw.dtype == torch.float64 else F.softplus(raw, beta=beta)


def head_parameters(o, sd, hd):
    """`likelihood.forward` on o [*,C] in o's dtype: (mu [*,1], sd [*,1]) for the Gaussian head (`O.gaussian_head`), (logits [*,n],
    mu [*,1,n], sd [*,1,n]) for a mixture."""
    W, b = sd["likelihood.params.weight"], sd["likelihood.params.bias"]
    if hd.num_mix == 0:
        if o.dtype == torch.float64:
            mu, raw = F.linear(o, W, b).chunk(2, dim=-1)
            return mu, O.softplus_beta64(raw, hd.beta) + EPS
        return O.gaussian_head(o, W, b, 1.0, EPS)
    p = F.linear(o, W, b)
    K = hd.num_mix
    mu, raw = p[..., K:].reshape(*p.shape[:-1], 1, 2 * K).chunk(2, dim=-1)
    return p[..., :K], mu, _softplus(raw, hd.beta) + EPS


def forward_restated(sd, x, x_sl, n_layers, n_stacks, head, n_stack_frames=1, pad_receptive_field=True):
    """`O.wavenet_forward` (pad_causal = True) with a Gaussian head in place of the DMoL one, in the dtype of `sd`."""
    hd = HEADS[head] if isinstance(head, str) else head
    dil = O.wavenet_dilations(n_layers, n_stacks, 2)
    rf = sum(dil) + 2
    y = x.detach() if pad_receptive_field else x.detach()[:, rf * n_stack_frames :]
    h = (O.stack_tensor(x, n_stack_frames)[0] if n_stack_frames > 1 else x.unsqueeze(-1)).transpose(1, 2)  # [B,C_in,T']
    if pad_receptive_field:
        skip_size = h.size(2)
        h = F.pad(h, (rf, 0))
    else:
        skip_size = h.size(2) - rf
        x_sl = x_sl - rf
    h = F.conv1d(h[..., :-1], sd["causal.conv.weight"], sd["causal.conv.bias"])
    skips = sum(O.residual_stack_skips(sd, "res_stack", h, dil, skip_size)) * math.sqrt(n_layers / n_stacks)
    out = F.relu(F.linear(F.relu(skips.transpose(1, 2)), sd["out_transform.linear.weight"], sd["out_transform.linear.bias"]))
    if n_stack_frames > 1:
        out = out.reshape(out.size(0), out.size(1) * n_stack_frames, -1)[:, : y.size(1)]
    par = head_parameters(out, sd, hd)
    if hd.num_mix == 0:
        ll = O.gaussian_ll(y, par[0].squeeze(-1), par[1].squeeze(-1), epsilon=0)
    else:
        ll = O.gaussian_mixture_ll(y.unsqueeze(-1), *par, epsilon=0).squeeze(-1)
    ll_twise = ll * O.sequence_mask(x_sl, max_len=y.size(1))
    log_prob = ll_twise.sum(1)
    loss = -log_prob.nansum() / x_sl.nansum()
    return dict(loss=loss, log_prob=log_prob, log_prob_twise=ll_twise, bpd=float((-log_prob.detach() / O.LN2).sum() / x_sl.sum()))


def generate_f64(sd, window, n_frames, n_layers, n_stacks, uniforms, head):
    """`test_wavenet_prompt.generate_f64` with a Gaussian head's draw, in the dtype of `sd`; uniforms[t] = (u or None, n); None in
    place of the list: the mode (the arg-max component's mean / the mean).  -> (x [B,n_frames,1], the smallest gap between the best
    and the second-best perturbed logit over all rows and frames; inf for one component or none)."""
    hd = HEADS[head] if isinstance(head, str) else head
    dil = O.wavenet_dilations(n_layers, n_stacks, 2)
    dt = sd["causal.conv.weight"].dtype
    assert tuple(window.shape[1:]) == (sum(dil) + 2, 1)
    x = window.to(dt).transpose(1, 2)  # [B,1,rf]
    scale = math.sqrt(n_layers / n_stacks)
    out, gap = [], float("inf")
    for t in range(n_frames):
        h = F.conv1d(x, sd["causal.conv.weight"], sd["causal.conv.bias"])
        skips = sum(O.residual_stack_skips(sd, "res_stack", h, dil, 1)) / scale  # [B,C,1]
        o = F.relu(F.linear(F.relu(skips.transpose(1, 2)), sd["out_transform.linear.weight"], sd["out_transform.linear.bias"]))
        par = head_parameters(o, sd, hd)
        if uniforms is None:
            pred = par[0] if hd.num_mix == 0 else O.mix_mode(par[0], par[1])
            if hd.num_mix > 1:
                top = par[0].topk(2, dim=-1).values
                gap = min(gap, float((top[..., 0] - top[..., 1]).min()))
        elif hd.num_mix == 0:
            pred = par[0] + par[1] * uniforms[t][1].to(dt).reshape(-1, 1, 1)
        else:
            u, n = uniforms[t][0].to(dt), uniforms[t][1].to(dt).reshape(-1, 1, 1)
            if hd.num_mix > 1:
                top = (par[0] - torch.log(-torch.log(u))).topk(2, dim=-1).values
                gap = min(gap, float((top[..., 0] - top[..., 1]).min()))
            pred = O.gmm_sample(*par, u, n)  # [B,1,1]
        out.append(pred)
        x = torch.cat([x[:, :, 1:], pred], dim=2)
    return torch.hstack(out), gap


@functools.lru_cache(maxsize=None)
def reference(shape, head, P):
    """(model on the CPU, prompt, draws, float64 samples [B,n,1], smallest gap) of a case — computed once, never changed."""
    case = case_of(shape, head)
    m = build_model(shape, head)
    prompt, uni = draws(shape, head, P)
    sd64 = {k: v.detach().double() for k, v in m.state_dict().items()}
    x64, gap = generate_f64(sd64, window_of(prompt, case.rf), case.n_frames, case.layers, case.stacks, uni, head)
    return m, prompt, uni, x64, gap


@functools.lru_cache(maxsize=None)
def mode_reference(shape, head):
    """The float64 samples of the zero start with no draws — every frame the arg-max component's mean (the mean) — and the smallest
    gap between the two largest logits."""
    case = case_of(shape, head)
    sd64 = {k: v.detach().double() for k, v in build_model(shape, head).state_dict().items()}
    return generate_f64(sd64, torch.zeros(case.B, case.rf, 1), case.n_frames, case.layers, case.stacks, None, head)
