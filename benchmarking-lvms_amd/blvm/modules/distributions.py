"""Distribution heads with the reference's constructor signatures and parameter names
(blvm/modules/distributions.py:105-150 DiagonalGaussianDense, :310-387 DiscretizedLogisticMixtureDense).

The modules own the parameters (`params` = nn.Linear, so state_dict keys and initialisation order match the
reference); the arithmetic runs in HIP kernels.  Inside the recurrent models the heads are consumed by the fused
sequence kernels directly and these `forward`s are not on the hot path.
"""
import math

import torch
import torch.nn as nn

from .. import ops
from .convenience import AddConstant


class ConditionalDistribution(nn.Module):
    def reset_parameters(self):
        pass


class DiagonalGaussianDense(ConditionalDistribution):
    def __init__(self, x_dim, y_dim, initial_sd: float = 1, epsilon: float = 1e-6):
        super().__init__()
        self.x_dim, self.y_dim, self.initial_sd, self.epsilon = x_dim, y_dim, initial_sd, epsilon
        self.out_features = 2 * y_dim
        self.params = nn.Linear(x_dim, 2 * y_dim)
        # kept for repr/state parity with the reference; the softplus itself is fused into the HIP epilogues
        beta = math.log(2) / (initial_sd - epsilon)
        self.sd_activation = nn.Sequential(nn.Softplus(beta=beta), AddConstant(epsilon)) if epsilon > 0 else nn.Softplus(beta=beta)
        self.reset_parameters()

    @property
    def softplus_beta(self) -> float:
        return math.log(2) / (self.initial_sd - self.epsilon)

    def mode(self, params):
        return params[0].contiguous()

    @torch.no_grad()
    def sample(self, params, noise=None):
        """mu + sd n; `noise` (standard normals of params[0]'s shape) optionally supplies n, otherwise it comes from the device RNG."""
        return params[0] + params[1] * (torch.randn_like(params[0]) if noise is None else noise.to(params[0]).reshape(params[0].shape))

    def forward(self, x: torch.Tensor):
        lead = x.shape[:-1]
        p = ops.mlp(x.reshape(-1, x.shape[-1]), [self.params], act=ops.ACT_NONE)
        mu, raw = p.view(*lead, -1).chunk(2, dim=-1)
        # softplus on a small [*, y_dim] tensor: torch element-wise (not on the fused hot path)
        return mu, self.sd_activation(raw)

    def fused_log_prob(self, dec, y, x_sl_dev, layout, B, T, Tp, S, fused_linear: bool = True):
        """Masked per-utterance log-likelihood sums [B] straight from decoder activations (K7c): the head's Linear(2->2),
        softplus and `gaussian_ll(..., epsilon=0)` (distributions.py:142-149) in one pass."""
        if self.y_dim != 1:
            raise NotImplementedError("Gaussian likelihood head: y_dim must be 1 on the audio path")
        W, b = (self.params.weight, self.params.bias) if fused_linear else (None, None)
        return ops.gauss_log_prob(dec, W, b, y, x_sl_dev, layout, B, T, Tp, S, self.softplus_beta, self.epsilon)


class DiscretizedLogisticMixtureDense(ConditionalDistribution):
    def __init__(self, x_dim: int, y_dim: int, num_mix: int = 10, num_bins: int = 256, log_epsilon: float = -7.0):
        super().__init__()
        self.x_dim, self.y_dim, self.num_mix, self.num_bins, self.log_epsilon = x_dim, y_dim, num_mix, num_bins, log_epsilon
        self.out_features = num_mix * (2 * y_dim + 1)
        self.params = nn.Linear(x_dim, self.out_features)
        self.reset_parameters()

    def forward(self, x):
        """(logits [*,K], locs [*,1,K], log_scales [*,1,K]) as the reference returns them (distributions.py:381-387)."""
        if self.y_dim != 1:
            raise NotImplementedError("DMoL head: y_dim must be 1 on the audio path")
        lead = x.shape[:-1]
        p = ops.mlp(x.reshape(-1, x.shape[-1]), [self.params], act=ops.ACT_NONE).view(*lead, -1)
        logits = p[..., : self.num_mix]
        locs, log_scales = p[..., self.num_mix :].reshape(*lead, 1, 2 * self.num_mix).chunk(2, dim=-1)
        return logits, locs, log_scales.clamp(min=self.log_epsilon)

    def fused_log_prob(self, dec, y, x_sl_dev, layout, B, T, Tp, S, fused_linear: bool = True):
        """Masked per-utterance log-likelihood sums [B] straight from decoder activations (K7)."""
        W, b = (self.params.weight, self.params.bias) if fused_linear else (None, None)
        return ops.dmol_log_prob(dec, W, b, y, x_sl_dev, layout, B, T, Tp, S, self.num_mix, self.num_bins, self.log_epsilon)

    def fused_mlp_log_prob(self, x2d, layers, act, slope, y, x_sl_dev, layout, B, T, Tp, S, given=None, dec_node=None):
        """The decoder MLP `layers` (activation after every layer) and this head on its output: (activations DETACHED, log_prob [B]).
        The head's backward hands the MLP the gradient of its last pre-activation and the head Linear's own gradients (K7 fused).
        `given`: the MLP's activations where they were computed already (`ops.mlp_given`); `dec_node`: the MLP's output where another
        node owns the MLP (`ops.DecoderFold.dec`)."""
        return ops.mlp_dmol_log_prob(x2d, layers, self.params.weight, self.params.bias, y, x_sl_dev, layout, B, T, Tp, S, act, slope,
                                     self.num_mix, self.num_bins, self.log_epsilon, given, dec_node)  # fmt: skip

    @staticmethod
    def _pack(params):
        """(logits [*,K], a [*,1,K], b [*,1,K]) -> head-output layout [*, 3K] the kernels read."""
        return torch.cat([params[0], params[1].squeeze(-2), params[2].squeeze(-2)], -1).contiguous()

    @torch.no_grad()
    def mode(self, params):
        return ops.mix_sample(self._pack(params), None, None, 0, self.log_epsilon).unsqueeze(-1)

    @torch.no_grad()
    def sample(self, params, eps: float = 1e-5, uniforms=None):
        """Gumbel-max component pick + logistic sample clamped to [-1,1] (blvm/utils/variational.py:309-349) in one kernel.
        `uniforms` = (u [*,K] in (eps, 1-eps), u2 [*,1] in (1e-8, 1-1e-8)) optionally supplies the two draws the reference
        makes, in its order; otherwise they come from the device RNG."""
        logits = params[0]
        u = torch.empty_like(logits).uniform_(eps, 1.0 - eps) if uniforms is None else uniforms[0].to(logits)
        u2 = torch.empty(*logits.shape[:-1], device=logits.device).uniform_(1e-8, 1.0 - 1e-8) if uniforms is None else uniforms[1].to(logits)
        return ops.mix_sample(self._pack(params), u, u2, 0, self.log_epsilon).unsqueeze(-1)


class DiagonalGaussianMixtureDense(ConditionalDistribution):
    """Gaussian mixture head with the reference's constructor and parameter layout (distributions.py:153-206); note the
    reference's softplus beta here is ln2 / initial_sd (epsilon is NOT subtracted, :168-171)."""

    def __init__(self, x_dim, y_dim, num_mix: int, initial_sd: float = 1, epsilon: float = 1e-6):
        super().__init__()
        self.x_dim, self.y_dim, self.num_mix, self.initial_sd, self.epsilon = x_dim, y_dim, num_mix, initial_sd, epsilon
        self.out_features = num_mix * (2 * y_dim + 1)
        self.params = nn.Linear(x_dim, self.out_features)
        beta = self.softplus_beta
        self.sd_activation = nn.Sequential(nn.Softplus(beta=beta), AddConstant(epsilon)) if epsilon > 0 else nn.Softplus(beta=beta)
        self.reset_parameters()

    @property
    def softplus_beta(self) -> float:
        return math.log(2) / self.initial_sd if self.epsilon > 0 else math.log(2) / (self.initial_sd - self.epsilon)

    def forward(self, x):
        """(logits [*,K], means [*,1,K], sds [*,1,K]) as the reference returns them (distributions.py:190-206)."""
        if self.y_dim != 1:
            raise NotImplementedError("GMM head: y_dim must be 1 on the audio path")
        lead = x.shape[:-1]
        p = ops.mlp(x.reshape(-1, x.shape[-1]), [self.params], act=ops.ACT_NONE).view(*lead, -1)
        logits = p[..., : self.num_mix]
        mu, raw = p[..., self.num_mix :].reshape(*lead, 1, 2 * self.num_mix).chunk(2, dim=-1)
        return logits, mu, self.sd_activation(raw)

    def fused_log_prob(self, dec, y, x_sl_dev, layout, B, T, Tp, S, fused_linear: bool = True):
        """Masked per-utterance log-likelihood sums [B] straight from decoder activations (K7b)."""
        W, b = (self.params.weight, self.params.bias) if fused_linear else (None, None)
        return ops.gmm_log_prob(dec, W, b, y, x_sl_dev, layout, B, T, Tp, S, self.num_mix, self.softplus_beta,
                                self.epsilon if self.epsilon > 0 else 0.0)  # fmt: skip

    @torch.no_grad()
    def mode(self, params):
        return ops.mix_sample(DiscretizedLogisticMixtureDense._pack(params), None, None, 1).unsqueeze(-1)

    @torch.no_grad()
    def sample(self, params, eps: float = 1e-6, noise=None):
        """Gumbel-max component pick + Gaussian sample (blvm/utils/variational.py:156-195) in one kernel; `noise` = (u [*,K]
        uniforms, n [*,1] standard normals) optionally supplies the reference's two draws."""
        logits = params[0]
        u = torch.empty_like(logits).uniform_(eps, 1.0 - eps) if noise is None else noise[0].to(logits)
        nrm = torch.randn(*logits.shape[:-1], device=logits.device) if noise is None else noise[1].to(logits)
        return ops.mix_sample(DiscretizedLogisticMixtureDense._pack(params), u, nrm, 1, sd_beta=0.0).unsqueeze(-1)


class CategoricalDense(ConditionalDistribution):
    """Softmax over `y_dim` classes with the reference's constructor and parameter names (distributions.py:207-235: `logits` =
    nn.Linear, so its state_dict loads unchanged).  Training goes through `fused_log_prob` (K7d: the [frames, y_dim] logits are never
    stored); `forward` materialises logits for the few rows generation and the lazy outputs ask for."""

    def __init__(self, x_dim, y_dim):
        super().__init__()
        ops.categorical_check_widths(x_dim, y_dim)
        self.x_dim, self.y_dim = x_dim, y_dim
        self.out_features = y_dim
        self.logits = nn.Linear(x_dim, y_dim)
        # the class values, computed where `Quantize` computes its boundaries (on the host) so that the two agree to the bit; not
        # part of the state_dict
        self.register_buffer("levels", torch.linspace(-1.0, 1.0, y_dim), persistent=False)
        self.reset_parameters()

    def forward(self, x):
        lead = x.shape[:-1]
        return ops.mlp(x.reshape(-1, x.shape[-1]), [self.logits], act=ops.ACT_NONE).view(*lead, -1)

    def fused_log_prob(self, dec, y, x_sl_dev, B, T, Tp, S):
        """Masked per-utterance log-likelihood sums [B] (float64) of integer targets y [B,T] straight from the activations `dec`
        [B*T', S*x_dim] (time-major rows)."""
        return ops.categorical_log_prob(dec, self.logits.weight, self.logits.bias, y, x_sl_dev, B, T, Tp, S)

    def log_prob(self, y, logits, reduce_dim=None):
        """`categorical_ll(y, logits, reduce_dim)` (log_likelihoods.py:63-80) per frame on materialised logits — a handful of rows,
        element-wise torch off the hot path (training uses `fused_log_prob`)."""
        ll = (logits - logits.logsumexp(dim=-1, keepdim=True)).gather(-1, y.long().unsqueeze(-1)).squeeze(-1)
        return ll if reduce_dim is None else ll.sum(reduce_dim)

    @torch.no_grad()
    def mode(self, logits):
        return ops.categorical_sample(logits)

    @torch.no_grad()
    def sample(self, logits, uniforms=None):
        """Inverse-CDF draw, one uniform per row (`uniforms` [*] in [0,1) optionally supplies them)."""
        u = torch.rand(logits.shape[:-1], device=logits.device) if uniforms is None else uniforms
        return ops.categorical_sample(logits, u)

    def dequantize(self, k):
        """Class k -> linspace(-1, 1, y_dim)[k]: the value `Quantize(bins=y_dim)` maps back to class k."""
        return self.levels.to(k.device)[k.long()]


def gauss_rollout_head(lik):
    """The head the one-launch VRNN / SRNN roll-outs draw for a Gaussian likelihood (`ops.GmmHead`, `ops.GaussHead`); None for any
    other module (the DMoL head is those roll-outs' default and needs none)."""
    if isinstance(lik, DiagonalGaussianMixtureDense) and lik.y_dim == 1:
        return ops.GmmHead(lik.num_mix, lik.softplus_beta, lik.epsilon if lik.epsilon > 0 else 0.0)
    if isinstance(lik, DiagonalGaussianDense) and lik.y_dim == 1:
        return ops.GaussHead(lik.softplus_beta, lik.epsilon if lik.epsilon > 0 else 0.0)
    return None


def gauss_rollout_noise(head, T, B, S, Z, device, want_eps=True, want_draws=True):
    """The device noise of a T-step roll-out with a Gaussian head, drawn in the reference's order and ranges — per step randn(B, Z)
    for the prior, then (GMM) uniform(1e-6, 1 - 1e-6) over [B,S,K] for the component pick, then randn(B, S, 1) — so that a seeded
    call draws the same numbers whichever path replays them.  -> (eps [T,B,Z], u [T,B,S,K] or None, n [T,B,S]); a part that is not
    wanted is not drawn and None."""
    K = head.num_mix if isinstance(head, ops.GmmHead) else 0
    eps, u, n = [], [], []
    for _ in range(T):
        if want_eps:
            eps.append(torch.randn(B, Z, device=device))
        if want_draws:
            if K:
                u.append(torch.empty(B, S, K, device=device).uniform_(1e-6, 1.0 - 1e-6))
            n.append(torch.randn(B, S, 1, device=device))
    stack = lambda ts: torch.stack(ts) if ts else None  # noqa: E731
    n = stack(n)
    return stack(eps), stack(u), None if n is None else n.squeeze(-1)


def gauss_rollout_draws(head, uniforms, T, B, S, device):
    """A caller's `uniforms` = (u [T,B,S,K] or None, n [T,B,S]) for a Gaussian head -> (u, n) float32 on `device` in those shapes."""
    K = head.num_mix if isinstance(head, ops.GmmHead) else 0
    u, n = uniforms
    if (u is None) != (K == 0):
        raise ValueError("uniforms: (u [T,B,S,K], n [T,B,S]) for the GMM head, (None, n [T,B,S]) for the Gaussian head")
    u = None if u is None else torch.as_tensor(u)[:T].reshape(T, B, S, K).to(device, torch.float32).contiguous()
    return u, torch.as_tensor(n)[:T].reshape(T, B, S).to(device, torch.float32).contiguous()


def gauss_head_sample(lik, head, parameters, u_t, n_t):
    """One step of the step-by-step path with given draws: lik.sample with u_t [B,S,K] (GMM) and n_t [B,S] handed over as `noise=`."""
    if isinstance(head, ops.GmmHead):
        return lik.sample(parameters, noise=(u_t, n_t))
    return lik.sample(parameters, noise=n_t.unsqueeze(-1))


def mlp_log_prob(lik, x2d, layers, act, slope, y, x_sl_dev, layout, B, T, Tp, S, given=None, dec_node=None):
    """Decoder MLP + likelihood head `lik` on its output: (decoder activations DETACHED, masked per-utterance log-likelihood sums [B]).
    The DMoL head takes its fused form; the Gaussian heads run the MLP and `fused_log_prob` as separate nodes.
    `given`: the MLP's activations, one tensor per layer, where they were computed already (the VRNN forward launch)."""
    if isinstance(lik, DiscretizedLogisticMixtureDense):
        return lik.fused_mlp_log_prob(x2d, layers, act, slope, y, x_sl_dev, layout, B, T, Tp, S, given, dec_node)
    if dec_node is not None:
        raise ops._hip.BlvmHipError("mlp_log_prob: only the fused DMoL head takes a decoder output with head gates")
    dec = ops.mlp(x2d, layers, act, slope) if given is None else ops.mlp_given(x2d, layers, given, act, slope)
    return dec.detach(), lik.fused_log_prob(dec, y, x_sl_dev, layout, B, T, Tp, S)
