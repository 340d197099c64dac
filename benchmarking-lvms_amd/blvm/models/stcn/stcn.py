"""Stochastic Temporal Convolutional Network with the reference's construction API, module tree and outputs
(blvm/models/stcn/stcn.py: `DiagonalGaussianDenseSTCN` :32-76, `STCN` :78-442 — `compute_loss` :247-294, `infer` :296-327,
`forward` :346-431), computed by HIP kernels: the dilated gated residual stack with per-stack skip outputs (K10), the
per-level prior / posterior MLPs (K6), the latent heads with the precision-weighted posterior and the reparameterised
sample (K8b), the per-level KL with free nats (K8), the un-dilated output stack (K10) and the DMoL head (K7).
The model has no recurrence: everything is time-parallel on time-major channel-last tensors [T,B,C].
"""
import math
import warnings
from types import SimpleNamespace
from typing import List, Optional

import torch
import torch.nn as nn

from blvm import ops
from blvm._hip import BlvmHipError
from blvm.evaluation import BitsPerDimMetric, DeferredScalars, KLMetric, LatestMeanMetric, LLMetric, LossMetric
from blvm.models import importance
from blvm.models.base_model import BaseModel
from blvm.models.vrnn import LazyNamespace
from blvm.models.wavenet.wavenet_modules import CausalConv1d, ResidualStack
from blvm.modules.convenience import AddConstant
from blvm.modules.distributions import (ConditionalDistribution, DiagonalGaussianDense, DiagonalGaussianMixtureDense,
                                        DiscretizedLogisticMixtureDense, mlp_log_prob)  # fmt: skip


class DiagonalGaussianDenseSTCN(ConditionalDistribution):
    """Two 3-layer MLPs (mean, standard deviation) + softplus_beta + epsilon (stcn.py:32-76)."""

    def __init__(self, in_channels: int, out_channels: int, hidden_channels: int, activation: nn.Module = nn.LeakyReLU,
                 init_sd_mean: float = 1, epsilon: float = 1e-3) -> None:  # fmt: skip
        super().__init__()
        if activation is not nn.LeakyReLU:
            raise NotImplementedError("libblvm_hip: DiagonalGaussianDenseSTCN is built for LeakyReLU")
        self.in_channels, self.out_channels, self.activation = in_channels, out_channels, activation
        self.init_sd_mean, self.epsilon = init_sd_mean, epsilon

        def mlp():
            return nn.Sequential(nn.Linear(in_channels, hidden_channels), activation(), nn.Linear(hidden_channels, hidden_channels),
                                 activation(), nn.Linear(hidden_channels, out_channels))  # fmt: skip

        self.transform_mu = mlp()
        self.transform_sd = mlp()
        self.sd_act = nn.Sequential(nn.Softplus(beta=math.log(2) / (init_sd_mean - epsilon)), AddConstant(epsilon))

    @property
    def softplus_beta(self) -> float:
        return math.log(2) / (self.init_sd_mean - self.epsilon)

    def raw(self, x2d: torch.Tensor):
        """(mu, pre-softplus sd) on [rows, in_channels]; the softplus is applied by the fused latent head (K8b)."""
        out = []
        for seq in (self.transform_mu, self.transform_sd):
            h = ops.mlp(x2d, [seq[0], seq[2]], ops.ACT_LEAKY, seq[1].negative_slope)
            out.append(ops.linear(h, seq[4].weight, seq[4].bias))
        return out


class PromptNeedsDeviceError(BlvmHipError, NotImplementedError):
    """A prompt handed to `STCN.generate` on a model that is not on a HIP device.  Its latents and the decode state are made by the
    HIP kernels, so on the CPU continuing a prompt stays what it was before prompts could be continued — not implemented
    (NotImplementedError) — and it is the CPU hand-off every entry point refuses (BlvmHipError)."""


class STCNDecodeState:
    """What `STCN.generate` needs to go on after `n_steps` model steps (a prompt's included): `x_window` [receptive_field,n,S], the
    last stacks time-major, and `z_window` [n_layers,n,Zin], the output stack's input (cat(z), or z[0] without `dense`) over the last
    steps — zero stacks / frames stand in front of step 0.  `scratch`: the one-launch kernel's buffer whose ring region is that
    kernel's state (None after a prompt or the step-by-step path: the rings are then primed from the windows).  A continued call
    updates the rings in place: a state is good for ONE continuation."""

    __slots__ = ("n_steps", "x_window", "z_window", "scratch")

    def __init__(self, n_steps: int, x_window, z_window, scratch=None):
        self.n_steps, self.x_window, self.z_window, self.scratch = n_steps, x_window, z_window, scratch


class STCN(BaseModel):
    def __init__(self, likelihood: str = "DMoL", in_channels: int = 1, n_layers: int = 5, n_stacks: Optional[int] = None,
                 latent_size: List[int] = [256, 128, 64, 32, 16], res_channels: int = 256, kernel_size: int = 2,
                 base_dilation: int = 2, n_stack_frames: int = 1, precision_posterior: bool = True, dense: bool = True,
                 top_down: bool = True) -> None:  # fmt: skip
        """Same arguments as the reference (stcn.py:78-123)."""
        super().__init__()
        n_latents = len(latent_size)
        n_stacks = len(latent_size) if n_stacks is None else n_stacks
        if n_stacks != n_latents:
            raise NotImplementedError("libblvm_hip: STCN is built for n_stacks == number of latent variables")
        self.likelihood, self.n_layers, self.n_stacks, self.n_latents = likelihood, n_layers, n_stacks, n_latents
        self.latent_size, self.in_channels, self.res_channels = latent_size, in_channels, res_channels
        self.kernel_size, self.base_dilation, self.n_stack_frames = kernel_size, base_dilation, n_stack_frames
        self.precision_posterior, self.dense, self.top_down = precision_posterior, dense, top_down

        # registration / RNG order of the reference (stcn.py:146-235)
        self.causal = CausalConv1d(in_channels=in_channels * n_stack_frames, out_channels=res_channels, kernel_size=kernel_size)
        self.res_stack = ResidualStack(n_layers=n_layers, n_stacks=n_stacks, res_channels=res_channels, kernel_size=kernel_size,
                                       base_dilation=base_dilation)  # fmt: skip
        self.receptive_fields = [rf + self.causal.kernel_size - 1 for rf in self.res_stack.receptive_fields]
        self.receptive_field = self.receptive_fields[-1]

        prior, posterior = [None] * n_latents, [None] * n_latents
        for i, l in enumerate(reversed(range(n_latents)) if top_down else range(n_latents)):  # (also the creation = RNG order)
            c_in = res_channels if i == 0 else res_channels + latent_size[l + 1 if top_down else l - 1]
            prior[l] = DiagonalGaussianDenseSTCN(c_in, latent_size[l], res_channels, init_sd_mean=0.5)
            posterior[l] = DiagonalGaussianDenseSTCN(c_in, latent_size[l], res_channels, init_sd_mean=0.1)
        self.prior, self.posterior = nn.ModuleList(prior), nn.ModuleList(posterior)

        self.out_transform = ResidualStack(n_layers=n_layers, n_stacks=1, res_channels=res_channels,
                                           in_channels=sum(latent_size) if dense else latent_size[0], kernel_size=kernel_size,
                                           base_dilation=1)  # fmt: skip
        self.inv_std = 1 / math.sqrt(self.n_stacks)

        num_mix = 10
        if likelihood == "DMoL":
            likelihood_module = DiscretizedLogisticMixtureDense(x_dim=2 * num_mix + num_mix, y_dim=1, num_mix=num_mix, num_bins=2**16)
        elif likelihood == "GMM":
            likelihood_module = DiagonalGaussianMixtureDense(x_dim=2 * num_mix + num_mix, y_dim=1, num_mix=num_mix, initial_sd=1,
                                                             epsilon=1e-4)  # fmt: skip
        elif likelihood == "Gaussian":
            likelihood_module = DiagonalGaussianDense(x_dim=2, y_dim=1, epsilon=1e-4)
        else:
            raise ValueError(f"Unknown likelihood type {likelihood}")
        self.out_upsample = nn.Sequential(nn.Linear(res_channels, likelihood_module.out_features * n_stack_frames), nn.ReLU())
        self.likelihood_module = likelihood_module

    # ---- inference over the latent hierarchy (stcn.py:296-327) -------------------------------------------------------
    @staticmethod
    def represent_levels(n_latents: int, top_down: bool, level: Optional[int]):
        """The levels `represent(level=...)` computes, in `infer`'s order: top-down z[l] needs levels n-1 .. l, bottom-up 0 .. l."""
        return importance.levels_upto(reversed(range(n_latents)) if top_down else range(n_latents), level)

    def infer(self, skips, eps, x_sl_dev, B: int, T: int, free_nats: float, log_ratio: bool = False, latents_to: Optional[int] = None):
        """skips[l] [T+1,B,C] time-major.  Returns per level (mu_p, sd_p, mu_q, sd_q, z) [T,B,Z_l] and the KL sums.
        `log_ratio` (`iw_bound`): the sums are those of log q(z) - log p(z) at the drawn z (K8m), for either direction.
        `latents_to` = l (`represent`): only the levels `represent_levels` names are visited, and no sums are made."""
        n, S = self.n_latents, self.n_stack_frames
        mu_p, sd_p, mu_q, sd_q, z = ([None] * n for _ in range(5))
        klds, klds_fn = [None] * n, [None] * n
        order = list(reversed(range(n))) if self.top_down else list(range(n))  # bottom-up: each latent conditions on the one below
        if latents_to is not None:
            order = self.represent_levels(n, self.top_down, latents_to)  # (a prefix of the full order)
        for i, l in enumerate(order):
            d_p, d_q = skips[l][:-1], skips[l][1:]  # prior sees frame t-1's features, the posterior frame t's (stcn.py:300-302)
            if i > 0:
                zc = z[l + 1 if self.top_down else l - 1]
                d_p, d_q = torch.cat([d_p, zc], -1), torch.cat([d_q, zc], -1)
            Z = self.latent_size[l]
            mp, sp_raw = self.prior[l].raw(d_p.reshape(T * B, -1))
            mq, sq_raw = self.posterior[l].raw(d_q.reshape(T * B, -1))
            e = eps[l].reshape(T * B, Z)
            sp, mq_c, sq_c, z_l = ops.gauss_latent(mp, sp_raw, mq, sq_raw, e, self.prior[l].softplus_beta,
                                                   self.posterior[l].softplus_beta, self.prior[l].epsilon,
                                                   ops.RSSM_PRECISION if self.precision_posterior else ops.RSSM_PLAIN)  # fmt: skip
            if latents_to is not None:
                pass  # the latents alone: no sums of either kind
            elif log_ratio:
                klds[l] = klds_fn[l] = ops.gauss_log_ratio_sums(mq_c, sq_c, mp, sp, z_l, e, x_sl_dev, ops.LAYOUT_TIME_MAJOR, B, T, Z, S)
            elif self.top_down:
                klds[l], klds_fn[l] = ops.gaussian_kl_sums(mq_c, sq_c, mp, sp, x_sl_dev, ops.LAYOUT_TIME_MAJOR, B, T, Z, S, free_nats)
            else:
                # Monte-Carlo KL at the drawn z (stcn.py:286-287, variational.py:73-83): log q(z) - log p(z) per element, masked to the
                # frame stacks that start inside the utterance, free nats shared over the level's Z dimensions; per-utterance sums.
                # (elementwise torch on [T*B, Z]: this mode is not on a BASELINE configuration and has no fused kernel)
                ll = lambda v, mu, sd: -((v - mu) ** 2) / (2 * sd**2) - sd.log() - 0.5 * math.log(2 * math.pi)  # noqa: E731
                kl = (ll(z_l, mq_c, sq_c) - ll(z_l, mp, sp)).view(T, B, Z)
                mask = (torch.arange(T, device=kl.device).unsqueeze(1) * S < x_sl_dev.unsqueeze(0)).unsqueeze(-1)
                kl_fn = torch.clamp(kl, min=free_nats / Z) if free_nats else kl
                klds[l] = (kl * mask).double().sum((0, 2))
                klds_fn[l] = (kl_fn * mask).double().sum((0, 2))
            mu_p[l], sd_p[l], mu_q[l], sd_q[l], z[l] = (t.view(T, B, Z) for t in (mp, sp, mq_c, sq_c, z_l))
        return mu_p, sd_p, mu_q, sd_q, z, klds, klds_fn

    def split_sequence(self, x, x_sl, length: int):
        raise NotImplementedError()

    def forward_split(self, x, x_sl, i_split: int, y=None, eps=None):
        """Receptive-field padding on the first split only (stcn.py:332-342); `eps` as in `forward`."""
        return self.forward(x, x_sl, y=y, pad_receptive_field=(i_split == 0), eps=eps)

    def _front(self, x, x_sl, y, pad_receptive_field: bool):
        """The deterministic front of `forward` and `iw_bound`: the target, the lengths and the encoder stacks' skip outputs ->
        (y [B,T_y], x_sl on the host, mask lengths on the device, B, T, T_y, skips[l] [T+1,B,C])."""
        if x.ndim == 3:
            x = x.squeeze(-1)
        if not x.is_cuda:
            raise BlvmHipError("blvm HIP kernels were handed a CPU tensor (no CPU fallback)")
        dev, S, rf, C = x.device, self.n_stack_frames, self.receptive_field, self.res_channels
        x = x.to(torch.float32)
        x_sl_host = x_sl.detach().cpu().to(torch.int64)
        if y is None:
            y = x.detach()
            if not pad_receptive_field:
                y = y[:, rf * S :]
        y = y.reshape(y.size(0), -1).contiguous()
        B, T_x = x.shape
        Tp = (T_x + S - 1) // S
        xs = torch.nn.functional.pad(x, (0, Tp * S - T_x)) if Tp * S != T_x else x
        xt = xs.view(B, Tp, S).transpose(0, 1).contiguous()  # time-major stacked frames [T',B,S]
        if pad_receptive_field:
            T = Tp
            xt = torch.cat([torch.zeros(rf, B, S, device=dev), xt], 0)
            if T < rf:
                warnings.warn(f"Padded input of {T} frames with a larger receptive_field={rf}.")
        else:
            T = Tp - rf
            x_sl_host = x_sl_host - S * rf
            if Tp <= rf:
                raise ValueError(f"Input must be at least as long as the receptive field if {pad_receptive_field=}")
        T_y = y.size(1)
        mask_len = ops.upload_i32(x_sl_host.clamp(min=0, max=T_y), dev)

        out = self.causal.forward_tm(xt, pad_causal=False)  # [T + rf - 1, B, C]
        n = self.n_latents
        # `d[n_latents - 1 :: n_latents]` (stcn.py:299): every n_latents-th skip connection, the first n_latents of them are
        # used — with n_layers == n_latents (the default) that is the last block of every stack
        groups = self._skip_groups()
        skips = self.res_stack.forward_tm(out, T + 1, groups=groups)
        return y, x_sl_host, mask_len, B, T, T_y, skips

    def _observe(self, z, y, mask_len, B: int, T: int, T_y: int):
        """The observation model on the latents z[l] [T,B,Z_l]: output stack, upsampling Linear and likelihood head ->
        (dec [T*B, S*F] detached, log_prob [B] float64)."""
        dev, S, C, lik = y.device, self.n_stack_frames, self.res_channels, self.likelihood_module
        logits_in = torch.cat(z, -1) if self.dense else z[0]
        ot = self.out_transform
        logits_in = torch.cat([torch.zeros(ot.receptive_field - 1, B, logits_in.size(-1), device=dev), logits_in], 0)
        skip_sum = ot.forward_tm(logits_in, T)  # [T,B,C]: sum of the output blocks' skips
        h = ops.scale_act(skip_sum.view(T * B, C), self.inv_std, 1.0)  # * inv_std (slope 1: no activation)
        up = self.out_upsample[0]
        return mlp_log_prob(lik, h, [up], ops.ACT_RELU, 0.0, y, mask_len, ops.LAYOUT_TIME_MAJOR, B, T_y, T, S)  # dec [T*B, S*F]

    def forward(self, x, x_sl, y=None, pad_receptive_field: bool = True, free_nats: float = 0, beta: float = 1,
                eps: Optional[List[torch.Tensor]] = None):  # fmt: skip
        """x [B,T] in [-1,1]; x_sl [B] (host ints).  `eps[l]` [T',B,z_l] optionally supplies the reparameterisation noise
        (otherwise drawn on the device, top level first as in the reference)."""
        y, x_sl_host, mask_len, B, T, T_y, skips = self._front(x, x_sl, y, pad_receptive_field)
        dev, S, n = y.device, self.n_stack_frames, self.n_latents
        lik = self.likelihood_module

        if eps is None:
            eps = [None] * n
            for l in (reversed(range(n)) if self.top_down else range(n)):  # the reference's draw order
                eps[l] = torch.randn(T, B, self.latent_size[l], device=dev)
        mu_p, sd_p, mu_q, sd_q, z, klds, klds_fn = self.infer(skips, [e.to(device=dev, dtype=torch.float32).contiguous() for e in eps],
                                                              mask_len, B, T, free_nats)  # fmt: skip

        dec, log_prob = self._observe(z, y, mask_len, B, T, T_y)

        kld, kld_fn = sum(klds), sum(klds_fn)
        n_frames = float(x_sl_host.sum())
        elbo = log_prob - kld
        loss = -(log_prob - beta * kld_fn).sum() / n_frames
        metrics = self.build_metrics(loss, elbo, log_prob, kld, klds, x_sl_host, beta, free_nats)

        F = lik.out_features

        def params():
            d = dec.detach().view(T, B, S, F).permute(1, 0, 2, 3).reshape(B, T * S, F)[:, :T_y]
            return lik(d.contiguous())

        bt = lambda ts: [t.transpose(0, 1) for t in ts]  # noqa: E731  (reference layout [B,T,Z])
        lazy = dict(params=params, reconstructions=lambda ns: lik.sample(ns.params), reconstructions_mode=lambda ns: lik.mode(ns.params))
        output = LazyNamespace(lazy, loss=loss, elbo=elbo, klds=klds, log_prob=log_prob, z=bt(z),
                               z_sl=[torch.ceil(x_sl_host / S).long()] * self.n_stacks, enc_mus=bt(mu_q), prior_mus=bt(mu_p),
                               y=y.unsqueeze(-1))  # fmt: skip
        return loss, metrics, output

    @torch.no_grad()
    def iw_bound(self, x, x_sl, num_samples: int, eps: Optional[List[torch.Tensor]] = None, max_rows: Optional[int] = None):
        """K-sample importance-weighted bound per utterance -> (bound [B] float64, metrics, outputs(log_w [K,B], ess, elbo_mc)).
        The deterministic encoder stacks run once on the B utterances; the latent hierarchy and the observation model run on passes
        of c * B rows (row k * B + b), c * B <= `max_rows` (default max(B, blvm_pchain_max_batch())).  `eps[l]` [K,T',B,z_l]
        optionally supplies the noise.  No free nats, no beta; always fp32 operands."""
        K = importance.check_samples(num_samples)
        with importance.fp32_operands():
            y, x_sl_host, mask_len, B, T, T_y, skips = self._front(x, x_sl, None, True)
            parts = []
            for k0, c in importance.passes(K, B, max_rows):
                n = c * B
                order = reversed(range(self.n_latents)) if self.top_down else range(self.n_latents)  # the reference's draw order
                e = [None] * self.n_latents
                for l in order:
                    e[l] = importance.pass_eps(None if eps is None else eps[l], k0, c, T, B, self.latent_size[l], y.device)
                sl, yy = mask_len.repeat(c), importance.tile_rows(y, c, 0)
                *_, z, ratios, _ = self.infer([importance.tile_rows(s, c) for s in skips], e, sl, n, T, 0, log_ratio=True)
                _, log_prob = self._observe(z, yy, sl, n, T, T_y)
                parts.append(log_prob - sum(ratios))
            return importance.finish(parts, K, B, float(x_sl_host.sum()))

    @torch.no_grad()
    def represent(self, x, x_sl, level: Optional[int] = None, num_samples: int = 1, eps: Optional[List[torch.Tensor]] = None,
                  max_rows: Optional[int] = None):  # fmt: skip
        """Latents z_l ~ q(z_l | x, z of the level visited before) of a frozen model -> (z, z_sl): per level z [T',B,z_l] fp32
        TIME-MAJOR and z_sl [B] as `forward`'s `output.z_sl[l]` — the lists over levels for `level=None`, one entry for `level=l`;
        frames t >= z_sl[b] are exactly zero.  Only what z needs runs: the encoder stacks once on the B utterances and the prior /
        posterior MLPs and latent heads of the levels `represent_levels` names (top-down n-1 .. l, bottom-up 0 .. l) — never the
        observation model (`_observe`), the KL sums, the ELBO or the metrics.  `num_samples` = K: the mean over K draws, on passes of
        c * B rows as `iw_bound` lays them (c * B <= `max_rows`), summed in particle order by K8r (`ops.particle_mean`):
        bit-identical for every `max_rows`.  `eps[l]` [T',B,z_l] ([K,T',B,z_l] for K > 1) supplies the noise, else it is drawn in
        `forward`'s order (K = 1: the same seed gives `forward`'s latents).  Receptive-field padding, as `forward`'s default.
        Operand mode: the process's current one."""
        K = importance.check_samples(num_samples)
        n, S = self.n_latents, self.n_stack_frames
        levels = self.represent_levels(n, self.top_down, level)
        y, x_sl_host, mask_len, B, T, _, skips = self._front(x, x_sl, None, True)
        z_sl = torch.ceil(x_sl_host / S).long()
        lens = ops.upload_i32(z_sl, y.device)
        outs = dict.fromkeys(levels)
        for k0, c in importance.passes(K, B, max_rows):
            e = [None] * n
            for l in levels:  # the reference's draw order
                e[l] = importance.pass_eps(None if eps is None else importance.particle_axis(eps[l], K), k0, c, T, B, self.latent_size[l],
                                           y.device)  # fmt: skip
            sl = mask_len if c == 1 else mask_len.repeat(c)
            z = self.infer([importance.tile_rows(s, c) for s in skips], e, sl, c * B, T, 0, latents_to=levels[-1])[4]
            for l in levels:
                outs[l] = importance.mean_pass(outs[l], z[l], lens, B, k0, c, K)
        if level is not None:
            return outs[level], z_sl
        return [outs[l] for l in range(n)], [z_sl] * self.n_stacks

    def build_metrics(self, loss, elbo, log_prob, kld, klds, x_sl, beta, free_nats):
        """Metric names / reductions of stcn.py:208-245."""
        n, B = self.n_latents, elbo.numel()
        sums = DeferredScalars(torch.stack([loss.detach().double(), elbo.detach().sum(), log_prob.detach().sum(), kld.detach().sum()]
                                           + [k.detach().sum() for k in klds]))  # fmt: skip
        ln2, nx = math.log(2), float(x_sl.sum())
        nz = float(torch.div(x_sl, self.n_stack_frames, rounding_mode="floor").sum())
        return [
            LossMetric(sums[0], weight_by=B),
            BitsPerDimMetric(sums[1], name="elbo (bpx)", reduce_by=nx),
            LLMetric(sums[1], name="elbo (nats)", reduce_by=B),
            LatestMeanMetric(beta, name="beta"),
            LatestMeanMetric(free_nats, name="free_nats"),
            LLMetric(sums[2], name="rec (nats)", reduce_by=B, log_to_console=False),
            BitsPerDimMetric(sums[2], name="rec (bpx)", reduce_by=nx),
            KLMetric(sums[3], name="kl (nats)", reduce_by=B, log_to_console=False),
            KLMetric(sums[3] / ln2, name="kl (bpz)", reduce_by=nz),
            *[KLMetric(sums[4 + l], name=f"kl_{l} (nats)", reduce_by=B, log_to_console=False) for l in range(n)],
            *[KLMetric(sums[4 + l] / ln2, name=f"kl_{l} (bpz)", reduce_by=nz) for l in range(n)],
            *[KLMetric(sums[4 + l] / ln2, name=f"kl_{l} (bpx)", reduce_by=nx) for l in range(n)],
        ]

    def _skip_groups(self):
        """`d[n_latents - 1 :: n_latents]` (stcn.py:299) as one entry per block: the latent level that reads its skip, or -1."""
        n, n_blocks = self.n_latents, len(self.res_stack.dilations)
        if n_blocks // n < n:
            raise IndexError(f"STCN needs n_layers * n_stacks >= n_latents**2 skip connections, got {n_blocks} for {n} latents")
        return [(i // n) if (i % n == n - 1 and i // n < n) else -1 for i in range(n_blocks)]

    def _one_launch_applies(self) -> bool:
        """The structures `blvm_stcn_generate` (K10d) takes: the DMoL head on one input channel and its width rules."""
        lik, C = self.likelihood_module, self.res_channels
        return (isinstance(lik, DiscretizedLogisticMixtureDense) and 3 * lik.num_mix <= 32 and self.in_channels == 1 and self.kernel_size == 2
                and C % 16 == 0 and all(z % 16 == 0 for z in self.latent_size) and self.n_latents <= 8
                and len(self.res_stack.dilations) <= 64 and self.n_layers <= 64)  # fmt: skip

    def _one_launch_parts(self):
        """The `weights` argument of `ops.stcn_generate` / `ops.stcn_generate_pack`."""
        rs, ot, up, lik, n = self.res_stack, self.out_transform, self.out_upsample[0], self.likelihood_module, self.n_latents
        conv1x1 = lambda c: (c.weight.view(c.out_channels, -1), c.bias)  # noqa: E731
        linears = lambda seq: [seq[0], seq[2], seq[4]]  # noqa: E731
        order = list(reversed(range(n))) if self.top_down else list(range(n))
        return ((self.causal.conv.weight, self.causal.conv.bias), conv1x1(rs.in_transform), [b.kernel_params() for b in rs.res_blocks],
                rs.dilations, self._skip_groups(), [(linears(p.transform_mu), linears(p.transform_sd)) for p in self.prior], order,
                conv1x1(ot.in_transform), [b.kernel_params() for b in ot.res_blocks], (up.weight, up.bias),
                (lik.params.weight, lik.params.bias), self.dense)  # fmt: skip

    def _one_launch_shape(self):
        """The shape arguments of `ops.stcn_ring_views` / `ops.stcn_generate_scratch` between the dilations and B."""
        n = self.n_latents
        order = list(reversed(range(n))) if self.top_down else list(range(n))
        return len(self.out_transform.res_blocks), list(self.latent_size), order, self.dense

    def _latent_pass(self, xt, eps, posterior: bool):
        """xt [T,B,S] time-major stacks from step 0 -> z per level [T,B,z_l] from ONE time-parallel pass: the posterior's draws exactly
        as `forward` makes them (the same calls on the same shapes), or each level drawn from its prior given x[<t]."""
        T, B, S = xt.shape
        dev, rf, n = xt.device, self.receptive_field, self.n_latents
        xp = torch.cat([torch.zeros(rf, B, S, device=dev), xt], 0)
        out = self.causal.forward_tm(xp, pad_causal=False)
        skips = self.res_stack.forward_tm(out, T + 1, groups=self._skip_groups())
        if posterior:
            mask_len = ops.upload_i32(torch.full((B,), T * S, dtype=torch.int64), dev)
            return self.infer(skips, eps, mask_len, B, T, 0)[4]
        z = [None] * n
        order = list(reversed(range(n))) if self.top_down else list(range(n))
        for i, l in enumerate(order):
            d = skips[l][:-1]  # the features that have seen x[<t]
            if i > 0:
                d = torch.cat([d, z[order[i - 1]]], -1)
            mp, sp_raw = self.prior[l].raw(d.reshape(T * B, -1))
            beta = self.prior[l].softplus_beta
            z[l] = ops.gauss_latent(mp, sp_raw, mp, sp_raw, eps[l].reshape(T * B, -1), beta, beta, self.prior[l].epsilon,
                                    ops.RSSM_PLAIN)[3].view(T, B, -1)  # fmt: skip
        return z

    @torch.no_grad()
    def _prime(self, x, prompt_eps=None, prompt_latents: str = "posterior"):
        """Prompt x [n,P] (P a positive multiple of S; checked by `generate`) -> (the state after its P' = P / S steps, prompt_z per level
        [n,P',z_l]).  The latents over the prompt come from one time-parallel pass (`_latent_pass`); the windows take the last
        receptive_field stacks and the last n_layers frames of the output stack's input, zero-padded on the left."""
        dev, S, rf, n = self.device, self.n_stack_frames, self.receptive_field, self.n_latents
        n_out = len(self.out_transform.res_blocks)
        f32 = dict(device=dev, dtype=torch.float32)
        x = x.to(**f32)
        B, Tp = x.size(0), x.size(1) // S
        xt = x.view(B, Tp, S).transpose(0, 1).contiguous()
        if prompt_eps is None:
            prompt_eps = [None] * n
            for l in (reversed(range(n)) if self.top_down else range(n)):  # the draw order of `forward`
                prompt_eps[l] = torch.randn(Tp, B, self.latent_size[l], **f32)
        z = self._latent_pass(xt, [e.to(**f32).contiguous() for e in prompt_eps], prompt_latents == "posterior")
        zin = torch.cat(z, -1) if self.dense else z[0]
        x_window = torch.cat([torch.zeros(rf, B, S, **f32), xt], 0)[-rf:].contiguous()
        z_window = torch.cat([torch.zeros(n_out, B, zin.size(-1), **f32), zin], 0)[-n_out:].contiguous()
        return STCNDecodeState(Tp, x_window, z_window, None), [t.transpose(0, 1) for t in z]

    @torch.no_grad()
    def _prime_rings(self, state, num_mix: int):
        """A fresh one-launch scratch buffer whose rings hold `state`: dilated block i's input over steps t0 - d_i .. t0 - 1, output
        block j's at step t0 - 1.  Step tau of block 0's input is in_transform(causal conv of the stacks tau-2, tau-1), so the window
        that fills the rings ends one stack before the newest; `ops.wavenet_prime_rings` runs the time-parallel block kernels over it."""
        rs, ot, C, S = self.res_stack, self.out_transform, self.res_channels, self.n_stack_frames
        B, t0, inv_std = state.x_window.size(1), state.n_steps, rs.res_blocks[0].inv_std
        scratch, (rings, orings) = ops.stcn_generate_scratch(rs.dilations, *self._one_launch_shape(), B, C, S, num_mix, state.x_window.device)
        feats = self.causal.forward_tm(state.x_window[:-1], pad_causal=False)  # [sum(dilations),B,C]: steps t0 - sum(dilations) .. t0 - 1
        for stack, frames, dil, views in ((rs, feats, rs.dilations, rings), (ot, state.z_window, [1] * len(ot.res_blocks), orings)):
            L, t_in = frames.size(0), stack.in_transform
            h0 = ops.linear(frames.reshape(L * B, -1), t_in.weight.view(t_in.out_channels, -1), t_in.bias).view(L, B, C)
            ops.wavenet_prime_rings(h0, [b.kernel_params() for b in stack.res_blocks], dil, inv_std, C, t0, views)
        return scratch

    def _scratch_floats(self, B: int):
        """Size of the one-launch kernel's scratch buffer at B rows, or None where the kernel does not apply."""
        if not self._one_launch_applies():
            return None
        try:
            return ops.stcn_generate_scratch_floats(self.res_stack.dilations, *self._one_launch_shape(), B, self.res_channels,
                                                    self.n_stack_frames, self.likelihood_module.num_mix)  # fmt: skip
        except BlvmHipError:
            return None

    @torch.no_grad()
    def generate(self, n_samples: int = 1, max_timesteps: int = 100, use_mode_observations: bool = False, x=None,
                 eps: Optional[List[torch.Tensor]] = None, uniforms=None, fused: Optional[bool] = None, prompt_eps=None,
                 prompt_latents: str = "posterior", state=None, return_state: bool = False):  # fmt: skip
        """Ancestral sampling from an all-zero past, from a prompt or from an earlier call's state.  The reference declares `generate`
        and leaves it unimplemented (stcn.py:435-442);
        the generative model is the one `forward` / `infer` define (stcn.py:299-326, 389-409).  One model step t gives one stack of
        S = n_stack_frames samples: the dilated stack on x[<t] gives each level its features d_t[l] (the `d_p` of `infer`), the levels
        are visited in the model's order and z_t[l] = mu + sd * eps[l][t] is drawn from prior[l](cat[d_t[l], z_t[level visited
        before]]) — the posterior is not used —, the output stack runs on cat(z_t) (`dense`) or z_t[0] with z_{t-1}, ... as its past
        (the response to `forward`'s zero padding before step 0), and x_t is drawn from the head (its mode if `use_mode_observations`:
        the arg-max component's location) and fed back.

        `max_timesteps` counts waveform samples (as `CWVAE.generate`): T' = ceil(max_timesteps / S) steps run and the output is cut.
        eps[l] [T',n,z_l] supplies the latent noise (otherwise `torch.randn` on the device in the visiting order); uniforms =
        (u [T',n,S,num_mix], v [T',n,S]) replays the DMoL sampler's draws (otherwise drawn in (1e-5, 1-1e-5) and (1e-8, 1-1e-8)).
        Returns ((x [n,max_timesteps,1], x_sl = max_timesteps per row), ns(z, prior_mus, prior_sds: per level [n,T',z_l])).

        `x` [n,P] or [n,P,1] is a prompt, P a positive multiple of S: steps P' = P / S, P' + 1, ... are drawn (x holds the generated
        samples only).  The dilated stack sees the prompt's stacks behind the zero past; the output stack needs z over the last
        n_layers prompt steps, which one time-parallel pass gives: prompt_latents="posterior" exactly the z of `forward(x, x_sl=P,
        eps=prompt_eps)`, "prior" each level from its prior given x[<t] (what free generation would have drawn).  prompt_eps[l]
        [P',n,z_l] replays those draws.  The namespace then carries `prompt_z` (per level [n,P',z_l]).  On a model that is not on a
        HIP device a prompt still raises NotImplementedError (`PromptNeedsDeviceError`, a BlvmHipError too).
        `return_state=True` adds `state` (an `STCNDecodeState`) to the namespace and `state=` continues from one — generation in
        chunks; eps and uniforms are indexed from 0 for every call, and max_timesteps must then be a multiple of S.  A continued call
        updates the state's rings in place: a state is good for ONE continuation.

        fused=None takes the one-launch kernel (`ops.stcn_generate`, K10d; from a state through its `resume=`, the rings primed
        from the state's windows when it carries none) when it applies: the DMoL head, res_channels and every
        latent size multiples of 16, within the kernel's 160 KB of LDS.  fused=True insists.  fused=False, the GMM and Gaussian heads and
        other widths run step by step on the time-parallel operators over a receptive-field window — an independent second path,
        which continues from the same state."""
        n, N, S, C, B = self.n_latents, int(max_timesteps), self.n_stack_frames, self.res_channels, int(n_samples)
        lik = self.likelihood_module
        if B < 1 or N < 1:
            raise ValueError(f"STCN.generate: n_samples and max_timesteps must be positive (got {B}, {N})")
        rf, n_out = self.receptive_field, len(self.out_transform.res_blocks)
        Zin = sum(self.latent_size) if self.dense else self.latent_size[0]
        if x is not None and state is not None:
            raise ValueError("STCN.generate: a prompt `x` and a `state` are given; a state already contains its past")
        if x is not None:
            if not torch.is_tensor(x) or x.ndim < 1 or x.size(0) != B:
                raise ValueError(f"STCN.generate: the prompt must be a tensor of n_samples = {B} rows")
            if x.ndim >= 2 and (x.size(1) < S or x.size(1) % S != 0):
                raise ValueError(f"STCN.generate: a prompt of {x.size(1)} samples is no positive multiple of n_stack_frames = {S}")
            if x.ndim not in (2, 3) or (x.ndim == 3 and x.size(2) != 1):
                raise ValueError(f"STCN.generate: the prompt must be [n,P] or [n,P,1], got {tuple(x.shape)}")
        if prompt_latents not in ("posterior", "prior"):
            raise ValueError(f"STCN.generate: prompt_latents must be 'posterior' or 'prior', got {prompt_latents!r}")
        if prompt_eps is not None:
            Pp = x.size(1) // S if x is not None else None
            if not (isinstance(prompt_eps, (tuple, list)) and len(prompt_eps) == n and all(torch.is_tensor(e) for e in prompt_eps)
                    and all(e.ndim == 3 and e.size(1) == B and e.size(2) == z and (Pp is None or e.size(0) == Pp)
                            for e, z in zip(prompt_eps, self.latent_size))):  # fmt: skip
                raise ValueError(f"STCN.generate: prompt_eps must hold one [P',{B},z_l] tensor per level, z_l = {self.latent_size}")
            if x is None:
                raise ValueError("STCN.generate: prompt_eps replays the latent draws over a prompt, and there is none (x is None)")
        if (state is not None or return_state) and N % S != 0:
            raise ValueError(f"STCN.generate: with a state, max_timesteps = {N} must be a multiple of n_stack_frames = {S}: a cut output "
                             "would lose samples between chunks")  # fmt: skip
        if state is not None:
            if not (isinstance(state, STCNDecodeState) and torch.is_tensor(state.x_window) and torch.is_tensor(state.z_window)
                    and tuple(state.x_window.shape) == (rf, B, S) and tuple(state.z_window.shape) == (n_out, B, Zin)
                    and int(state.n_steps) >= 0):  # fmt: skip
                raise ValueError(f"STCN.generate: the state does not fit this model and n_samples = {B}: it needs x_window [{rf},{B},{S}] "
                                 f"and z_window [{n_out},{B},{Zin}]")  # fmt: skip
            if state.scratch is not None and not (torch.is_tensor(state.scratch) and state.scratch.dtype == torch.float32
                                                  and state.scratch.numel() == self._scratch_floats(B)):  # fmt: skip
                raise ValueError("STCN.generate: the state's scratch buffer does not belong to this model and batch size")
        if self.in_channels != 1:
            raise NotImplementedError("STCN.generate: the likelihood heads draw one channel (in_channels must be 1)")
        Tp = (N + S - 1) // S
        if eps is not None:
            if not (isinstance(eps, (tuple, list)) and len(eps) == n
                    and all(torch.is_tensor(e) and tuple(e.shape) == (Tp, B, z) for e, z in zip(eps, self.latent_size))):  # fmt: skip
                raise ValueError(f"STCN.generate: eps must hold one [{Tp},{B},z_l] tensor per level, z_l = {self.latent_size}")
        dmol = isinstance(lik, DiscretizedLogisticMixtureDense)
        if uniforms is not None:
            if not dmol:
                raise ValueError("STCN.generate: uniforms replay the DMoL sampler's draws; this model has another head")
            K = lik.num_mix
            if not (isinstance(uniforms, (tuple, list)) and len(uniforms) == 2 and all(torch.is_tensor(t) for t in uniforms)
                    and tuple(uniforms[0].shape) == (Tp, B, S, K) and tuple(uniforms[1].shape) == (Tp, B, S)):  # fmt: skip
                raise ValueError(f"STCN.generate: uniforms must be (u [{Tp},{B},{S},{K}], v [{Tp},{B},{S}])")
        groups = self._skip_groups()
        dev = self.device
        if dev.type != "cuda":
            if x is not None:
                raise PromptNeedsDeviceError("STCN.generate: continuing a prompt is not implemented on the CPU: the latent history over the "
                                             "prompt and the decode state are made by the HIP kernels (no CPU fallback); move the model to a "
                                             "HIP device")  # fmt: skip
            raise BlvmHipError("blvm HIP kernels were handed a CPU model (no CPU fallback): move the model to a HIP device")
        f32 = dict(device=dev, dtype=torch.float32)
        order = list(reversed(range(n))) if self.top_down else list(range(n))
        if eps is None:
            eps = [None] * n
            for l in order:  # the draw order of `forward`
                eps[l] = torch.randn(Tp, B, self.latent_size[l], **f32)
        eps = [e.to(**f32).contiguous() for e in eps]
        u = v = None
        if dmol and not use_mode_observations:
            if uniforms is None:
                u = torch.empty(Tp, B, S, lik.num_mix, **f32).uniform_(1e-5, 1.0 - 1e-5)
                v = torch.empty(Tp, B, S, **f32).uniform_(1e-8, 1.0 - 1e-8)
            else:
                u, v = uniforms[0].to(**f32).contiguous(), uniforms[1].to(**f32).contiguous()
        x_sl = torch.full((B,), N, dtype=torch.int)
        extra, st = {}, state
        if x is not None:
            st, prompt_z = self._prime(x.reshape(B, -1), prompt_eps, prompt_latents)
            extra["prompt_z"] = prompt_z
        if st is not None:
            st.x_window, st.z_window = st.x_window.to(**f32).contiguous(), st.z_window.to(**f32).contiguous()
        rs, ot, up = self.res_stack, self.out_transform, self.out_upsample[0]
        bt = lambda ts: [t.transpose(0, 1) for t in ts]  # noqa: E731  (reference layout [B,T',Z])

        auto = fused is None
        if auto:
            fused = self._one_launch_applies()
        if fused:
            if not dmol:
                raise BlvmHipError("STCN.generate: the one-launch kernel is built for the DMoL head")
            try:
                p0 = self.prior[0]
                resume = None
                if st is not None:
                    # the kernel takes the phase of step `n_steps` in every ring: any t0 equal to it modulo all dilations
                    resume = (st.n_steps % math.lcm(*rs.dilations), st.x_window[-2:].transpose(0, 1).contiguous(),
                              st.scratch if st.scratch is not None else self._prime_rings(st, lik.num_mix))  # fmt: skip
                xs, z, mu, sd, scratch, _ = ops.stcn_generate(self._one_launch_parts(), B, Tp, S, rs.res_blocks[0].inv_std, self.inv_std,
                                                              p0.softplus_beta, p0.epsilon, p0.transform_mu[1].negative_slope, lik.num_mix,
                                                              lik.log_epsilon, eps, u, v, resume=resume)  # fmt: skip
                if return_state:
                    x_old = st.x_window if st is not None else torch.zeros(rf, B, S, **f32)
                    z_old = st.z_window if st is not None else torch.zeros(n_out, B, Zin, **f32)
                    z_new = torch.cat(z, -1) if self.dense else z[0]
                    extra["state"] = STCNDecodeState((st.n_steps if st is not None else 0) + Tp, torch.cat([x_old, xs.transpose(0, 1)], 0)[-rf:].contiguous(),
                                                     torch.cat([z_old, z_new], 0)[-n_out:].contiguous(), scratch)  # fmt: skip
                return ((xs.view(B, Tp * S)[:, :N].unsqueeze(-1), x_sl),
                        SimpleNamespace(z=bt(z), prior_mus=bt(mu), prior_sds=bt(sd), **extra))  # fmt: skip
            except (BlvmHipError, NotImplementedError):
                # the library validates before it launches, so nothing has run: only an EXPLICIT fused=True insists
                if not auto:
                    raise

        # Step by step: every step re-evaluates its receptive-field window with the time-parallel operators of `forward`.
        # (`forward` pads the output stack's input with at least n_out zero frames)
        xs = torch.zeros(rf + Tp, B, S, **f32)  # rf zero stacks (or the state's), then the generated ones
        zin = torch.zeros(n_out + Tp, B, Zin, **f32)  # the output stack's input behind its zero padding (or the state's past)
        if st is not None:
            xs[:rf], zin[:n_out] = st.x_window, st.z_window
        zs, mus, sds = ([torch.empty(Tp, B, z, **f32) for z in self.latent_size] for _ in range(3))
        for t in range(Tp):
            feats = self.causal.forward_tm(xs[t : t + rf], pad_causal=False)  # [rf - 1,B,C]
            skips = rs.forward_tm(feats, 1, groups=groups)  # per level [1,B,C]: the features that have seen x[<t]
            for i, l in enumerate(order):
                d = skips[l].view(B, C)
                if i > 0:
                    d = torch.cat([d, zs[order[i - 1]][t]], -1)
                mp, sp_raw = self.prior[l].raw(d)
                beta = self.prior[l].softplus_beta
                sp, _, _, z_l = ops.gauss_latent(mp, sp_raw, mp, sp_raw, eps[l][t], beta, beta, self.prior[l].epsilon, ops.RSSM_PLAIN)
                zs[l][t], mus[l][t], sds[l][t] = z_l, mp, sp
            zin[n_out + t] = torch.cat([z[t] for z in zs], -1) if self.dense else zs[0][t]
            skip_sum = ot.forward_tm(zin[t : t + n_out + 1], 1)  # [1,B,C]
            h = ops.scale_act(skip_sum.view(B, C), self.inv_std, 1.0)  # * inv_std (slope 1: no activation)
            dec = ops.linear(h, up.weight, up.bias, ops.ACT_RELU, 0.0)
            parameters = lik(dec.view(B, S, lik.out_features))
            if use_mode_observations:
                x_t = lik.mode(parameters)
            else:
                x_t = lik.sample(parameters, uniforms=(u[t], v[t])) if dmol else lik.sample(parameters)
            xs[rf + t] = x_t.reshape(B, S)
        x_out = xs[rf:].permute(1, 0, 2).reshape(B, Tp * S)[:, :N].unsqueeze(-1)
        if return_state:
            extra["state"] = STCNDecodeState((st.n_steps if st is not None else 0) + Tp, xs[-rf:].clone(), zin[-n_out:].clone(), None)
        return (x_out, x_sl), SimpleNamespace(z=bt(zs), prior_mus=bt(mus), prior_sds=bt(sds), **extra)
