"""VRNN [Chung et al. 2015] with the reference's construction API and state_dict layout, computed by HIP kernels.

Reference: blvm/models/vrnn.py — `VRNNCell` :36-164, `VRNN` :167-434 (`compute_elbo` :255-279, `forward` :281-369),
`VRNNAudio` :437-545.  The modules below own the parameters in the same registration order (so seeded
initialisation and checkpoints are interchangeable with the reference) while `forward` hands whole sequences to
`libblvm_hip.so`: encoder/decoder MLPs (K6), the recurrent cell over all steps incl. BPTT (K1), the Gaussian KL with
free nats (K8, its backward fused into K1) and the DMoL head (K7).
"""
import math
from types import SimpleNamespace
from typing import Optional, Union

import torch
import torch.nn as nn
import torch.nn.init as init

from blvm import _hip, ops
from blvm.data.transforms import StackTensor
from blvm.evaluation import BitsPerDimMetric, DeferredScalars, KLMetric, LatestMeanMetric, LLMetric, LossMetric
from blvm.models import importance
from blvm.models.base_model import BaseModel
from blvm.modules.convenience import View
from blvm.modules.distributions import (DiagonalGaussianDense, DiagonalGaussianMixtureDense, DiscretizedLogisticMixtureDense,
                                        gauss_head_sample, gauss_rollout_draws, gauss_rollout_head, gauss_rollout_noise,
                                        mlp_log_prob)  # fmt: skip

LIKELIHOOD_HEADS = (DiscretizedLogisticMixtureDense, DiagonalGaussianMixtureDense, DiagonalGaussianDense)


class LazyNamespace(SimpleNamespace):
    """SimpleNamespace whose expensive fields are computed on first access (the reference computes samples / modes /
    masks on every forward although the loss never uses them, vrnn.py:332-333).  A lazy callable that needs other fields
    takes the namespace as its argument (`lambda ns: ...`) instead of closing over it: a closure would make a reference cycle
    namespace -> dict -> lambda -> namespace that keeps the step's activations alive until the cyclic garbage collector runs."""

    def __init__(self, _lazy=None, **kwargs):
        super().__init__(**kwargs)
        object.__setattr__(self, "_lazy", dict(_lazy or {}))

    def __getattr__(self, name):
        lazy = object.__getattribute__(self, "_lazy")
        if name in lazy:
            fn = lazy.pop(name)
            value = fn(self) if fn.__code__.co_argcount else fn()
            setattr(self, name, value)
            return value
        raise AttributeError(name)


class VRNNCell(nn.Module):
    def __init__(self, x_dim: int, h_dim: int, z_dim: int, r_dim: Optional[int] = None, condition_h_on_x: bool = True,
                 residual_posterior: bool = False):  # fmt: skip
        super().__init__()
        r_dim = r_dim if r_dim else 2 * h_dim
        self.x_dim, self.h_dim, self.z_dim, self.r_dim = x_dim, h_dim, z_dim, r_dim
        self.condition_h_on_x = condition_h_on_x
        self.residual_posterior = residual_posterior

        def mlp(i, n):
            layers = []
            for k in range(n):
                layers += [nn.Linear(i if k == 0 else h_dim, h_dim), nn.ReLU()]
            return layers

        # registration (and therefore RNG) order as in the reference: phi_z, prior, posterior, gru_cell (vrnn.py:63-94)
        self.phi_z = nn.Sequential(*mlp(z_dim, 4))
        self.prior = nn.Sequential(*mlp(r_dim, 3), DiagonalGaussianDense(h_dim, z_dim))
        self.posterior = nn.Sequential(*mlp(x_dim + r_dim, 3), DiagonalGaussianDense(h_dim, z_dim))
        self.gru_cell = nn.GRUCell(x_dim + h_dim if condition_h_on_x else h_dim, r_dim)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        init.orthogonal_(self.gru_cell.weight_hh)

    def get_initial_state(self, batch_size: int, device=None):
        device = device if device is not None else self.prior[0].weight.device
        return torch.zeros(batch_size, self.r_dim, device=device)

    def kernel_params(self):
        """Parameters in the order of `ops._VRNN_PARAM_ORDER` / struct BlvmVrnnWeights."""
        p, q, f, g = self.prior, self.posterior, self.phi_z, self.gru_cell
        out = []
        for seq in (p, q):
            for i in (0, 2, 4):
                out += [seq[i].weight, seq[i].bias]
            out += [seq[6].params.weight, seq[6].params.bias]
        for i in (0, 2, 4, 6):
            out += [f[i].weight, f[i].bias]
        out += [g.weight_ih, g.weight_hh, g.bias_ih, g.bias_hh]
        return out

    def sequence(self, enc, h0, eps, x_sl_dev, stride: int, free_nats: float = 0.0, generate: bool = False, decoder=None):
        """`generate=True`: z is drawn from the prior instead of the posterior (`VRNNCell.generate`, vrnn.py:143-164).
        `decoder`: an `ops.DecoderFold` (see `ops.vrnn_sequence`)."""
        if not self.condition_h_on_x:
            raise NotImplementedError("libblvm_hip: VRNN cell kernels implement condition_h_on_x=True (the VRNNAudio form)")
        head = self.prior[6]
        if head.initial_sd != 1 or self.posterior[6].epsilon != head.epsilon:
            raise NotImplementedError("libblvm_hip: Gaussian heads with initial_sd != 1 are not supported")
        mode = 3 if generate else int(self.residual_posterior)
        return ops.vrnn_sequence(enc, h0, eps, x_sl_dev, self.kernel_params(), self.x_dim, self.h_dim, self.z_dim,
                                 self.r_dim, mode, stride, free_nats, head.epsilon, decoder=decoder)  # fmt: skip

    @torch.no_grad()
    def generate(self, x: torch.Tensor, h: torch.Tensor, use_mode: bool = False, eps: Optional[torch.Tensor] = None):
        """One step of ancestral sampling (vrnn.py:143-164) as a length-1 sequence in prior-sampling mode."""
        B = x.size(0)
        if eps is None:
            eps = torch.zeros(B, self.z_dim, device=x.device) if use_mode else torch.randn(B, self.z_dim, device=x.device)
        x_sl = torch.ones(B, dtype=torch.int32, device=x.device)
        decin, _, _, _, _, mu_p, sd_p, z = self.sequence(x.unsqueeze(0).contiguous(), h, eps.view(1, B, self.z_dim).contiguous(),
                                                         x_sl, 1, 0.0, generate=True)  # fmt: skip
        h_new = decin[1, :, self.h_dim :]
        out = SimpleNamespace(h=h_new, z=z[0], enc_mu=mu_p[0], enc_sd=sd_p[0], prior_mu=mu_p[0], prior_sd=sd_p[0],
                              phi_z=decin[0, :, : self.h_dim])  # fmt: skip
        return h_new, out

    def forward(self, x: torch.Tensor, h: torch.Tensor, eps: Optional[torch.Tensor] = None):
        """Single step (vrnn.py:109-141): a length-1 sequence through the same kernels."""
        B = x.size(0)
        eps = torch.randn(1, B, self.z_dim, device=x.device) if eps is None else eps.view(1, B, self.z_dim)
        x_sl = torch.ones(B, dtype=torch.int32, device=x.device)
        decin, _, _, mu_q, sd_q, mu_p, sd_p, z = self.sequence(x.unsqueeze(0).contiguous(), h, eps, x_sl, 1, 0.0)
        h_new = decin[1, :, self.h_dim :]
        out = SimpleNamespace(h=h_new, z=z[0], enc_mu=mu_q[0], enc_sd=sd_q[0], prior_mu=mu_p[0], prior_sd=sd_p[0],
                              phi_z=decin[0, :, : self.h_dim])  # fmt: skip
        return h_new, out


def _linears(seq: nn.Sequential):
    return [m for m in seq if isinstance(m, nn.Linear)]


class VRNN(nn.Module):
    def __init__(self, encoder: nn.Module, likelihood: nn.Module, x_dim: int, h_dim: int, z_dim: int,
                 r_dim: Optional[int] = None, decoder: nn.Module = None, residual_posterior: bool = False,
                 condition_h_on_x: bool = True, condition_x_on_h: bool = True, dropout: float = 0):  # fmt: skip
        super().__init__()
        r_dim = r_dim if r_dim else 2 * h_dim
        self.x_dim, self.h_dim, self.z_dim, self.r_dim = x_dim, h_dim, z_dim, r_dim
        self.residual_posterior = residual_posterior
        self.condition_h_on_x = condition_h_on_x
        self.condition_x_on_h = condition_x_on_h
        if dropout:
            raise NotImplementedError("libblvm_hip: dropout is not on the benchmark path (all runs use dropout 0)")

        self.encoder = encoder
        self.likelihood = likelihood
        if decoder is None:
            d_in = h_dim + r_dim if condition_x_on_h else h_dim
            self.decoder = nn.Sequential(nn.Linear(d_in, h_dim), nn.ReLU(), nn.Linear(h_dim, h_dim), nn.ReLU(),
                                         nn.Linear(h_dim, h_dim), nn.ReLU())  # fmt: skip
        else:
            self.decoder = decoder
        self.vrnn_cell = VRNNCell(x_dim=x_dim, h_dim=h_dim, z_dim=z_dim, condition_h_on_x=condition_h_on_x,
                                  residual_posterior=residual_posterior)  # fmt: skip
        self.dropout = None

    # ---- structure recognised by the fused path --------------------------------------------------------------------
    def _plan(self):
        enc, dec, lik = self.encoder, self.decoder, self.likelihood
        stack = next((m for m in enc if isinstance(m, StackTensor)), None) if isinstance(enc, nn.Sequential) else None
        ok = (
            stack is not None
            and isinstance(dec, nn.Sequential)
            and isinstance(lik, LIKELIHOOD_HEADS)
            and self.condition_h_on_x
            and self.condition_x_on_h
            and all(isinstance(m, (nn.Linear, nn.LeakyReLU, View, StackTensor)) for m in list(enc) + list(dec))
            and isinstance(dec[-2], nn.LeakyReLU)
        )
        if not ok:
            raise NotImplementedError(
                "libblvm_hip accelerates the VRNNAudio(likelihood='DMoL') structure (stacked-frame MLP encoder, MLP "
                "decoder, DMoL head, condition_h_on_x = condition_x_on_h = True); other compositions are not built yet"
            )
        return stack.n_frames, _linears(enc), _linears(dec), lik

    def _encode(self, x, x_sl, S, enc_lin):
        """The deterministic front of `forward` and `iw_bound`: (y [B,T] fp32, x_sl on the host, x_sl on the device, T', stride,
        enc [T',B,X])."""
        if x.ndim == 3:
            x = x.squeeze(-1)
        dev = x.device
        B, T = x.shape
        x_sl_host = x_sl.detach().cpu().to(torch.int64)
        x_sl_dev = ops.upload_i32(x_sl_host, dev)
        y = x.detach().to(torch.float32).contiguous()
        Tp = (T + S - 1) // S
        stride = math.ceil(T / Tp)

        # frames stacked time-major: [T', B, S]   (StackTensor, operations.py:14-32: right zero-pad)
        xs = torch.nn.functional.pad(y, (0, Tp * S - T)) if Tp * S != T else y
        xs = xs.view(B, Tp, S).transpose(0, 1).contiguous().view(Tp * B, S)
        enc = ops.mlp(xs, enc_lin, ops.ACT_LEAKY, ops.LEAKY_SLOPE).view(Tp, B, -1)
        return y, x_sl_host, x_sl_dev, Tp, stride, enc

    def _decoder_fold(self, dec_lin, lik):
        """The decoder handed down with the cell where it is three chained Linear + LeakyReLU (else None: it runs as K6)."""
        H, R = self.h_dim, self.r_dim
        widths = [(lin.in_features, lin.out_features) for lin in dec_lin]
        chained = len(dec_lin) == 3 and widths[0] == (H + R, widths[1][0]) and widths[1][1] == widths[1][0] == widths[2][0]
        # (head_gates: the DMoL head below returns the gradient of the decoder's last pre-activation, so the cell's node may take the
        # decoder in and run its backward on the backward launch's spare workgroups: `fold.dec`)
        gates = isinstance(lik, DiscretizedLogisticMixtureDense) and lik.params is not None
        return ops.DecoderFold(dec_lin, ops.LEAKY_SLOPE, gates) if chained and all(lin.bias is not None for lin in dec_lin) else None

    def forward(self, x: torch.Tensor, x_sl: torch.Tensor, beta: float = 1, free_nats: float = 0,
                h0: Optional[torch.Tensor] = None, eps: Optional[torch.Tensor] = None):  # fmt: skip
        """x [B,T] or [B,T,1] in [-1,1]; x_sl [B] lengths (host int tensor, as the reference's loaders give it).
        `eps` [T',B,z] optionally supplies the reparameterisation noise (otherwise drawn on the device)."""
        S, enc_lin, dec_lin, lik = self._plan()
        y, x_sl_host, x_sl_dev, Tp, stride, enc = self._encode(x, x_sl, S, enc_lin)
        dev = y.device
        B, T = y.shape
        H, Z, R = self.h_dim, self.z_dim, self.r_dim

        if eps is None:
            eps = torch.randn(Tp, B, Z, device=dev, dtype=torch.float32)
        # a decoder of three Linear + LeakyReLU goes down with the cell: the forward launch runs it on its spare workgroups where it
        # has them (`given`: its activations; None: not folded, the decoder runs as K6 below)
        fold = self._decoder_fold(dec_lin, lik)
        decin, kld, kld_fn, mu_q, sd_q, mu_p, sd_p, z = self.vrnn_cell.sequence(enc, h0, eps, x_sl_dev, stride, free_nats, decoder=fold)
        given, dec_node = (fold.given, fold.dec) if fold is not None else (None, None)

        # decoder MLP (K6, or its node alone) + likelihood head (K7 / K7b / K7c); dec [T'*B, S*F] detached
        dec, log_prob = mlp_log_prob(lik, decin[:Tp].view(Tp * B, H + R), dec_lin, ops.ACT_LEAKY, ops.LEAKY_SLOPE, y, x_sl_dev,
                                     ops.LAYOUT_TIME_MAJOR, B, T, Tp, S, given=given, dec_node=dec_node)  # fmt: skip

        # ELBO assembly in float64 as the reference does (mask dtype `float`, vrnn.py:266-279), one kernel:
        # elbo = log_prob - kld, loss = -(log_prob - beta * kld_fn).sum() / n_frames
        n_frames = float(x_sl_host.sum())
        loss, elbo, sums4 = ops.elbo_assemble(log_prob, kld, kld_fn, beta, n_frames)
        kl = kld_fn  # the reference returns the free-nats-clamped KL as `kl` (vrnn.py:275-279); == kld when free_nats is 0

        sums = DeferredScalars(sums4)  # (loss, elbo.sum(), log_prob.sum(), kl.sum())
        ln2 = math.log(2)
        metrics = [
            LossMetric(sums[0], weight_by=B),
            LLMetric(sums[1], name="elbo", reduce_by=B),
            LLMetric(sums[2], name="rec", reduce_by=B),
            KLMetric(sums[3], reduce_by=B),
            KLMetric(sums[3] / ln2, name="kl (bpt)", reduce_by=n_frames),
            BitsPerDimMetric(sums[1], reduce_by=n_frames),
            LatestMeanMetric(beta, name="beta"),
            LatestMeanMetric(free_nats, name="free_nats"),
        ]

        max_len = int(x_sl_host.max())
        F = lik.out_features

        def parameters():
            d = dec.detach().view(Tp, B, S, F).permute(1, 0, 2, 3).reshape(B, Tp * S, F)[:, :max_len]
            return lik(d.contiguous())

        lazy = dict(
            reconstructions_parameters=parameters,
            reconstructions=lambda ns: lik.sample(ns.reconstructions_parameters),
            reconstructions_mode=lambda ns: lik.mode(ns.reconstructions_parameters),
            seq_mask=lambda: (torch.arange(max_len, device=dev).unsqueeze(0) < x_sl_dev.unsqueeze(1)).to(torch.float64),
        )
        outputs = LazyNamespace(
            lazy,
            elbo=elbo,
            log_prob=log_prob,
            kl=kl,
            y=y.unsqueeze(-1),
            z=z.transpose(0, 1),
            z_sl=(x_sl_host / stride).ceil().int(),
            h_n=decin[Tp - 1, :, H:],  # all_h[-1] after the pop at vrnn.py:310-311: the state ENTERING the last step
        )
        return loss, metrics, outputs

    @torch.no_grad()
    def iw_bound(self, x: torch.Tensor, x_sl: torch.Tensor, num_samples: int, eps: Optional[torch.Tensor] = None,
                 max_rows: Optional[int] = None):  # fmt: skip
        """K-sample importance-weighted bound per utterance -> (bound [B] float64, metrics, outputs(log_w [K,B], ess, elbo_mc)).
        The encoder runs once on the B utterances; the cell, the decoder and the head run on passes of c * B rows (row k * B + b),
        c * B <= `max_rows` (default max(B, blvm_pchain_max_batch())).  `eps` [K,T',B,z] optionally supplies the noise.  No free
        nats, no beta; always fp32 operands."""
        K = importance.check_samples(num_samples)
        S, enc_lin, dec_lin, lik = self._plan()
        H, Z, R = self.h_dim, self.z_dim, self.r_dim
        with importance.fp32_operands():
            y, x_sl_host, x_sl_dev, Tp, stride, enc = self._encode(x, x_sl, S, enc_lin)
            B, T = y.shape
            parts = []
            for k0, c in importance.passes(K, B, max_rows):
                n = c * B
                e = importance.pass_eps(eps, k0, c, Tp, B, Z, y.device)
                sl, yy = x_sl_dev.repeat(c), importance.tile_rows(y, c, 0)
                fold = self._decoder_fold(dec_lin, lik)
                decin, _, _, mu_q, sd_q, mu_p, sd_p, z = self.vrnn_cell.sequence(importance.tile_rows(enc, c), None, e, sl, stride, 0.0,
                                                                                 decoder=fold)  # fmt: skip
                given, dec_node = (fold.given, fold.dec) if fold is not None else (None, None)
                _, log_prob = mlp_log_prob(lik, decin[:Tp].view(Tp * n, H + R), dec_lin, ops.ACT_LEAKY, ops.LEAKY_SLOPE, yy, sl,
                                           ops.LAYOUT_TIME_MAJOR, n, T, Tp, S, given=given, dec_node=dec_node)  # fmt: skip
                ratio = ops.gauss_log_ratio_sums(mu_q, sd_q, mu_p, sd_p, z, e, sl, ops.LAYOUT_TIME_MAJOR, n, Tp, Z, stride)
                parts.append(log_prob - ratio)
            return importance.finish(parts, K, B, float(x_sl_host.sum()))

    @torch.no_grad()
    def represent(self, x: torch.Tensor, x_sl: torch.Tensor, level: Optional[int] = None, num_samples: int = 1,
                  eps: Optional[torch.Tensor] = None, max_rows: Optional[int] = None):  # fmt: skip
        """Latents z ~ q(z | x) of a frozen model -> (z [T',B,z] fp32 TIME-MAJOR, z_sl [B] as `forward`'s `output.z_sl`); frames
        t >= z_sl[b] are exactly zero.  Only what z needs runs: the encoder once on the B utterances and the cell (no decoder, in the
        cell's launch or after it, no head, no KL sums, no ELBO, no metrics).  `num_samples` = K: the mean over K draws, the particles
        on passes of c * B rows as `iw_bound` lays them (c * B <= `max_rows`), summed in particle order by K8r
        (`ops.particle_mean`): bit-identical for every `max_rows`.  `eps` [T',B,z] ([K,T',B,z] for K > 1) supplies the noise, else
        it is drawn as `forward` draws it (K = 1: the same seed gives `forward`'s latents).  `level`: None or 0.  Operand mode: the
        process's current one."""
        K = importance.check_samples(num_samples)
        importance.levels_upto([0], level)
        S, enc_lin, _, _ = self._plan()
        y, x_sl_host, x_sl_dev, Tp, stride, enc = self._encode(x, x_sl, S, enc_lin)
        B, Z = y.shape[0], self.z_dim
        z_sl = (x_sl_host / stride).ceil().int()
        lens = ops.upload_i32(z_sl, y.device)
        eps, out = importance.particle_axis(eps, K), None
        for k0, c in importance.passes(K, B, max_rows):
            e = importance.pass_eps(eps, k0, c, Tp, B, Z, y.device)
            sl = x_sl_dev if c == 1 else x_sl_dev.repeat(c)
            z = self.vrnn_cell.sequence(importance.tile_rows(enc, c), None, e, sl, stride, 0.0, decoder=None)[7]
            out = importance.mean_pass(out, z, lens, B, k0, c, K)
        return out, z_sl

    @torch.no_grad()
    def generate(self, x: torch.Tensor, h0: Optional[torch.Tensor] = None, n_samples: int = 1, max_timesteps: int = 100,
                 stop_value: float = None, use_mode: bool = False, eps: Optional[torch.Tensor] = None, uniforms=None,
                 fused: Optional[bool] = None):  # fmt: skip
        """Autoregressive sampling (vrnn.py:371-434): the previous frame stack is encoded, the cell draws z from its prior and
        updates h, the decoder (on cat[phi_z, h_new] — the UPDATED state here, unlike `forward`) parameterises the next frame
        stack, which is sampled (or its mode taken) and fed back.  x [B,S,1] initial frame stack; returns ((x [B,1+T,S], x_sl), ns).
        `eps` [T,B,z] optionally supplies the prior noise, `uniforms` = (u [T,B,S,K], v [T,B,S]) the sampler's draws.  Every step
        runs the K6 / K1 / K7-head kernels at T' = 1; `fused=True` (DMoL head, no stop value) runs ALL steps in one launch (K1c);
        the default (None) takes the one-launch path whenever the model has that structure: hidden, latent and recurrent sizes in
        multiples of 16, 10 mixture components, any frame-stack size S >= 1 (up to blvm_pchain_max_batch() utterances; beyond that
        the per-CU form, which needs S % 16 == 0, or else the step-by-step path).
        The GMM and Gaussian heads take the same paths under the same rules (`_generate_gauss`; the Gaussian head has no per-CU
        form); their `uniforms` = (u [T,B,S,K] in (1e-6, 1-1e-6), n [T,B,S] standard normals), u = None for the Gaussian head."""
        S, enc_lin, dec_lin, lik = self._plan()
        head = gauss_rollout_head(lik)
        if head is not None:
            return self._generate_gauss(head, x, h0, n_samples, max_timesteps, stop_value, use_mode, eps, uniforms, fused)
        auto = fused is None
        if auto:
            c = self.vrnn_cell
            fused = (stop_value is None and max_timesteps > 0 and isinstance(lik, DiscretizedLogisticMixtureDense) and len(enc_lin) == 3
                     and len(dec_lin) == 3 and all(v % 16 == 0 for v in (c.h_dim, c.z_dim, c.r_dim)))  # fmt: skip
        if fused:
            try:
                return self._generate_fused(x, h0, n_samples, max_timesteps, stop_value, use_mode, eps, uniforms)
            except _hip.BlvmHipError:
                # the one-launch kernels have limits of their own beyond the structure test above (batch above the persistent
                # path's and shapes K1c's LDS plan does not take): only an EXPLICIT fused=True insists, the default serves every
                # shape the step-by-step path serves.  Nothing has run yet: the library validates before it launches.
                if not auto:
                    raise
        if x.size(0) > 1:
            assert x.size(0) == n_samples
        else:
            x = x.repeat(n_samples, *[1] * (x.ndim - 1))
        dev = x.device
        H = self.h_dim
        all_x = [x]
        x_sl = torch.ones(n_samples, dtype=torch.int)
        h = self.vrnn_cell.get_initial_state(n_samples, dev) if h0 is None else h0
        seq_active = torch.ones(n_samples, dtype=torch.int)
        t, all_ended = 0, False
        while not all_ended and t < max_timesteps:
            enc = ops.mlp(x.reshape(n_samples, S).to(torch.float32).contiguous(), enc_lin, ops.ACT_LEAKY, ops.LEAKY_SLOPE)
            # the reference does not forward use_mode to the cell (vrnn.py:405): z is always SAMPLED from the prior
            h, out = self.vrnn_cell.generate(enc, h.contiguous(), use_mode=False, eps=None if eps is None else eps[t])
            dec = ops.mlp(torch.cat([out.phi_z, h], -1).contiguous(), dec_lin, ops.ACT_LEAKY, ops.LEAKY_SLOPE)  # [B, S*F]
            parameters = lik(dec.view(n_samples, S, lik.out_features))
            if use_mode:
                x = lik.mode(parameters)
            else:
                x = lik.sample(parameters) if uniforms is None else lik.sample(parameters, uniforms=(uniforms[0][t], uniforms[1][t]))  # [B,S,1]
            all_x.append(x)
            x_sl += seq_active
            if stop_value is not None:
                ending = (x == stop_value).flatten(1).all(1).to(torch.int).cpu()
                seq_active *= 1 - ending
            t += 1
            all_ended = bool(torch.all(1 - seq_active))
        x = torch.cat(all_x, dim=-1).permute(0, 2, 1)
        return (x, x_sl), SimpleNamespace()


    @torch.no_grad()
    def _generate_fused(self, x, h0, n_samples, max_timesteps, stop_value, use_mode, eps, uniforms):
        S, enc_lin, dec_lin, lik = self._plan()
        cell = self.vrnn_cell
        if stop_value is not None or not isinstance(lik, DiscretizedLogisticMixtureDense) or len(enc_lin) != 3 or len(dec_lin) != 3:
            raise NotImplementedError("libblvm_hip: the one-launch decoder is built for the VRNNAudio(DMoL) structure without a stop value")
        if x.size(0) == 1:
            x = x.repeat(n_samples, *[1] * (x.ndim - 1))
        assert x.size(0) == n_samples
        dev, T, B = x.device, max_timesteps, n_samples
        if eps is None:
            eps = torch.randn(T, B, cell.z_dim, device=dev)
        if use_mode:
            u = v = None
        elif uniforms is None:
            u = torch.empty(T, B, S, lik.num_mix, device=dev).uniform_(1e-5, 1.0 - 1e-5)
            v = torch.empty(T, B, S, device=dev).uniform_(1e-8, 1.0 - 1e-8)
        else:
            u, v = uniforms[0].reshape(T, B, S, lik.num_mix).to(dev), uniforms[1].reshape(T, B, S).to(dev)
        slope = next(m.negative_slope for m in self.encoder if isinstance(m, nn.LeakyReLU))
        xs, _ = ops.vrnn_decode(enc_lin, cell.kernel_params(), dec_lin, lik.params, x.reshape(B, S), h0, eps[:T], u, v, S, cell.h_dim,
                                cell.z_dim, cell.r_dim, lik.num_mix, cell.prior[6].epsilon, slope, lik.log_epsilon)  # fmt: skip
        out = torch.cat([x.reshape(B, 1, S), xs], 1)  # [B,1+T,S] like the step-by-step path
        return (out, torch.full((B,), T + 1, dtype=torch.int)), SimpleNamespace()


    @torch.no_grad()
    def _generate_gauss(self, head, x, h0, n_samples, max_timesteps, stop_value, use_mode, eps, uniforms, fused):
        """`generate` for the GMM and Gaussian heads.  The path is decided BEFORE any noise is drawn, from the structure and the
        library's own limits (`blvm_pchain_max_batch`, `blvm_vrnn_decode_applies`), and the noise is drawn once, in the reference's
        per-step order (`gauss_rollout_noise`), for whichever path replays it: a seeded call gives the same draws on either, and a
        library error is an error, never a silent second run.  use_mode: the head's mode, z still sampled (as for the DMoL head)."""
        S, enc_lin, dec_lin, lik = self._plan()
        c = self.vrnn_cell
        H, Z, R = c.h_dim, c.z_dim, c.r_dim
        if x.size(0) == 1:
            x = x.repeat(n_samples, *[1] * (x.ndim - 1))
        assert x.size(0) == n_samples
        dev, T, B = x.device, max_timesteps, n_samples
        gmm = isinstance(head, ops.GmmHead)
        structure = stop_value is None and T > 0 and len(enc_lin) == 3 and len(dec_lin) == 3
        if fused is None:
            lib = ops.load()
            fused = (structure and all(v % 16 == 0 for v in (H, Z, R)) and (not gmm or head.num_mix == 10)
                     and (B <= lib.blvm_pchain_max_batch() or (gmm and lib.blvm_vrnn_decode_applies(S, H, Z, R) == 1)))  # fmt: skip
        elif fused and not structure:
            raise NotImplementedError("libblvm_hip: the one-launch decoder is built for the VRNNAudio structure without a stop value")
        want_draws = not use_mode and uniforms is None
        e_, u, n = gauss_rollout_noise(head, T, B, S, Z, dev, eps is None, want_draws)
        eps = e_ if eps is None else torch.as_tensor(eps)[:T].reshape(T, B, Z).to(dev, torch.float32)
        if not use_mode and uniforms is not None:
            u, n = gauss_rollout_draws(head, uniforms, T, B, S, dev)
        if fused:
            slope = next(m.negative_slope for m in self.encoder if isinstance(m, nn.LeakyReLU))
            xs, _ = ops.vrnn_decode(enc_lin, c.kernel_params(), dec_lin, lik.params, x.reshape(B, S), h0, eps, u, n, S, H, Z, R,
                                    head.num_mix if gmm else 0, c.prior[6].epsilon, slope, 0.0, head=head)  # fmt: skip
            return (torch.cat([x.reshape(B, 1, S), xs], 1), torch.full((B,), T + 1, dtype=torch.int)), SimpleNamespace()
        all_x = [x]
        x_sl = torch.ones(B, dtype=torch.int)
        h = c.get_initial_state(B, dev) if h0 is None else h0
        seq_active = torch.ones(B, dtype=torch.int)
        t, all_ended = 0, False
        while not all_ended and t < T:
            enc = ops.mlp(x.reshape(B, S).to(torch.float32).contiguous(), enc_lin, ops.ACT_LEAKY, ops.LEAKY_SLOPE)
            h, out = c.generate(enc, h.contiguous(), use_mode=False, eps=eps[t])
            dec = ops.mlp(torch.cat([out.phi_z, h], -1).contiguous(), dec_lin, ops.ACT_LEAKY, ops.LEAKY_SLOPE)  # [B, S*F]
            parameters = lik(dec.view(B, S, lik.out_features))
            x = lik.mode(parameters) if use_mode else gauss_head_sample(lik, head, parameters, None if u is None else u[t], n[t])  # [B,S,1]
            all_x.append(x)
            x_sl += seq_active
            if stop_value is not None:
                seq_active *= 1 - (x == stop_value).flatten(1).all(1).to(torch.int).cpu()
            t += 1
            all_ended = bool(torch.all(1 - seq_active))
        return (torch.cat(all_x, dim=-1).permute(0, 2, 1), x_sl), SimpleNamespace()


class VRNNAudio(BaseModel):
    def __init__(self, likelihood: Union[str, nn.Module], input_size: int = 200, hidden_size: int = 256,
                 latent_size: int = 64, residual_posterior: bool = False, condition_h_on_x: bool = True,
                 condition_x_on_h: bool = True, num_mix: int = 10, num_bins: int = 256):  # fmt: skip
        super().__init__()
        self.likelihood = likelihood
        self.input_size = input_size
        self.hidden_size = hidden_size
        self.latent_size = latent_size
        self.residual_posterior = residual_posterior
        self.condition_h_on_x = condition_h_on_x
        self.condition_x_on_h = condition_x_on_h
        self.num_mix = num_mix
        self.num_bins = num_bins

        if likelihood == "DMoL":
            # the reference hard-codes num_mix=10, num_bins=2**16 on this branch whatever the ctor args say
            # (vrnn.py:464-469); x_dim still follows num_mix.
            likelihood_module = DiscretizedLogisticMixtureDense(x_dim=2 * num_mix + num_mix, y_dim=1, num_mix=10, num_bins=2**16)
        elif likelihood == "GMM":
            likelihood_module = DiagonalGaussianMixtureDense(x_dim=2 * num_mix + num_mix, y_dim=1, num_mix=num_mix, initial_sd=1,
                                                             epsilon=1e-4)  # fmt: skip
        elif likelihood == "Gaussian":
            likelihood_module = DiagonalGaussianDense(x_dim=2, y_dim=1, epsilon=1e-4)
        else:
            raise ValueError(f"Unknown likelihood type {likelihood}")

        encoder = nn.Sequential(
            View(-1),
            StackTensor(input_size, dim=1),
            nn.Linear(input_size, hidden_size),
            nn.LeakyReLU(),
            nn.Linear(hidden_size, hidden_size),
            nn.LeakyReLU(),
            nn.Linear(hidden_size, hidden_size),
            nn.LeakyReLU(),
        )
        decoder = nn.Sequential(
            nn.Linear(3 * hidden_size, hidden_size),
            nn.LeakyReLU(),
            nn.Linear(hidden_size, hidden_size),
            nn.LeakyReLU(),
            nn.Linear(hidden_size, input_size * likelihood_module.out_features),
            nn.LeakyReLU(),
            View(-1, likelihood_module.out_features),
        )
        self.vrnn = VRNN(encoder=encoder, decoder=decoder, likelihood=likelihood_module, x_dim=hidden_size, h_dim=hidden_size,
                         z_dim=latent_size, residual_posterior=residual_posterior, condition_h_on_x=condition_h_on_x,
                         condition_x_on_h=condition_x_on_h)  # fmt: skip

    def forward(self, x, x_sl, beta: float = 1, free_nats: float = 0, h0=None, eps=None):
        return self.vrnn(x, x_sl, beta, free_nats, h0, eps)

    @torch.no_grad()
    def iw_bound(self, x, x_sl, num_samples: int, eps=None, max_rows=None):
        return self.vrnn.iw_bound(x, x_sl, num_samples, eps, max_rows)

    @torch.no_grad()
    def represent(self, x, x_sl, level=None, num_samples: int = 1, eps=None, max_rows=None):
        return self.vrnn.represent(x, x_sl, level, num_samples, eps, max_rows)

    def generate(self, n_samples: int = 1, max_timesteps: int = 100, use_mode: bool = False, x=None, h0=None, eps=None, uniforms=None,
                 fused: Optional[bool] = None):  # fmt: skip
        """Same arguments as the reference (vrnn.py:529-546); `fused`: every step in one launch (K1c; default: when it applies)."""
        x = torch.zeros(n_samples, self.input_size, 1, device=self.device) if x is None else x
        return self.vrnn.generate(n_samples=n_samples, max_timesteps=max_timesteps, stop_value=None, use_mode=use_mode, x=x, h0=h0,
                                  eps=eps, uniforms=uniforms, fused=fused)  # fmt: skip
