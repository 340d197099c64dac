"""WaveNet with the reference's construction API and state_dict layout (blvm/models/wavenet/wavenet.py:29-293).

forward: left-pad by the receptive field -> causal conv -> in_transform -> 50 gated residual blocks (K10, one autograd
node) -> sum of skips * variance_scale -> ReLU-Linear-ReLU -> likelihood Linear (K6) -> DMoL log-likelihood (K7), the Gaussian-mixture
(K7b, 1..16 components) or Gaussian one (K7c), or with a `CategoricalDense` head its Linear and the softmax log-likelihood in one (K7d:
the logits are never stored).
Loss in fp32 like the reference: -sum(ll * mask) / sum(x_sl) (wavenet.py:128-146).

`embedding_dim=E` is the class-in model of the original paper (wavenet.py:105-113,182): sample classes -> nn.Embedding(num_bins, E) ->
a causal conv with groups = res_channels.  Embedding, padding and that convolution run as one gather from two lookup tables (K10e,
`ops.wavenet_embed_front`); the rest of the network is the float model's.
"""
import math
from typing import Optional

import torch
import torch.nn as nn

from blvm import ops
from blvm.evaluation import BitsPerDimMetric, DeferredScalars, LLMetric, LossMetric
from blvm.models.base_model import BaseModel
from blvm.models.vrnn import LazyNamespace
from blvm.modules.distributions import (CategoricalDense, DiagonalGaussianDense, DiagonalGaussianMixtureDense,
                                        DiscretizedLogisticMixtureDense, gauss_rollout_head)  # fmt: skip
from blvm.utils.operations import split_sequence
from blvm.utils.padding import get_modulo_length

from .wavenet_modules import CausalConv1d, PointwiseTransform, ResidualStack


class InputSizeError(Exception):
    def __init__(self, input_size, receptive_field):
        message = "Input size has to be larger than receptive_field\n"
        message += f"Input size: {input_size}, Receptive fields size: {receptive_field}"
        super().__init__(message)


class WaveNetDecodeState:
    """What cached generation needs to go on after `n_frames` samples (a prompt's included): every block's ring buffer of its
    own input over its last `dilation` frames ([d,B,C], frame tau in slot tau mod d) and the last two samples.
    `scratch`: the decode kernel's buffer the rings are views into (None on the block-by-block path).  A continued call updates
    the rings in place: a state is good for ONE continuation.  An embedded model keeps the last two CLASSES (int32) as `samples`."""

    __slots__ = ("scratch", "rings", "samples", "n_frames")

    def __init__(self, scratch, rings, samples, n_frames: int):
        self.scratch, self.rings, self.samples, self.n_frames = scratch, rings, samples, n_frames


class WaveNet(BaseModel):
    def __init__(self, likelihood: nn.Module, in_channels: int = 1, embedding_dim: int = None, num_bins: int = 256,
                 n_layers: int = 10, n_stacks: int = 5, res_channels: int = 512, skip_channels: Optional[int] = None,
                 gate_channels: Optional[int] = None, kernel_size: int = 2, base_dilation: int = 2, n_stack_frames: int = 1,
                 activation: nn.Module = nn.ReLU):  # fmt: skip
        super().__init__()
        if embedding_dim is not None and n_stack_frames > 1:
            raise ValueError("Cannot stack frames if using an embedding (which is what we do when in_channels>1)")
        if embedding_dim is not None and in_channels > 1:
            raise ValueError("Cannot use more than 1 input_channel if also wanting to use an embedding.")
        if embedding_dim is not None and (embedding_dim % res_channels != 0 or kernel_size != 2 or res_channels % 4 != 0):
            # (nn.Conv1d(groups=res_channels) itself refuses an embedding_dim that is no multiple of res_channels)
            raise NotImplementedError("libblvm_hip: the embedding input variant of WaveNet is built for embedding_dim a multiple of "
                                      "res_channels (its causal conv has groups=res_channels), res_channels a multiple of 4, kernel_size 2")  # fmt: skip
        self.n_layers, self.n_stacks, self.in_channels, self.embedding_dim = n_layers, n_stacks, in_channels, embedding_dim
        self.res_channels, self.skip_channels, self.gate_channels = res_channels, skip_channels, gate_channels
        self.kernel_size, self.base_dilation, self.num_bins = kernel_size, base_dilation, num_bins
        self.n_stack_frames, self.activation = n_stack_frames, activation
        self.variance_scale = math.sqrt(1 / self.n_stacks * self.n_layers)
        if embedding_dim is None:
            self.embedding = None
            self.causal = CausalConv1d(in_channels=in_channels * n_stack_frames, out_channels=res_channels, kernel_size=kernel_size)
        else:
            self.embedding = nn.Embedding(num_embeddings=num_bins, embedding_dim=embedding_dim)
            self.causal = CausalConv1d(in_channels=embedding_dim, out_channels=res_channels, kernel_size=kernel_size, groups=res_channels)
            # the class values `Quantize(bins=num_bins)` maps back to the classes (as `CategoricalDense.levels`); not in the state_dict
            self.register_buffer("levels", torch.linspace(-1.0, 1.0, num_bins), persistent=False)
        self.res_stack = ResidualStack(n_layers=n_layers, n_stacks=n_stacks, res_channels=res_channels, kernel_size=kernel_size,
                                       base_dilation=base_dilation)  # fmt: skip
        self.receptive_field = self.res_stack.receptive_field + self.causal.kernel_size - 1
        self.out_transform = PointwiseTransform(res_channels, res_channels * n_stack_frames)
        self.likelihood = likelihood

    def forward(self, x, x_sl, y=None, pad_causal: bool = True, pad_receptive_field: bool = True):
        lik, nsf, rf = self.likelihood, self.n_stack_frames, self.receptive_field
        cat = isinstance(lik, CategoricalDense)
        if not cat and not isinstance(lik, (DiscretizedLogisticMixtureDense, DiagonalGaussianMixtureDense, DiagonalGaussianDense)):
            raise NotImplementedError("libblvm_hip: WaveNet is built with the DMoL, the categorical, the Gaussian and the Gaussian-mixture likelihood heads")
        if x.ndim == 3:
            x = x.squeeze(-1)
        dev = x.device
        k = None
        if self.embedding is not None:  # classes in: an integer x as it stands, a float x quantised by the categorical target's rule
            k = self._classes(x)
            if y is None and cat and lik.y_dim != self.num_bins:
                raise ValueError(f"WaveNet: the {self.num_bins} input classes are no targets for a head of {lik.y_dim} classes: give y")
            x = x.detach().to(torch.float32) if x.is_floating_point() else (self.levels[k] if y is None and not cat else k)
        else:
            x = x.to(torch.float32)
        x_sl_host = x_sl.detach().cpu().to(torch.int64)
        if y is None and k is not None and cat:  # the classes are the targets
            y = k if pad_receptive_field else k[:, rf:]
        elif y is None:
            y = x.detach()
            if cat:  # Quantize(bins=V) on the device: class V (a value above 1) joins the top class
                y = torch.bucketize(y, lik.levels, right=False).clamp(max=lik.y_dim - 1)
            if not pad_receptive_field:
                y = y[:, rf * nsf :]
        elif cat and (y.is_floating_point() or y.is_complex()):
            raise TypeError(f"WaveNet: the categorical head takes integer class targets y [B,T], got {y.dtype}")
        y = y.reshape(y.size(0), -1).contiguous()
        x_sl_strided = (x_sl_host / nsf).ceil().int()
        B = x.size(0)
        if k is not None:
            xt = k.t().to(torch.int32)  # time-major classes [T,B]
        elif nsf > 1:
            T = x.size(1)
            Tp = (T + nsf - 1) // nsf
            xt = torch.nn.functional.pad(x, (0, Tp * nsf - T)).view(B, Tp, nsf).transpose(0, 1).contiguous()
        else:
            xt = x.unsqueeze(-1).transpose(0, 1).contiguous()  # time-major [T',B,C_in]
        if pad_receptive_field:
            skip_size = xt.size(0)
            # zeros in front; of an embedded model index -1, the zero row: the reference pads AFTER embedding (wavenet.py:182-188)
            pad = torch.zeros(rf, B, xt.size(2), device=dev) if k is None else torch.full((rf, B), -1, device=dev, dtype=torch.int32)
            xt = torch.cat([pad, xt], 0)
        else:
            skip_size = xt.size(0) - rf
            x_sl_host = x_sl_host - rf
        if xt.size(0) - int(pad_causal) < rf:
            raise InputSizeError(xt.size(0), rf)

        if k is None:
            out = self.causal.forward_tm(xt, pad_causal=pad_causal)
        else:
            out = ops.wavenet_embed_front(xt, self.embedding.weight, self.causal.conv.weight, self.causal.conv.bias, pad_causal)
        skip_sum = self.res_stack.forward_tm(out, skip_size)  # [skip_size,B,C]
        C = self.res_channels
        logits = self.out_transform.forward_rows(skip_sum.view(skip_size * B, C), self.variance_scale)  # [skip*B, C*nsf]
        T_y = y.size(1)
        mask_len = ops.upload_i32(x_sl_host.clamp(min=0, max=T_y), dev)
        if cat:
            return self._categorical_outputs(logits, y, mask_len, x_sl_host, x_sl_strided, skip_sum, B, T_y, skip_size)
        return self._float_head_outputs(logits, y, mask_len, x_sl_host, x_sl_strided, skip_sum, B, T_y, skip_size)

    def _head_parameters(self, p):
        """Head outputs p [B,T,F] -> `likelihood.forward`'s tuple in the reference's shapes: DMoL (logits [B,T,K], locs [B,T,1,K],
        log_scales [B,T,1,K] clamped), the mixture (logits, mu [B,T,1,K], sd [B,T,1,K]), the Gaussian (mu [B,T,1], sd [B,T,1])."""
        lik = self.likelihood
        if isinstance(lik, DiagonalGaussianDense):
            mu, raw = p.chunk(2, dim=-1)
            return mu, lik.sd_activation(raw)
        K = lik.num_mix
        logits_, rest = p[..., :K], p[..., K:].reshape(*p.shape[:-1], 1, 2 * K)
        locs, scales = rest.chunk(2, dim=-1)
        if isinstance(lik, DiagonalGaussianMixtureDense):
            return logits_, locs, lik.sd_activation(scales)
        return logits_, locs, scales.clamp(min=lik.log_epsilon)

    def _head_ll_twise(self, par2d, y, mask_len, B, T_y, skip_size):
        """Masked frame-wise log-likelihood [B,T_y] of a float head from its outputs par2d [skip*B, nsf*F] (K7 / K7b / K7c)."""
        lik, nsf = self.likelihood, self.n_stack_frames
        tm = (par2d, None, None, y, mask_len, ops.LAYOUT_TIME_MAJOR, B, T_y, skip_size, nsf)
        if isinstance(lik, DiagonalGaussianMixtureDense):
            return ops.gmm_ll_twise(*tm, lik.num_mix, lik.softplus_beta, lik.epsilon if lik.epsilon > 0 else 0.0)[0]
        if isinstance(lik, DiagonalGaussianDense):
            return ops.gauss_ll_twise(*tm, lik.softplus_beta, lik.epsilon)[0]
        return ops.dmol_ll_twise(*tm, lik.num_mix, lik.num_bins, lik.log_epsilon)[0]

    def _float_head_outputs(self, dec, y, mask_len, x_sl_host, x_sl_strided, skip_sum, B, T_y, skip_size):
        """A head on float targets — DMoL, Gaussian mixture, Gaussian — on the output transform's activations `dec` [skip*B, C*nsf]:
        the head Linear C -> F as a K6 GEMM, then the head's fused log-likelihood on its F outputs per frame (F = 3 num_mix, or 2)."""
        lik, nsf, C = self.likelihood, self.n_stack_frames, self.res_channels
        F = lik.out_features
        par = ops.linear(dec.view(skip_size * B * nsf, C), lik.params.weight, lik.params.bias)  # [skip*B*nsf, F]
        log_prob = lik.fused_log_prob(par.view(skip_size * B, nsf * F), y, mask_len, ops.LAYOUT_TIME_MAJOR, B, T_y, skip_size, nsf,
                                      fused_linear=False).to(torch.float32)  # fmt: skip
        n_frames = float(x_sl_host.sum())
        loss = -log_prob.sum() / n_frames

        sums = DeferredScalars(torch.stack([loss.detach().double(), log_prob.detach().double().sum()]))
        metrics = [
            LossMetric(sums[0], weight_by=B),
            LLMetric(sums[1], reduce_by=B),
            BitsPerDimMetric(sums[1], reduce_by=n_frames),
        ]

        def parameters():
            p = par.detach().view(skip_size, B, nsf, F).permute(1, 0, 2, 3).reshape(B, skip_size * nsf, F)[:, :T_y]
            return self._head_parameters(p)

        lazy = dict(
            parameters=parameters,
            log_prob_twise=lambda: self._head_ll_twise(par.detach().view(skip_size * B, nsf * F), y, mask_len, B, T_y, skip_size),
            predictions=lambda ns: lik.sample(ns.parameters),
            predictions_mode=lambda ns: lik.mode(ns.parameters),
        )
        output = LazyNamespace(lazy, loss=loss, log_prob=log_prob, z=[skip_sum.detach().transpose(0, 1)], z_sl=x_sl_strided,
                               y=y.unsqueeze(-1))  # fmt: skip
        return loss, metrics, output

    def _categorical_outputs(self, dec, y, mask_len, x_sl_host, x_sl_strided, skip_sum, B, T_y, skip_size):
        """The categorical head on the output transform's activations `dec` [skip*B, C*nsf] (K7d: the head's Linear, the
        log-softmax, the gather at y, the mask and the per-utterance sums without a [frames, V] tensor); the same loss, metrics and
        lazy outputs as the DMoL head.  `output.parameters` are the materialised logits [B,T,V]: ask for them at small T * V only."""
        lik, nsf, C = self.likelihood, self.n_stack_frames, self.res_channels
        log_prob = lik.fused_log_prob(dec, y, mask_len, B, T_y, skip_size, nsf).to(torch.float32)
        n_frames = float(x_sl_host.sum())
        loss = -log_prob.sum() / n_frames
        sums = DeferredScalars(torch.stack([loss.detach().double(), log_prob.detach().double().sum()]))
        metrics = [
            LossMetric(sums[0], weight_by=B),
            LLMetric(sums[1], reduce_by=B),
            BitsPerDimMetric(sums[1], reduce_by=n_frames),
        ]
        V = lik.y_dim

        def parameters():
            with torch.no_grad():
                p = lik(dec.detach().view(skip_size * B * nsf, C))
            return p.view(skip_size, B, nsf, V).permute(1, 0, 2, 3).reshape(B, skip_size * nsf, V)[:, :T_y]

        lazy = dict(
            parameters=parameters,
            log_prob_twise=lambda: ops.categorical_ll_twise(dec, lik.logits.weight, lik.logits.bias, y, mask_len, B, T_y, skip_size, nsf),
            predictions=lambda ns: lik.sample(ns.parameters),
            predictions_mode=lambda ns: lik.mode(ns.parameters),
        )
        output = LazyNamespace(lazy, loss=loss, log_prob=log_prob, z=[skip_sum.detach().transpose(0, 1)], z_sl=x_sl_strided,
                               y=y.unsqueeze(-1))  # fmt: skip
        return loss, metrics, output

    def _classes(self, x):
        """x [B,T] of an embedded model -> its classes [B,T] int64: an integer x as it stands, a float x by `Quantize(bins=num_bins)`'s
        rule (`bucketize` on linspace(-1, 1, V), a value above 1 joining the top class)."""
        if x.ndim == 3:
            x = x.squeeze(-1)
        if x.is_floating_point():
            return torch.bucketize(x.detach().to(torch.float32), self.levels, right=False).clamp(max=self.num_bins - 1)
        return x.detach().long()

    def _draw(self, parameters, u):
        """One draw per head evaluation -> floats [B,nsf,1]; the categorical head's class k is fed back as `dequantize(k)`."""
        lik = self.likelihood
        if isinstance(lik, CategoricalDense):
            k = lik.sample(parameters, uniforms=None if u is None else u.reshape(parameters.shape[:-1]))
            return lik.dequantize(k).unsqueeze(-1)
        if isinstance(lik, DiagonalGaussianMixtureDense):  # u = (u [B,nsf,n], n [B,nsf]); None: uniform(1e-6, 1 - 1e-6), then randn
            if u is None:
                return lik.sample(parameters)
            lead = parameters[0].shape[:-1]
            return lik.sample(parameters, noise=(u[0].reshape(*lead, lik.num_mix), u[1].reshape(lead)))
        if isinstance(lik, DiagonalGaussianDense):  # u = (None, n [B,nsf]) or n; None: randn
            if u is None:
                return lik.sample(parameters)
            return lik.sample(parameters, noise=u[1] if isinstance(u, (tuple, list)) else u)
        return lik.sample(parameters) if u is None else lik.sample(parameters, uniforms=u)

    def split_sequence(self, x, x_sl, length: int):
        """Overlap = receptive field (wavenet.py:230-242)."""
        overlap = self.receptive_field * self.n_stack_frames
        length = get_modulo_length(length, stride=self.n_stack_frames)
        mode = "extend" if overlap >= length else "consume"
        splits_x, splits_x_sl = split_sequence(x, x_sl, length=length, overlap=overlap, mode=mode)
        if mode == "extend":
            # pad_to_length(split, overlap + length, "left", dim=1) (wavenet.py:240): zeros in front of the TIME axis, whatever follows it
            splits_x = [torch.nn.functional.pad(s, (0, 0) * (s.ndim - 2) + (max(overlap + length - s.size(1), 0), 0)) for s in splits_x]
        return splits_x, splits_x_sl

    def forward_split(self, x, x_sl, i_split: int, y=None):
        return self.forward(x, x_sl, y=y, pad_causal=True, pad_receptive_field=(i_split == 0))

    @torch.no_grad()
    def generate(self, n_samples: int, n_frames: int = 48000, x=None, uniforms=None, cached: bool = False, state=None,
                 return_state: bool = False):  # fmt: skip
        """Sample-by-sample generation from a zero start (wavenet.py:254-293): every frame re-runs the causal conv and the
        whole residual stack over a receptive-field window (no cached sampling, as in the reference), takes the single skip
        output, DIVIDES it by variance_scale (the reference's generate divides where forward multiplies, :274 — kept), applies
        the output transform and the head, samples, and shifts the window (FIFO).  Returns x_hat [B, n_frames, 1].
        `uniforms[t]` optionally supplies the head sampler's draws of frame t: the DMoL head's two, the categorical head's one [B]
        (its class k is fed back and returned as the float `dequantize(k)`), the Gaussian mixture's (u [B,nsf,num_mix] uniforms,
        n [B,nsf] standard normals), the Gaussian head's (None, n [B,nsf]) or n; the Gaussian draws are not clamped.
        `cached=True` (the reference's TODO, arXiv:1611.09482): the same samples from per-block queues of past activations —
        one new frame per block per step instead of the whole window; at the widths the decode kernel takes (K10c: every frame in
        one launch) through `ops.wavenet_decode` (the DMoL head, the Gaussian head, the Gaussian mixture of up to 10 components, or the
        categorical head with 16 <= V <= 1024 classes, V a multiple of 16), otherwise block by block (`_generate_cached`).
        With `cached=True`, `x` [B,P,1] is a prompt: the queues are primed from its last receptive-field samples (`_prime`) and
        frames P, P+1, ... are drawn.  `return_state=True` returns (x_hat, state); `state=` continues from one (generation in
        chunks; `uniforms` are indexed from 0 for every call).
        An embedded model generates with the categorical head (the drawn class is the next input class) on all three paths and returns
        `dequantize(k)` floats like the float-input model; its zero start is a past of class 0 (the reference's `embedding(zeros)`
        window, wavenet.py:264-266), a prompt is classes [B,P] or floats [B,P,1] (quantised), on either path."""
        lik, C, nsf = self.likelihood, self.res_channels, self.n_stack_frames
        if self.embedding is not None:
            if not isinstance(lik, CategoricalDense):
                raise NotImplementedError("libblvm_hip: the embedded WaveNet generates with the categorical head (a drawn class is the next input)")
            if lik.y_dim != self.num_bins:
                raise ValueError(f"WaveNet.generate: a head of {lik.y_dim} classes cannot feed an embedding of {self.num_bins}")
        if nsf != 1 and (cached or self.in_channels != 1):
            raise NotImplementedError("libblvm_hip: WaveNet.generate on frame stacks is the window path with in_channels=1 (cached=False)")
        if not cached and (state is not None or return_state):
            raise NotImplementedError("libblvm_hip: WaveNet.generate keeps a resumable state on the cached path only (cached=True)")
        if cached:
            if x is not None and state is not None:
                raise ValueError("WaveNet.generate: a prompt `x` and a `state` are given; a state already contains its past")
            if x is not None:
                if x.size(0) != n_samples:
                    raise ValueError(f"WaveNet.generate: prompt of {x.size(0)} rows for n_samples = {n_samples}")
                state = self._prime(x)
            one_launch = self._decode_kernel_applies() or self._cat_decode_kernel_applies() or self._gauss_decode_kernel_applies()
            run = self._generate_one_launch if one_launch else self._generate_cached
            if state is None and not return_state:
                return run(n_samples, n_frames, uniforms)
            x_hat, state = run(n_samples, n_frames, uniforms, state=state, want_state=True)
            return (x_hat, state) if return_state else x_hat
        dev = self.causal.conv.weight.device
        if self.embedding is not None:
            return self._generate_window_embedded(n_samples, n_frames, x, uniforms)
        win = torch.zeros(self.receptive_field, n_samples, self.in_channels * nsf, device=dev) if x is None else x.transpose(0, 1).contiguous()
        x_hat = []
        for t in range(n_frames):
            out = self.causal.forward_tm(win, pad_causal=False)
            skip = self.res_stack.forward_tm(out, 1)  # [1,B,C]
            logits = self.out_transform.forward_rows(skip.view(n_samples, C), 1.0 / self.variance_scale)  # [B, C * nsf]
            parameters = lik(logits.view(n_samples, nsf, C))  # unstack_tensor(logits, nsf) (wavenet.py:277-278): one head evaluation per stacked sample
            pred = self._draw(parameters, None if uniforms is None else uniforms[t])  # [B,nsf,1]
            x_hat.append(pred)
            # the nsf new samples are the channels of the next input frame (wavenet.py:290; nsf = 1: one sample, one channel)
            win = torch.cat([win[1:], pred.reshape(1, n_samples, nsf).to(torch.float32)], 0)
        return torch.hstack(x_hat)

    def _class_window(self, x, n_samples: int, width: int):
        """The last `width` classes of a prompt (classes [B,P] or floats [B,P,1]; None: no prompt), class 0 in front of a shorter
        one (the zero start) -> int32 [B,width] on the model's device."""
        dev = self.causal.conv.weight.device
        if x is None:
            return torch.zeros(n_samples, width, device=dev, dtype=torch.int32)
        k = self._classes(x.to(dev))
        if k.ndim != 2 or k.size(0) != n_samples:
            raise ValueError(f"WaveNet.generate: a prompt of classes [B,P] or floats [B,P,1] with B = {n_samples}, got {tuple(x.shape)}")
        k = k[:, -width:].to(torch.int32)
        return torch.nn.functional.pad(k, (width - k.size(1), 0))

    def _front_tables(self):
        return ops.wavenet_embed_tables(self.embedding.weight, self.causal.conv.weight)

    @torch.no_grad()
    def _generate_window_embedded(self, n_samples: int, n_frames: int, x=None, uniforms=None):
        """The window path of `generate` on classes: the window holds the last receptive_field classes, the front is the table
        lookup (K10e), the drawn class shifts in."""
        lik, C, B = self.likelihood, self.res_channels, n_samples
        tables, bias = self._front_tables(), self.causal.conv.bias
        win = self._class_window(x, B, self.receptive_field).t().contiguous()  # [rf,B]
        ks = []
        for t in range(n_frames):
            out = ops.wavenet_embed_lookup(tables, bias, win, pad_causal=False)
            skip = self.res_stack.forward_tm(out, 1)  # [1,B,C]
            logits = self.out_transform.forward_rows(skip.view(B, C), 1.0 / self.variance_scale)
            k = lik.sample(lik(logits.view(B, 1, C)), uniforms=None if uniforms is None else uniforms[t].reshape(B, 1))  # [B,1]
            ks.append(k)
            win = torch.cat([win[1:], k.view(1, B).to(torch.int32)], 0)
        return lik.dequantize(torch.cat(ks, 1)).unsqueeze(-1)

    def _decode_widths_fit(self):
        """The widths the decode kernel (K10c) takes, whatever the head."""
        C, blk = self.res_channels, self.res_stack.res_blocks[0]
        return (self.in_channels == 1 and C % 16 == 0 and blk.skip_channels % 16 == 0 and C <= 128 and blk.skip_channels <= 128
                and len(self.res_stack.res_blocks) <= 64)  # fmt: skip

    def _decode_kernel_applies(self):
        lik = self.likelihood
        return isinstance(lik, DiscretizedLogisticMixtureDense) and lik.y_dim == 1 and lik.out_features <= 32 and self._decode_widths_fit()

    def _cat_decode_kernel_applies(self):
        """The decode kernel's categorical head: 16 <= V <= 1024 in multiples of 16 (a larger softmax wants its head Linear split
        across workgroups: block by block, `_generate_cached`), the widths of `_decode_kernel_applies`.  An embedded model (which
        generates with this head only, y_dim == num_bins) runs the kernel's embedded arm at the same widths."""
        lik = self.likelihood
        return (isinstance(lik, CategoricalDense) and 16 <= lik.y_dim <= 1024 and lik.y_dim % 16 == 0 and self.n_stack_frames == 1
                and self._decode_widths_fit())  # fmt: skip

    def _gauss_decode_kernel_applies(self):
        """The decode kernel's Gaussian heads: one output dimension, a mixture of 3 * num_mix <= 32 head rows (the DMoL head's padded
        image; 11 or more components generate block by block), the widths of `_decode_kernel_applies`."""
        lik = self.likelihood
        if isinstance(lik, DiagonalGaussianMixtureDense):
            return lik.y_dim == 1 and 3 * lik.num_mix <= 32 and self._decode_widths_fit()
        return isinstance(lik, DiagonalGaussianDense) and lik.y_dim == 1 and self._decode_widths_fit()

    @torch.no_grad()
    def _prime(self, x):
        """Prompt x [B,P,1] (P >= 1) -> the decode state after its P samples.  Only the last receptive_field samples matter; a
        shorter prompt is left-padded with zeros, which is what the zero start means.  The frame the two newest samples give is
        the first one generation evaluates, so the window that fills the queues ends one sample earlier: the causal conv drops
        it (`pad_causal=True`), the in_transform and the time-parallel block kernels give every block's input over the window
        (`ops.wavenet_prime_rings`), and each ring buffer takes the last `dilation` frames of its block's input.
        An embedded model: the prompt is classes [B,P] (or floats, quantised), padded with class 0; the state keeps two classes."""
        rs, rf, C = self.res_stack, self.receptive_field, self.res_channels
        dev = self.causal.conv.weight.device
        if self.embedding is not None:
            if x.size(1) < 1:
                raise NotImplementedError("libblvm_hip: cached generation takes a prompt of P >= 1 samples")
            B, P = x.size(0), x.size(1)
            win = self._class_window(x, B, rf)  # [B,rf]
            out = ops.wavenet_embed_lookup(self._front_tables(), self.causal.conv.bias, win.t().contiguous(), pad_causal=True)  # [rf-2,B,C]
        else:
            if self.in_channels != 1 or x.ndim != 3 or x.size(2) != 1 or x.size(1) < 1:
                raise NotImplementedError("libblvm_hip: cached generation takes a prompt [B,P,1] with P >= 1 (in_channels = 1)")
            B, P = x.size(0), x.size(1)
            win = x[:, -rf:, 0].to(device=dev, dtype=torch.float32)
            win = torch.nn.functional.pad(win, (rf - win.size(1), 0))  # [B,rf]
            out = self.causal.forward_tm(win.t().contiguous().unsqueeze(-1), pad_causal=True)  # [rf-2,B,C]: absolute frames P-rf+2 .. P-1
        L, t_in, blk = out.size(0), rs.in_transform, rs.res_blocks[0]
        h0 = ops.linear(out.reshape(L * B, C), t_in.weight.view(t_in.out_channels, C), t_in.bias).view(L, B, C)
        scratch, rings = ops.wavenet_decode_scratch(rs.dilations, B, C, blk.skip_channels, dev)
        ops.wavenet_prime_rings(h0, [b.kernel_params() for b in rs.res_blocks], rs.dilations, blk.inv_std, blk.skip_channels, P, rings)
        return WaveNetDecodeState(scratch, rings, win[:, -2:].contiguous(), P)

    def _one_launch_parts(self):
        """The `weights` argument of `ops.wavenet_decode`; the head Linear is the categorical head's `logits`, any other head's `params`."""
        rs, lik = self.res_stack, self.likelihood
        t_in = rs.in_transform
        head = lik.logits if isinstance(lik, CategoricalDense) else lik.params
        causal = self.causal.conv.weight if self.embedding is None else self._front_tables()  # (K10e: the tables in the weights' place)
        return ((causal, self.causal.conv.bias), (t_in.weight.view(t_in.out_channels, -1), t_in.bias),
                [b.kernel_params() for b in rs.res_blocks], rs.dilations,
                (self.out_transform.linear.weight, self.out_transform.linear.bias), (head.weight, head.bias))  # fmt: skip

    def _one_launch_head(self, B: int, n_frames: int, uniforms):
        """-> (the `head` argument of `ops.wavenet_decode`, its draws).  Categorical: `uniforms[t]` [B] is the head's one draw of frame
        t (None: torch.rand on the device); class k comes back as `likelihood.levels[k]`, the float `dequantize(k)` returns."""
        lik, dev = self.likelihood, self.causal.conv.weight.device
        if isinstance(lik, CategoricalDense):
            if uniforms is None:
                u = torch.rand(n_frames, B, device=dev)
            else:
                u = torch.stack([a.reshape(B) for a in uniforms[:n_frames]]).to(device=dev, dtype=torch.float32)
            return ops.CategoricalHead(lik.levels), u
        head = gauss_rollout_head(lik)
        if head is not None:  # the Gaussian heads: (u [n_frames,B,num_mix], n [n_frames,B]) for the mixture, n alone otherwise
            mix = isinstance(head, ops.GmmHead)
            if uniforms is None:  # the ranges `gauss_rollout_noise` documents
                u = torch.empty(n_frames, B, lik.num_mix, device=dev).uniform_(1e-6, 1.0 - 1e-6) if mix else None
                nrm = torch.randn(n_frames, B, device=dev)
            else:
                draws = [a if isinstance(a, (tuple, list)) else (None, a) for a in uniforms[:n_frames]]
                u = torch.stack([torch.as_tensor(a).reshape(B, lik.num_mix) for a, _ in draws]).to(device=dev, dtype=torch.float32) if mix else None
                nrm = torch.stack([torch.as_tensor(b).reshape(B) for _, b in draws]).to(device=dev, dtype=torch.float32)
            return head, ((u, nrm) if mix else nrm)
        if uniforms is None:
            u = torch.empty(n_frames, B, lik.num_mix, device=dev).uniform_(1e-5, 1.0 - 1e-5)  # the reference's two draws (variational.py:309-349)
            v = torch.empty(n_frames, B, device=dev).uniform_(1e-8, 1.0 - 1e-8)
        else:
            u = torch.stack([a.reshape(B, lik.num_mix) for a, _ in uniforms[:n_frames]]).to(dev)
            v = torch.stack([b.reshape(B) for _, b in uniforms[:n_frames]]).to(dev)
        return ops.DmolHead(lik.num_mix, lik.log_epsilon), (u, v)

    @torch.no_grad()
    def _generate_one_launch(self, n_samples: int, n_frames: int, uniforms=None, state=None, want_state: bool = False):
        """The decode kernel (K10c), either head: every frame in one launch, from the zero start or from `state` (a prompt's, `_prime`,
        or an earlier call's, whose scratch buffer is updated in place); `want_state` returns (x_hat, state)."""
        rs, B = self.res_stack, n_samples
        blk = rs.res_blocks[0]
        head, draws = self._one_launch_head(B, n_frames, uniforms)
        resume = None
        if state is not None:
            if state.scratch is None or tuple(state.samples.shape) != (B, 2):
                raise ValueError("WaveNet.generate: the state does not come from the decode kernel's path at this batch size")
            # the kernel takes the phase of frame `state.n_frames` in every ring: any t0 equal to it modulo all dilations
            resume = (state.n_frames % math.lcm(*rs.dilations), state.samples, state.scratch)
        out = ops.wavenet_decode(self._one_launch_parts(), head, B, n_frames, blk.inv_std, 1.0 / self.variance_scale, draws=draws,
                                 resume=resume)  # fmt: skip
        x_hat = out.x.unsqueeze(-1)
        if not want_state:
            return x_hat
        if state is None:  # the zero start, keeping its scratch: the samples in front of frame 0 are zeros (embedded: class 0)
            last = out.x if self.embedding is None else out.k
            samples = torch.cat([last.new_zeros(B, 2), last], 1)[:, -2:].contiguous()
            rings, before = ops.wavenet_ring_views(out.scratch, rs.dilations, B, self.res_channels, blk.skip_channels), 0
        else:
            samples, rings, before = out.samples, state.rings, state.n_frames
        return x_hat, WaveNetDecodeState(out.scratch, rings, samples, before + n_frames)

    @torch.no_grad()
    def _generate_cached(self, n_samples: int, n_frames: int, uniforms=None, state=None, want_state: bool = False):
        """Queue-based generation.  A window of zeros is an all-zero past, under which every layer sits at a constant
        activation (its response to zero input, biases included); the queues start from those steady states — one chain of
        single-frame block evaluations with both taps on the same vector — and each step then feeds the last two samples
        through the causal conv and ONE frame through every block (tap 0 = the block's input `dilation` steps ago, from its
        ring buffer; tap 1 = its input now), accumulating the skip branches.
        `state` (a prompt's, `_prime`, or an earlier call's) replaces the steady-state fill; `want_state` returns (x_hat, state)."""
        lik, C, B = self.likelihood, self.res_channels, n_samples
        dev = self.causal.conv.weight.device
        rs, blocks = self.res_stack, self.res_stack.res_blocks
        S, inv_std = blocks[0].skip_channels, blocks[0].inv_std
        t_in = rs.in_transform

        emb = self.embedding is not None
        if emb:
            tables = self._front_tables()

        def causal_pair(x_prev, x_now):  # [B,Cin] each -> causal conv output for the newest position, then the 1x1 in_transform
            if emb:  # [B,1] classes each: two table rows (K10e)
                c = ops.wavenet_embed_lookup(tables, self.causal.conv.bias, torch.cat([x_prev, x_now], 1).t().contiguous(), pad_causal=False)
            else:
                c = self.causal.forward_tm(torch.stack([x_prev, x_now], 0), pad_causal=False)  # [1,B,C]
            return ops.linear(c.view(B, C), t_in.weight.view(t_in.out_channels, C), t_in.bias)

        def through_blocks(h, taps0, skip):
            """h [B,C]: input of block 0 now; taps0[i] [B,C]: block i's input `dilation_i` steps ago.  Returns every block's input."""
            inputs = []
            for i, blk in enumerate(blocks):
                inputs.append(h)
                last = i == len(blocks) - 1
                o = ops.wavenet_block_step(torch.stack([taps0[i], h], 0), blk.kernel_params(), inv_std, S, skip, want_output=not last)
                h = o.view(B, C) if o is not None else None
            return inputs

        zero_x = torch.zeros(B, 1, device=dev, dtype=torch.int32) if emb else torch.zeros(B, self.in_channels, device=dev)
        if state is None:
            # steady state under an all-zero past: block i's delayed input equals its current input
            h, steady = causal_pair(zero_x, zero_x), []
            for i, blk in enumerate(blocks):
                steady.append(h)
                if i < len(blocks) - 1:
                    h = ops.wavenet_block_step(torch.stack([h, h], 0), blk.kernel_params(), inv_std, S, torch.zeros(1, B, S, device=dev)).view(B, C)
            queues = [steady[i].unsqueeze(0).repeat(d, 1, 1) for i, d in enumerate(rs.dilations)]  # ring buffers [d_i,B,C]
            heads = [0] * len(blocks)
            x_prev, x_now = zero_x, zero_x
            scratch, frames_before = None, 0
        else:
            if tuple(state.samples.shape) != (B, 2) or self.in_channels != 1:
                raise ValueError("WaveNet.generate: the state does not fit this model and batch size")
            queues, scratch, frames_before = state.rings, state.scratch, state.n_frames
            heads = [frames_before % d for d in rs.dilations]  # frame tau lives in slot tau mod d
            x_prev, x_now = state.samples[:, 0:1].contiguous(), state.samples[:, 1:2].contiguous()
        x_hat = []
        for t in range(n_frames):
            skip = torch.zeros(1, B, S, device=dev)
            taps0 = [queues[i][heads[i]] for i in range(len(blocks))]
            inputs = through_blocks(causal_pair(x_prev, x_now), taps0, skip)
            for i, d in enumerate(rs.dilations):  # overwrite the oldest entry with the current input
                queues[i][heads[i]] = inputs[i]
                heads[i] = (heads[i] + 1) % d
            logits = self.out_transform.forward_rows(skip.view(B, C), 1.0 / self.variance_scale)
            parameters = lik(logits.view(B, 1, C))
            if emb:
                k = lik.sample(parameters, uniforms=None if uniforms is None else uniforms[t].reshape(B, 1))  # [B,1]
                x_hat.append(lik.dequantize(k).unsqueeze(-1))
                x_prev, x_now = x_now, k.view(B, 1).to(torch.int32)
                continue
            pred = self._draw(parameters, None if uniforms is None else uniforms[t])  # [B,1,1]
            x_hat.append(pred)
            x_prev, x_now = x_now, pred.view(B, 1).to(torch.float32)
        x_hat = torch.hstack(x_hat)
        if want_state:
            return x_hat, WaveNetDecodeState(scratch, queues, torch.cat([x_prev, x_now], 1), frames_before + n_frames)
        return x_hat
