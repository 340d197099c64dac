"""LSTMAudio: deterministic autoregressive baseline with the reference's API (blvm/models/lstm.py:17-141).

stack frames -> embedding MLP (K6) -> 1-layer LSTM with packed-sequence semantics (K4) -> decoder MLP (K6) ->
DMoL next-stack prediction (K7).  Faithful quirks: the loss mask uses x_sl against the SHIFTED target (so a row's
first stack is never scored and up to one stack past its packed length is), and the loss divides by sum(x_sl)
including those unscored frames (lstm.py:111-115).
"""
from types import SimpleNamespace
from typing import Optional

import torch
import torch.nn as nn

from blvm import _hip, ops
from blvm.evaluation import BitsPerDimMetric, DeferredScalars, LLMetric, LossMetric
from blvm.models.base_model import BaseModel
from blvm.models.vrnn import LazyNamespace
from blvm.modules.distributions import DiscretizedLogisticMixtureDense


class LSTMAudio(BaseModel):
    def __init__(self, stack_size: int = 64, hidden_size: int = 256, num_layers: int = 1, dropout: float = 0,
                 batch_first: bool = True, num_mix: int = 10, num_bins: int = 256):  # fmt: skip
        super().__init__()
        self.stack_size = stack_size
        self.hidden_size = hidden_size
        self.num_layers = num_layers
        self.dropout = dropout
        self.batch_first = batch_first
        self.num_mix = num_mix
        self.num_bins = num_bins
        if dropout:
            raise NotImplementedError("libblvm_hip: LSTMAudio is built for dropout=0 (every benchmark run)")

        def mlp(i, o):
            return nn.Sequential(nn.Linear(i, hidden_size), nn.ReLU(), nn.Linear(hidden_size, hidden_size), nn.ReLU(),
                                 nn.Linear(hidden_size, o), nn.ReLU())  # fmt: skip

        self.embedding = mlp(stack_size, hidden_size)
        self.lstm = nn.LSTM(input_size=hidden_size, hidden_size=hidden_size, num_layers=num_layers, bias=True,
                            batch_first=batch_first, dropout=dropout, bidirectional=False, proj_size=0)  # fmt: skip
        self.dropout = None
        self.decoder = mlp(hidden_size, 3 * num_mix * stack_size)
        self.likelihood = DiscretizedLogisticMixtureDense(x_dim=3 * num_mix, y_dim=1, num_mix=num_mix, num_bins=num_bins)

    def forward(self, x: torch.Tensor, x_sl: torch.Tensor, s_0=None):
        S, H, lik = self.stack_size, self.hidden_size, self.likelihood
        dev = x.device
        x_sl_host = x_sl.detach().cpu().to(torch.int64)
        B, T = x.shape
        Tp = (T + S - 1) // S
        L = Tp - 1  # input steps = stacks[:-1], targets = stacks[1:]
        if L < 1:
            raise ValueError("LSTMAudio needs at least two stacks of samples")
        x_sl_stack = (x_sl_host / S).ceil().int()
        xf = x.detach().to(torch.float32)
        xs = torch.nn.functional.pad(xf, (0, Tp * S - T)) if Tp * S != T else xf
        xs = xs.view(B, Tp, S)
        y = xs[:, 1:].reshape(B, L * S).contiguous()  # targets
        inp = xs[:, :-1].transpose(0, 1).contiguous().view(L * B, S)  # time-major inputs
        emb = ops.mlp(inp, [m for m in self.embedding if isinstance(m, nn.Linear)], ops.ACT_RELU, 0.0).view(L, B, H)

        lens = ops.upload_i32((x_sl_stack - 1).clamp(min=0), dev)
        # nn.LSTM(num_layers = n) on packed sequences (lstm.py:93-101): layer l reads layer l-1's outputs (zero beyond a length),
        # every layer with its own carried state; one K4 sequence launch per layer
        out, hns, cns = emb, [], []
        for l in range(self.num_layers):
            h0 = c0 = None
            if s_0 is not None:
                h0, c0 = s_0[0][l].reshape(B, H).contiguous(), s_0[1][l].reshape(B, H).contiguous()
            w = [getattr(self.lstm, f"{n}_l{l}") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
            out, hn, cn = ops.lstm_sequence(out, h0, c0, lens, *w)
            hns.append(hn)
            cns.append(cn)
        dec_lin = [m for m in self.decoder if isinstance(m, nn.Linear)]

        # mask = arange(L*S) < x_sl  (lstm.py:111): lengths are compared with the SHIFTED target axis
        mask_len = ops.upload_i32(x_sl_host.clamp(max=L * S), dev)
        dec, log_prob = lik.fused_mlp_log_prob(out.view(L * B, H), dec_lin, ops.ACT_RELU, 0.0, y, mask_len, ops.LAYOUT_TIME_MAJOR, B,
                                               L * S, L, S)  # fmt: skip
        log_prob = log_prob.to(torch.float32)
        n_frames = float(x_sl_host.sum())
        loss = -log_prob.sum() / n_frames

        sums = DeferredScalars(torch.stack([loss.detach().double(), log_prob.detach().double().sum()]))
        metrics = [
            LossMetric(sums[0], weight_by=B),
            LLMetric(sums[1], reduce_by=B),
            BitsPerDimMetric(sums[1], reduce_by=n_frames),
        ]
        F = lik.out_features

        def parameters():
            d = dec.detach().view(L, B, S, F).permute(1, 0, 2, 3).reshape(B, L * S, F)
            return lik(d.contiguous())

        lazy = dict(
            _parameters=parameters,
            reconstruction_sample=lambda ns: lik.sample(ns._parameters),
            reconstruction_mode=lambda ns: lik.mode(ns._parameters),
        )
        outputs = LazyNamespace(lazy, loss=loss, ll=log_prob, z=out.transpose(0, 1), z_sl=x_sl_stack,
                                s_n=(torch.stack(hns), torch.stack(cns)))  # fmt: skip
        return loss, metrics, outputs

    @torch.no_grad()
    def generate(self, n_samples: int = 1, max_timesteps: int = 100, use_mode: bool = False, x=None, h0=None, uniforms=None,
                 fused: Optional[bool] = None):  # fmt: skip
        """Free-running sampling: embed the previous stack, one LSTM step through all layers, decode, apply the DMoL head, draw the
        next stack (its mode if `use_mode`) and feed it back, `max_timesteps` times.  The reference declares these arguments
        (lstm.py:133-141) and leaves the body unimplemented.

        x: the start stack [n,S], [n,1,S] or [n,S,1] (one row is repeated to n_samples; None: zeros).  h0: the pair (h_0, c_0), each
        [num_layers,n,H] — exactly `forward`'s s_0 / outputs.s_n (None: zeros).  `forward(prompt, x_sl)` has consumed every stack
        of the prompt but the last, so `generate(x=prompt[:, -S:], h0=outputs.s_n)` continues a prompt.  uniforms = (u
        [T,n,S,num_mix], v [T,n,S]) replays the sampler's draws; otherwise they come from the device RNG.
        Returns ((x [n,T,S,1], x_sl = T per row), ns(s_n=(h_n, c_n))), s_n as `forward` returns it.

        fused=None takes the one-launch path (`ops.lstm_generate`) whenever H is a multiple of 16, num_mix is 10 and
        0 < n <= blvm_pchain_max_batch() (any stack size S >= 1), and falls back to the step-by-step path if the library declines; fused=True insists;
        fused=False runs step by step on the sequence kernels, for any width (hidden sizes that are no multiple of 16 run
        zero-padded), num_mix and batch."""
        S, H, L, lik, n, T = self.stack_size, self.hidden_size, self.num_layers, self.likelihood, int(n_samples), int(max_timesteps)
        K = lik.num_mix
        if n < 1 or T < 0:
            raise ValueError(f"LSTMAudio.generate: n_samples must be positive and max_timesteps non-negative (got {n}, {T})")
        if x is not None:
            if x.dim() == 3 and x.size(1) == 1:
                x = x[:, 0]
            elif x.dim() == 3 and x.size(2) == 1:
                x = x[:, :, 0]
            if x.dim() != 2 or x.size(1) != S or x.size(0) not in (1, n):
                raise ValueError(f"LSTMAudio.generate: x must be one start stack per sample, [{n},{S}], [{n},1,{S}] or [{n},{S},1] "
                                 f"(or one row to repeat); got {tuple(x.shape)}")  # fmt: skip
        if h0 is not None:
            if not (isinstance(h0, (tuple, list)) and len(h0) == 2 and all(torch.is_tensor(t) and tuple(t.shape) == (L, n, H) for t in h0)):
                raise ValueError(f"LSTMAudio.generate: h0 must be the pair (h_0, c_0), each [{L},{n},{H}]")
        if uniforms is not None:
            if not (isinstance(uniforms, (tuple, list)) and len(uniforms) == 2 and all(torch.is_tensor(t) for t in uniforms)
                    and tuple(uniforms[0].shape) == (T, n, S, K) and tuple(uniforms[1].shape) == (T, n, S)):  # fmt: skip
                raise ValueError(f"LSTMAudio.generate: uniforms must be (u [{T},{n},{S},{K}], v [{T},{n},{S}])")
        dev = self.device
        f32 = dict(device=dev, dtype=torch.float32)
        x = torch.zeros(n, S, **f32) if x is None else x.to(**f32).expand(n, S).contiguous()
        h, c = (None, None) if h0 is None else (h0[0].to(**f32).contiguous(), h0[1].to(**f32).contiguous())
        if use_mode:
            u = v = None
        elif uniforms is None:
            u = torch.empty(T, n, S, K, **f32).uniform_(1e-5, 1.0 - 1e-5)
            v = torch.empty(T, n, S, **f32).uniform_(1e-8, 1.0 - 1e-8)
        else:
            u, v = uniforms[0].to(**f32), uniforms[1].to(**f32)
        emb_lin = [m for m in self.embedding if isinstance(m, nn.Linear)]
        dec_lin = [m for m in self.decoder if isinstance(m, nn.Linear)]
        x_sl = torch.full((n,), T, dtype=torch.int)
        if T == 0:  # nothing to draw: the state passes through
            s_n = tuple(torch.zeros(L, n, H, **f32) if t is None else t for t in (h, c))
            return (torch.empty(n, 0, S, 1, **f32), x_sl), SimpleNamespace(s_n=s_n)
        auto = fused is None
        if auto:
            fused = H % 16 == 0 and K == 10 and 0 < n <= ops.load().blvm_pchain_max_batch()
        if fused:
            try:
                xs, h_n, c_n = ops.lstm_generate(emb_lin, self.lstm, dec_lin, lik.params, x, h, c, u, v, S, H, K, lik.log_epsilon, T=T)
                return (xs.unsqueeze(-1), x_sl), SimpleNamespace(s_n=(h_n, c_n))
            except _hip.BlvmHipError:
                # the library validates before it launches, so nothing has run: only an EXPLICIT fused=True insists
                if not auto:
                    raise
        # The sequence kernel takes hidden sizes in multiples of 16: any other width runs zero-padded to the next one.  A padded unit
        # has zero weights and biases and starts at zero, so its c and h stay zero (c' = c / 2 + 0) and nothing reads it through
        # the zero columns of the layer above; the decoder gets the first H columns.
        Hp = (H + 15) // 16 * 16
        pad = torch.nn.functional.pad

        def padded(l):
            wih, whh, bih, bhh = (getattr(self.lstm, f"{k}_l{l}").detach() for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
            if Hp == H:
                return wih, whh, bih, bhh
            cols = Hp - H if l > 0 else 0  # layer 0 reads the embedding (H columns), the layers above a padded state
            return (pad(wih.view(4, H, -1), (0, cols, 0, Hp - H)).reshape(4 * Hp, -1), pad(whh.view(4, H, H), (0, Hp - H, 0, Hp - H)).reshape(4 * Hp, Hp),
                    pad(bih.view(4, H), (0, Hp - H)).reshape(-1), pad(bhh.view(4, H), (0, Hp - H)).reshape(-1))  # fmt: skip

        ws = [padded(l) for l in range(L)]
        hs = [torch.zeros(n, Hp, **f32) if h is None else pad(h[l], (0, Hp - H)) for l in range(L)]
        cs = [torch.zeros(n, Hp, **f32) if c is None else pad(c[l], (0, Hp - H)) for l in range(L)]
        ones = torch.ones(n, dtype=torch.int32, device=dev)
        all_x = []
        for t in range(T):
            out = ops.mlp(x, emb_lin, ops.ACT_RELU, 0.0).view(1, n, H)
            for l in range(L):
                out, hs[l], cs[l] = ops.lstm_sequence(out, hs[l], cs[l], ones, *ws[l])
            dec = ops.mlp(out.view(n, Hp)[:, :H].contiguous(), dec_lin, ops.ACT_RELU, 0.0)
            parameters = lik(dec.view(n, S, lik.out_features))
            xs = lik.mode(parameters) if use_mode else lik.sample(parameters, uniforms=(u[t], v[t]))  # [n,S,1]
            all_x.append(xs)
            x = xs.reshape(n, S)
        return (torch.stack(all_x, dim=1), x_sl), SimpleNamespace(s_n=(torch.stack(hs)[..., :H].contiguous(), torch.stack(cs)[..., :H].contiguous()))
