"""LSTMBlock: consecutive (bi)directional LSTM layers with the reference's arguments and state_dict (blvm/modules/lstm_block.py:9-82).

A bidirectional layer is ONE K4b call (`ops.lstm_bidir_sequence`): both directions' chains run side by side in one persistent launch
that writes [forward | reverse] straight into the layer's [T,N,2H] output (packed-sequence semantics through the lengths: zeros past a
row's length); the reverse direction is the per-row time reversal that leaves right padding in place
(`utils.operations.reverse_sequences`) folded into the kernel's indexing.  `sum_directions` adds the two halves.  Shapes outside that
call (hidden size not 128 / 256 / 384, T < 4, more tiles than the device has CUs) and unidirectional layers take one K4 sequence call
(`ops.lstm_sequence`) per direction, the reverse one between two `reverse_sequences` gathers, joined by a cat / add.  The dropout
scale is a torch multiply per layer.

Dropout is a scale on the layer's output: `temporal_dropout=True` draws one [1,F] scale per layer and call, `(rand > p) / (1 - p)`,
shared by every frame and row (the reference's 1-d dropout on packed data); False draws it per element.  Training mode only.
`dropout_masks` replaces the draws, as `eps=` / `uniforms=` do in the other models.
"""
from typing import List, Optional

import torch
import torch.nn as nn

from blvm import ops
from blvm.utils.operations import reverse_sequences


class LSTMBlock(nn.Module):
    def __init__(self, input_size: int, hidden_size: int, num_layers: int = 1, bidirectional: bool = True, sum_directions: bool = False,
                 dropout_prob: float = 0.40, temporal_dropout: bool = True, return_all: bool = False):  # fmt: skip
        super().__init__()
        if sum_directions and not bidirectional:
            raise ValueError("LSTM block must be bidirectional to sum directions.")
        self.input_size = input_size
        self.hidden_size = hidden_size
        self.num_layers = num_layers
        self.bidirectional = bidirectional
        self.sum_directions = sum_directions
        self.p = dropout_prob
        self.temporal_dropout = temporal_dropout
        self.return_all = return_all
        self.output_size = hidden_size * (2 if bidirectional and not sum_directions else 1)
        # nn.LSTM is the parameter container only (keys lstm_layers.{i}.weight_ih_l0[_reverse] ...): its forward is never called
        self.lstm_layers = nn.ModuleList()
        for _ in range(num_layers):
            self.lstm_layers.append(nn.LSTM(input_size=input_size, hidden_size=hidden_size, bidirectional=bidirectional))
            input_size = self.output_size

    def _scale(self, like: torch.Tensor, mask: Optional[torch.Tensor]):
        """The dropout scale of one layer's output, or None where the layer passes through."""
        if mask is not None:
            return mask.to(device=like.device, dtype=like.dtype)
        if not self.training or self.p <= 0:
            return None
        shape = (1, like.shape[-1]) if self.temporal_dropout else like.shape
        return (torch.rand(shape, device=like.device) > self.p).to(like.dtype) / (1.0 - self.p)

    def forward(self, input: torch.Tensor, seq_lens: torch.Tensor, dropout_masks: Optional[List[torch.Tensor]] = None):
        """input [T,N,F] float32, seq_lens [N] (any order, 0 allowed) -> (out [T,N,F_out], seq_lens), or the list of every layer's
        output with `return_all`.  dropout_masks: one [1,F_l] scale (or any shape broadcastable to the layer's output) per layer."""
        if dropout_masks is not None and len(dropout_masks) != self.num_layers:
            raise ValueError(f"LSTMBlock: dropout_masks must hold one scale per layer ({self.num_layers}), got {len(dropout_masks)}")
        sl_host = torch.as_tensor(seq_lens).detach().cpu().to(torch.int64)
        T = input.shape[0]
        if sl_host.numel() != input.shape[1] or int(sl_host.min()) < 0 or int(sl_host.max()) > T:
            raise ValueError(f"LSTMBlock: seq_lens must hold one length in [0, T = {T}] per row")
        lens = ops.upload_i32(sl_host, input.device)
        rev_lens = sl_host  # on the host: reverse_sequences builds its index map from it without a device read-back
        x, outputs = input, []
        for i, lstm in enumerate(self.lstm_layers):
            both = None
            if self.bidirectional:
                both = ops.lstm_bidir_sequence(
                    x, lens, (lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0),
                    (lstm.weight_ih_l0_reverse, lstm.weight_hh_l0_reverse, lstm.bias_ih_l0_reverse, lstm.bias_hh_l0_reverse))  # fmt: skip
            if both is not None:
                H = self.hidden_size
                x = both[..., :H] + both[..., H:] if self.sum_directions else both
            elif self.bidirectional:
                fwd = ops.lstm_sequence(x, None, None, lens, lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0)[0]
                xr = _reverse(x, rev_lens)
                bwd = ops.lstm_sequence(xr, None, None, lens, lstm.weight_ih_l0_reverse, lstm.weight_hh_l0_reverse,
                                        lstm.bias_ih_l0_reverse, lstm.bias_hh_l0_reverse)[0]  # fmt: skip
                bwd = _reverse(bwd, rev_lens)
                x = fwd + bwd if self.sum_directions else torch.cat([fwd, bwd], dim=2)
            else:
                x = ops.lstm_sequence(x, None, None, lens, lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0)[0]
            scale = self._scale(x, None if dropout_masks is None else dropout_masks[i])
            if scale is not None:
                x = x * scale
            outputs.append(x)
        if self.return_all:
            return outputs, seq_lens
        return x, seq_lens


def _reverse(x: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
    """reverse_sequences over all T frames of x (it cuts at the longest row; the frames behind it are padding and stay)."""
    T = x.shape[0]
    if lens.numel() == 0 or int(lens.max()) == 0:
        return x
    out = reverse_sequences(x, lens)
    if out.shape[0] < T:
        out = torch.cat([out, x[out.shape[0] :]], dim=0)
    return out.contiguous()
