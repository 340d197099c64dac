"""SimpleLSTMASR: the phoneme / character recognition probe, with the reference's API (blvm/models/lstm_asr.py:14-84).

features [B,I,T] -> LSTMBlock (K4 per direction and layer) -> Linear (K6) -> CTC loss on the un-normalised logits (K9, the
log-softmax is fused) and the greedy decode on the device (K9); error rates on the host.
"""
from types import SimpleNamespace

import torch
import torch.nn as nn

from blvm import ops
from blvm.data.token_map import BLANK_TOKEN, TokenMap, char_tokenizer, word_tokenizer
from blvm.evaluation import ErrorRateMetric, LossMetric
from blvm.models.base_model import BaseModel
from blvm.modules.lstm_block import LSTMBlock


class SimpleLSTMASR(BaseModel):
    def __init__(self, token_map: TokenMap, input_size: int, hidden_size: int, num_layers: int = 1, bidirectional: bool = False,
                 sum_directions: bool = False, dropout_prob: float = 0.0, temporal_dropout: bool = True):  # fmt: skip
        super().__init__()
        if isinstance(token_map, dict):  # a checkpoint's plain-data form (init_arguments below)
            token_map = TokenMap(**token_map)
        self.token_map = token_map
        self.output_size = len(token_map)
        self.input_size = input_size
        self.hidden_size = hidden_size
        self.num_layers = num_layers
        self.bidirectional = bidirectional
        self.sum_directions = sum_directions
        self.dropout_prob = dropout_prob
        self.temporal_dropout = temporal_dropout
        self.blank_index = token_map.token2index[BLANK_TOKEN]
        self.lstm = LSTMBlock(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers, bidirectional=bidirectional,
                              sum_directions=sum_directions, dropout_prob=dropout_prob, temporal_dropout=temporal_dropout)  # fmt: skip
        self.output = nn.Linear(self.lstm.output_size, self.output_size)

    def init_arguments(self):
        """The token map as plain data, so that `save` / `load` (torch.load(weights_only=True)) round-trip it."""
        args = dict(super().init_arguments())
        tm = self.token_map
        args["token_map"] = dict(tokens=tm.tokens[1:] if tm.add_blank else list(tm.tokens), add_blank=tm.add_blank)
        return args

    def forward(self, x: torch.Tensor, x_sl: torch.Tensor, y: torch.Tensor, y_sl: torch.Tensor, dropout_masks=None):
        """x [B,I,T] float32 features, x_sl [B] frames per row, y [B,Lmax] label indices, y_sl [B] labels per row ->
        (loss, metrics, outputs).  dropout_masks: see LSTMBlock.forward."""
        z, z_sl = self.lstm(x.permute(2, 0, 1).contiguous(), x_sl, dropout_masks=dropout_masks)  # [T,B,I]
        return self.ctc_decoder(z, z_sl, y, y_sl)

    def ctc_decoder(self, z: torch.Tensor, z_sl: torch.Tensor, y: torch.Tensor, y_sl: torch.Tensor):
        """z [T,B,F] time-major representations (the LSTM's, or a frozen model's dumped latents) -> CTC loss per label and error rates."""
        T, B, F = z.shape
        logits = ops.linear(z.reshape(T * B, F), self.output.weight, self.output.bias).view(T, B, self.output_size)
        z_sl_host = torch.as_tensor(z_sl).detach().cpu()
        y_sl_host = torch.as_tensor(y_sl).detach().cpu()
        n_labels = float(y_sl_host.sum())
        nll = ops.ctc_loss(logits, y, z_sl_host, y_sl_host, blank=self.blank_index)
        loss = nll.sum() / n_labels

        hyps_raw = ops.ctc_greedy(logits, z_sl_host, blank=self.blank_index)
        hyps = self.token_map.decode_batch(hyps_raw, [len(h) for h in hyps_raw], " ")
        refs = self.token_map.decode_batch(y, y_sl_host, " ")

        outputs = SimpleNamespace(logits=logits.transpose(0, 1), sl=z_sl, hyps=hyps, refs=refs)
        metrics = [
            LossMetric(loss, weight_by=n_labels),
            ErrorRateMetric(refs, hyps, word_tokenizer, name="wer"),
            ErrorRateMetric(refs, hyps, char_tokenizer, name="cer"),
        ]
        return loss, metrics, outputs
