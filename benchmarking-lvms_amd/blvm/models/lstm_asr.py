"""SimpleLSTMASR: the phoneme / character recognition probe, with the reference's API (blvm/models/lstm_asr.py:14-84).

features [B,I,T] -> LSTMBlock (K4 per direction and layer) -> Linear (K6) -> CTC loss on the un-normalised logits (K9, the
log-softmax is fused), the greedy decode and the word and character error counts on the device (K9): a forward call copies nothing
to the host; the metrics hold deferred scalars and the transcripts are decoded when `outputs.hyps` / `outputs.refs` are read.
"""
from types import SimpleNamespace

import torch
import torch.nn as nn

from blvm import ops
from blvm.data.token_map import BLANK_TOKEN, TokenMap, char_tokenizer, word_tokenizer
from blvm.evaluation import ErrorRateMetric, LossMetric
from blvm.evaluation.metrics import DeferredScalars
from blvm.models.base_model import BaseModel
from blvm.models.vrnn import LazyNamespace
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
        # labels and lengths go to the device once, for the loss and for the error counts
        dev, y = logits.device, torch.as_tensor(y)
        y_dev = y.to(torch.int32) if y.is_cuda else ops.upload_i32(y, dev)
        z_sl_dev, y_sl_dev = ops.upload_i32(z_sl_host.reshape(-1), dev), ops.upload_i32(y_sl_host.reshape(-1), dev)
        nll = ops.ctc_loss(logits, y_dev, z_sl_dev, y_sl_dev, blank=self.blank_index)
        loss = nll.sum() / n_labels

        tables = self.token_map.unit_tables()
        if tables is None or y.dim() != 2 or not ops.edit_distance_fits(y.shape[1], tables):
            return (loss, *self._host_error_rates(logits, z_sl, z_sl_host, y, y_sl_host, loss, n_labels))

        # the loss and both error rates as deferred device scalars: nothing of this call goes to the host until a metric or a
        # transcript is read
        totals, hyp, hyp_lens = ops.ctc_error_totals(logits, z_sl_dev, y_dev, y_sl_dev, tables, blank=self.blank_index)
        tm = self.token_map
        outputs = LazyNamespace(
            dict(hyps=lambda ns: tm.decode_batch(ns._hyp.cpu().tolist(), ns._hyp_lens.cpu().tolist(), " "),
                 refs=lambda ns: tm.decode_batch(ns._y, ns._y_sl, " ")),
            logits=logits.transpose(0, 1), sl=z_sl, _hyp=hyp, _hyp_lens=hyp_lens, _y=y, _y_sl=y_sl_host)  # fmt: skip
        d = DeferredScalars(totals.reshape(-1))  # per table (word, character): edits, reference units, refused rows
        metrics = [
            LossMetric(DeferredScalars(loss.detach().reshape(1))[0], weight_by=n_labels),
            ErrorRateMetric.from_counts((d[0], d[1]), name="wer", invalid=d[2]),
            ErrorRateMetric.from_counts((d[3], d[4]), name="cer", invalid=d[5]),
        ]
        return loss, metrics, outputs

    def _host_error_rates(self, logits, z_sl, z_sl_host, y, y_sl_host, loss, n_labels):
        """(metrics, outputs) by way of strings on the host: for a token map without unit tables (an empty token) and for label rows
        beyond the device distance's limit."""
        hyps_raw = ops.ctc_greedy(logits, z_sl_host, blank=self.blank_index)
        hyps = self.token_map.decode_batch(hyps_raw, [len(h) for h in hyps_raw], " ")
        refs = self.token_map.decode_batch(y, y_sl_host, " ")

        outputs = SimpleNamespace(logits=logits.transpose(0, 1), sl=z_sl, hyps=hyps, refs=refs)
        metrics = [
            LossMetric(loss, weight_by=n_labels),
            ErrorRateMetric(refs, hyps, word_tokenizer, name="wer"),
            ErrorRateMetric(refs, hyps, char_tokenizer, name="cer"),
        ]
        return metrics, outputs
