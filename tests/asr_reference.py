"""The ASR probe composed from stock torch modules, for the tests of SimpleLSTMASR: `nn.LSTM` on packed sequences + `nn.Linear` +
`log_softmax` + `ctc_loss`, with the module tree (and so the state_dict keys) of `blvm.models.SimpleLSTMASR`."""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence


class TorchASR(nn.Module):
    def __init__(self, output_size, input_size, hidden_size, num_layers=1, bidirectional=False, sum_directions=False):
        super().__init__()
        self.hidden_size, self.sum_directions = hidden_size, sum_directions
        width = hidden_size * (2 if bidirectional and not sum_directions else 1)
        self.lstm = nn.Module()
        self.lstm.lstm_layers = nn.ModuleList()
        for _ in range(num_layers):
            self.lstm.lstm_layers.append(nn.LSTM(input_size=input_size, hidden_size=hidden_size, bidirectional=bidirectional))
            input_size = width
        self.output = nn.Linear(width, output_size)

    def forward(self, x, x_sl, y, y_sl, blank=0, scales=None):
        """x [B,I,T]; scales: one multiplier per layer output (the dropout masks), broadcastable to [T,B,F_l].
        Returns (loss, logits [B,T,O], per-layer outputs [T,B,F_l])."""
        x = x.permute(2, 0, 1)
        T = x.shape[0]
        layers = []
        for i, lstm in enumerate(self.lstm.lstm_layers):
            packed = pack_padded_sequence(x, x_sl.cpu(), enforce_sorted=False)
            x = pad_packed_sequence(lstm(packed)[0], total_length=T)[0]
            if self.sum_directions:
                x = x.view(T, x.shape[1], 2, self.hidden_size).sum(2)
            if scales is not None:
                x = x * scales[i].to(x.dtype)
            layers.append(x)
        logits = self.output(x)
        nll = F.ctc_loss(logits.log_softmax(2), y, x_sl, y_sl, blank=blank, reduction="none", zero_infinity=False)
        return nll.sum() / y_sl.sum(), logits.transpose(0, 1), layers
