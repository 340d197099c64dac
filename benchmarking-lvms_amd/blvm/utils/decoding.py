"""Host-side CTC decoding (reference: blvm/utils/decoding.py:5-29).  `ops.ctc_greedy` is the device twin the model uses."""
import numpy as np
import torch


def greedy_ctc(logits, seq_lens, blank: int = 0):
    """logits [T,B,D] (tensor or array) -> per row the arg-max label of each of its first seq_lens[b] frames (lowest index on a tie),
    repeats collapsed, blanks dropped: a list of lists of ints."""
    if isinstance(logits, torch.Tensor):
        logits = logits.detach().cpu().numpy()
    if isinstance(seq_lens, torch.Tensor):
        seq_lens = seq_lens.tolist()
    best = np.asarray(logits).argmax(axis=2).T  # [B,T]
    decoded = []
    for row, n in zip(best, seq_lens):
        row = row[: int(n)]
        first = np.ones(len(row), dtype=bool)  # True where a run of equal labels starts
        first[1:] = row[1:] != row[:-1]
        kept = row[first]
        decoded.append(kept[kept != blank].tolist())
    return decoded
