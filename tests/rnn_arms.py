"""The dispatch arms of the LSTM / GRU sequence entry points as `blvm_rnn_path_counts` numbers them, and the length patterns of
tests/test_gpu_rnn_sequences.py; here so that files without a GPU can share them."""
import torch

REGS, PROGRAM, PER_STEP = 0, 1, 2


def sorted_lens(T_, B):
    """Descending, >= 1, the first row full: what pack_padded_sequence accepts."""
    return torch.tensor([max(1, T_ - (k * T_) // B) for k in range(B)], dtype=torch.int64)


def zero_row(B):
    """The row of length 0 of `unsorted_lens`: the middle of the last row tile (the partial one when B is no multiple of 16)."""
    r0 = 16 * ((B - 1) // 16)
    return r0 + (B - 1 - r0) // 2


def unsorted_lens(T_, B, with_zero=True):
    """What LSTMAudio produces, `(x_sl_stack - 1).clamp(min=0)`: unsorted; lens[0] = T; one row of length 1; with_zero: one row of
    length 0 inside the last row tile (B = 1 has room for the full row only)."""
    lens = torch.tensor([1 + (7 * b + 3) % T_ for b in range(B)], dtype=torch.int64)
    lens[0] = T_
    if B == 1:
        return lens
    z = zero_row(B) if with_zero and B >= 3 else -1
    one = B - 1 if B - 1 != z else 1
    lens[one] = 1
    if z >= 0:
        lens[z] = 0
    return lens
