"""CPU: the size functions of the one-launch bidirectional LSTM layer (K4b, include/blvm_hip.h) are host arithmetic — callable
without a device, never below what two unidirectional K4 calls reserve, and non-decreasing in T and B — and the binding knows the
new entry points."""
import ctypes
from ctypes import c_int, c_size_t, c_void_p

from blvm import _hip, ops

# B up to 128, the largest batch of the persistent kernels: past it no size function carves their operand slabs (K4's neither)
GRID_T, GRID_B, WIDTHS = (1, 2, 3, 4, 5, 7, 40), (1, 3, 15, 16, 17, 40, 113, 128), (16, 64, 128, 256, 384, 512)


def test_sizes_cover_two_unidirectional_calls_and_grow_with_the_shape():
    lib = _hip.load()
    pairs = ((lib.blvm_lstm_bidir_reserve_floats, lib.blvm_lstm_reserve_floats),
             (lib.blvm_lstm_bidir_bwd_workspace_floats, lib.blvm_lstm_bwd_workspace_floats))  # fmt: skip
    for both, one in pairs:
        for H in WIDTHS:
            table = [[both(T, B, H) for B in GRID_B] for T in GRID_T]
            for i, T in enumerate(GRID_T):
                for j, B in enumerate(GRID_B):
                    assert table[i][j] >= 2 * one(T, B, H) > 0, (T, B, H)
                    assert table[i][j] % 4 == 0, (T, B, H)  # whole 16-byte pieces: the second direction's buffers stay aligned
                    assert i == 0 or table[i][j] >= table[i - 1][j], (T, B, H)
                    assert j == 0 or table[i][j] >= table[i][j - 1], (T, B, H)


def test_entry_points_are_bound_from_the_header():
    sig = _hip.SIGNATURES
    assert sig["blvm_lstm_bidir_reserve_floats"] == sig["blvm_lstm_bidir_bwd_workspace_floats"] == (c_size_t, [c_int] * 3)
    assert sig["blvm_lstm_bidir_fwd"] == (c_int, [c_void_p] * 10 + [c_int] * 4 + [c_void_p] * 3)
    assert sig["blvm_lstm_bidir_bwd"] == (c_int, [c_void_p] * 8 + [c_int] * 4 + [c_void_p] * 11)
    assert sig["blvm_lstm_bidir_path_counts"] == (c_int, [c_void_p]) and sig["blvm_lstm_bidir_applies"] == (c_int, [c_int] * 3)


def test_sizes_beyond_the_persistent_batch_still_cover_two_calls():
    lib = _hip.load()
    for B in (129, 200):
        assert lib.blvm_lstm_bidir_reserve_floats(5, B, 128) >= 2 * lib.blvm_lstm_reserve_floats(5, B, 128)
        assert lib.blvm_lstm_bidir_bwd_workspace_floats(5, B, 128) >= 2 * lib.blvm_lstm_bwd_workspace_floats(5, B, 128)


def test_path_counts_is_a_host_side_read():
    lib = _hip.load()
    buf = (ctypes.c_ulonglong * 2)(7, 7)
    assert lib.blvm_lstm_bidir_path_counts(buf) == 0 and tuple(buf) == ops.lstm_bidir_path_counts()
    assert lib.blvm_lstm_bidir_path_counts(None) != 0 and b"null" in lib.blvm_last_error()
