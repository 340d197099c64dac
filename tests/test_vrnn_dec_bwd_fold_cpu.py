"""CPU: the entry point and the switch of the decoder leader on the VRNN backward walk (include/blvm_hip.h blvm_vrnn_seq_bwd_dec,
blvm_vrnn_dec_bwd_fold): bound from the header with the signature pinned literally, and read on the host with no device."""
from ctypes import POINTER, c_float, c_int, c_size_t, c_void_p

from blvm import _hip, ops


def test_entry_points_are_bound_from_the_header():
    lib, sig = _hip.load(), _hip.SIGNATURES
    assert all(hasattr(lib, n) for n in ("blvm_vrnn_seq_bwd_dec", "blvm_vrnn_bwd_dec_workspace_floats", "blvm_vrnn_dec_bwd_fold"))
    assert sig["blvm_vrnn_dec_bwd_fold"] == (c_int, [c_int])
    assert sig["blvm_vrnn_bwd_dec_workspace_floats"] == (c_size_t, [c_int] * 8)
    # blvm_vrnn_seq_bwd without d_decin, plus dz3, y1, y2, the three weights, dy2, dy1, DH, SF, slope and the out-flag
    assert sig["blvm_vrnn_seq_bwd_dec"] == (c_int, [POINTER(_hip.VrnnWeights)] + [c_void_p] * 12 + [c_int, c_float] + [c_int] * 7 + [c_float]
                                            + [c_void_p] * 2 + [POINTER(_hip.VrnnGrads)] + [c_void_p] * 7 + [c_int, c_int, c_float, c_void_p, c_void_p])  # fmt: skip
    bwd = sig["blvm_vrnn_seq_bwd"][1]
    assert len(sig["blvm_vrnn_seq_bwd_dec"][1]) == len(bwd) - 1 + 10


def test_switch_is_a_host_side_read_and_defaults_to_on():
    lib = _hip.load()
    was = lib.blvm_vrnn_dec_bwd_fold(-1)
    try:
        assert lib.blvm_vrnn_dec_bwd_fold(1) == was and lib.blvm_vrnn_dec_bwd_fold(-1) == 1
        assert lib.blvm_vrnn_dec_bwd_fold(0) == 1 and lib.blvm_vrnn_dec_bwd_fold(-1) == 0
        assert lib.blvm_vrnn_dec_bwd_fold(7) == 0 and lib.blvm_vrnn_dec_bwd_fold(-1) == 1  # (any positive mode: on)
        assert lib.blvm_vrnn_dec_bwd_fold(-2) >= 0 and lib.blvm_vrnn_dec_bwd_fold(-1) == 1  # the counter of folded calls; a query changes nothing
    finally:
        lib.blvm_vrnn_dec_bwd_fold(was)


def test_the_cell_takes_the_decoder_in_only_when_asked():
    """`DecoderFold` keeps its two-argument form (no head gates: the decoder stays a node of its own)."""
    f = ops.DecoderFold([object()] * 3)
    assert (f.head_gates, f.dec, f.given) == (False, None, None)
    assert ops.DecoderFold([object()] * 3, 0.1, head_gates=True).head_gates is True
