"""CPU: the switch of the d_enc follower on the VRNN backward walk (include/blvm_hip.h blvm_vrnn_enc_bwd_fold): bound from the header
and read on the host with no device; without a device no call folds, so the workspace is the unfolded one whatever the switch says."""
from ctypes import c_int, c_size_t

from blvm import _hip


def test_the_switch_is_bound_from_the_header():
    lib, sig = _hip.load(), _hip.SIGNATURES
    assert hasattr(lib, "blvm_vrnn_enc_bwd_fold")
    assert sig["blvm_vrnn_enc_bwd_fold"] == (c_int, [c_int])
    assert sig["blvm_vrnn_bwd_workspace_floats"] == (c_size_t, [c_int] * 6)  # (grown inside, where a call would fold: the signature stays)


def test_switch_is_a_host_side_read_and_defaults_to_on():
    lib = _hip.load()
    was = lib.blvm_vrnn_enc_bwd_fold(-1)
    try:
        assert lib.blvm_vrnn_enc_bwd_fold(1) == was and lib.blvm_vrnn_enc_bwd_fold(-1) == 1
        assert lib.blvm_vrnn_enc_bwd_fold(0) == 1 and lib.blvm_vrnn_enc_bwd_fold(-1) == 0
        assert lib.blvm_vrnn_enc_bwd_fold(7) == 0 and lib.blvm_vrnn_enc_bwd_fold(-1) == 1  # (any positive mode: on)
        assert lib.blvm_vrnn_enc_bwd_fold(-2) >= 0 and lib.blvm_vrnn_enc_bwd_fold(-1) == 1  # the counter of folded calls; a query changes nothing
    finally:
        lib.blvm_vrnn_enc_bwd_fold(was)
