"""CPU: the routing predicate of the K6 GEMM (`blvm_gemm_ws_route`, include/blvm_hip.h): which products `blvm_gemm_f32` hands to
the weight-stationary path (csrc/gemm_ws.hip) and which stay on the LDS-staged tiles.  Pure host arithmetic: every condition at its
edges, one condition broken at a time from a product that qualifies."""
import ctypes

import pytest

from blvm import _hip

F32, BF16, F16 = 0, 1, 2
BASE = dict(op_a=0, M=16000, N=256, K=256, a_addr=0x7F0000001000, lda=256, split_k=1, has_colsum=0, operand=F32, min_rows=1024)


def route(**kw):
    a = {**BASE, **kw}
    return _hip.load().blvm_gemm_ws_route(a["op_a"], a["M"], a["N"], a["K"], a["a_addr"], a["lda"], a["split_k"], a["has_colsum"],
                                          a["operand"], a["min_rows"])  # fmt: skip


def test_the_flagship_shapes_qualify():
    assert route() == 1
    for N, K in [(256, 64), (256, 256), (1536, 256), (1920, 256), (768, 256), (192, 192), (16, 16)]:
        assert route(N=N, K=K, lda=K) == 1, (N, K)


@pytest.mark.parametrize("K,want", [(0, 0), (16, 1), (32, 1), (48, 1), (50, 0), (8, 0), (240, 1), (255, 0), (256, 1), (257, 0), (272, 0), (768, 0)])
def test_reduction_length(K, want):
    assert route(K=K, lda=max(K, 4) + (-max(K, 4)) % 4) == want


@pytest.mark.parametrize("N,want", [(0, 0), (15, 0), (16, 1), (17, 0), (48, 1), (70, 0), (256, 1), (272, 1), (30, 0), (1 << 20, 1)])
def test_output_width(N, want):
    assert route(N=N) == want


@pytest.mark.parametrize("M,min_rows,want", [(1023, 1024, 0), (1024, 1024, 1), (1025, 1024, 1), (1, 1, 1), (1, 0, 1), (0, 0, 0), (15, 16, 0), (16, 16, 1)])
def test_row_threshold(M, min_rows, want):
    assert route(M=M, min_rows=min_rows) == want


def test_operand_layout_and_alignment():
    assert route(op_a=1) == 0  # the weight-gradient form and A^T products stay staged
    for lda, want in [(256, 1), (257, 0), (258, 0), (259, 0), (260, 1), (768, 1)]:
        assert route(lda=lda) == want, lda
    for off, want in [(0, 1), (4, 0), (8, 0), (12, 0), (16, 1), (1, 0)]:
        assert route(a_addr=BASE["a_addr"] + off) == want, off


def test_split_colsum_and_operand_type():
    for split, want in [(1, 1), (2, 0), (16, 0)]:
        assert route(split_k=split) == want, split
    assert route(has_colsum=1) == 0
    assert route(operand=BF16) == 0 and route(operand=F16) == 0


def test_threshold_setter_round_trips_without_a_device():
    lib = _hip.load()
    builtin = lib.blvm_gemm_ws_min_rows(-1)
    try:
        builtin = lib.blvm_gemm_ws_min_rows(7)  # (whatever was in force before: now the built-in value for sure)
        assert builtin > 0
        assert lib.blvm_gemm_ws_min_rows(-1) == 7
        assert lib.blvm_gemm_ws_min_rows(-1) == builtin
    finally:
        lib.blvm_gemm_ws_min_rows(-1)


def test_path_counts_is_a_host_side_read():
    lib = _hip.load()
    a, b = (ctypes.c_ulonglong * 2)(2**63 + 7, 2**63 + 7), (ctypes.c_ulonglong * 2)(2**63 + 9, 2**63 + 9)
    assert lib.blvm_gemm_path_counts(a) == 0 and lib.blvm_gemm_path_counts(b) == 0
    assert list(a) == list(b) and max(a) < 2**63
    assert lib.blvm_gemm_path_counts(None) != 0 and b"null" in lib.blvm_last_error()
