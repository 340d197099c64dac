"""GPU: the weight-stationary path of the K6 GEMM (csrc/gemm_ws.hip: forward / data-gradient forms with K <= 256; a wave keeps a
16-column slab of the weight in registers and streams 16-row blocks of the activations through v_mfma_f32_16x16x4_f32) through
`ops.gemm`, against float64 on the CPU.

Bounds.  `rel_l2 < 2e-6`, what tests/test_gpu_parity.py holds K6 to.  Per element
`|C - ref| <= (K + 3) * 2^-24 * (|A| . |B| + |bias|)`: an fp32 fma chain of length K plus the epilogue's roundings, each at most half an ulp = 2^-24 relative of a partial result that |A| . |B| + |bias| bounds (the
activation and the gate scale value and bound alike by |slope| <= 1).  Under `accumulate` the previous contents are one more term
of the sum and enter the magnitude.

Shapes: M in {1, 15, 16, 17, 33, 300} (fewer rows than a block, partial last block, several row ranges), N in {16, 48, 256, 272}
(one slab, fewer slabs than a workgroup has waves, more than one workgroup of columns), K in {16, 64, 192, 256}.  The row threshold
of the routing is lowered to 1 for this module through `blvm_gemm_ws_min_rows`, and the path counter (`blvm_gemm_path_counts`)
shows which path every call took."""
import ctypes
import itertools

import pytest
import torch

from blvm import _hip, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0**-24
MS, NS, KS = (1, 15, 16, 17, 33, 300), (16, 48, 256, 272), (16, 64, 192, 256)


@pytest.fixture(autouse=True, scope="module")
def _every_row_count_takes_the_new_path():
    assert torch.cuda.is_available() and _hip.load().blvm_device_ok() == 1
    before = _hip.load().blvm_gemm_ws_min_rows(1)
    yield
    _hip.load().blvm_gemm_ws_min_rows(before)
    _hip.check_async()


def counts():
    c = (ctypes.c_ulonglong * 2)()
    assert _hip.load().blvm_gemm_path_counts(c) == 0
    return c[0], c[1]


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


class Case:
    """One product: operands with the requested paddings (CPU, fp32), its float64 reference and its error magnitude."""

    def __init__(self, M, N, K, op_b, seed, bias=True, act=ops.ACT_NONE, gate=False, accumulate=False, pa=0, pb=0, pc=0, b_off=0, a_off=0):
        g = torch.Generator().manual_seed(seed)
        self.M, self.N, self.K, self.op_b, self.act, self.accumulate = M, N, K, op_b, act, accumulate
        self.slope = 0.01 if (act == ops.ACT_LEAKY or gate) else 0.0
        self.A_full = torch.randn(M, a_off + K + pa, generator=g)  # A = columns a_off .. a_off + K
        self.A = self.A_full[:, a_off : a_off + K]
        # op_b = 0: W[N, K] inside [N, K + pb]; op_b = 1: W[K, N] = columns b_off .. b_off + N of a [K, b_off + N + pb] matrix
        self.B_full = torch.randn(N, b_off + K + pb, generator=g) if op_b == 0 else torch.randn(K, b_off + N + pb, generator=g)
        self.B = self.B_full[:, b_off : b_off + K] if op_b == 0 else self.B_full[:, b_off : b_off + N]
        self.bias = torch.randn(N, generator=g) if bias else None
        self.gate = None
        if gate:  # negative, zero and positive entries
            self.gate = torch.randn(M, N + 4, generator=g)
            self.gate[torch.rand(M, N + 4, generator=g) < 0.2] = 0.0
        self.C0 = torch.randn(M, N + pc, generator=g)
        Bt = (self.B.t() if op_b == 0 else self.B).double()
        ref = self.A.double() @ Bt
        mag = self.A.double().abs() @ Bt.abs()
        if bias:
            ref, mag = ref + self.bias.double(), mag + self.bias.double().abs()
        if act == ops.ACT_RELU:
            ref = ref.clamp(min=0.0)
        elif act == ops.ACT_LEAKY:
            ref = torch.where(ref > 0, ref, self.slope * ref)
        if gate:
            ref = ref * torch.where(self.gate[:, :N].double() > 0, 1.0, self.slope)
        if accumulate:
            ref, mag = ref + self.C0[:, :N].double(), mag + self.C0[:, :N].double().abs()
        self.ref, self.mag = ref, mag

    def run(self, fill=None, expect_path=1):
        """-> the whole output buffer [M, N + pc] (prefilled with `fill`, or with C0 under accumulate)."""
        dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
        A_full, B_full, gate = dev(self.A_full), dev(self.B_full), dev(self.gate)
        A, B = A_full.view(-1)[self.A.storage_offset() :], B_full.view(-1)[self.B.storage_offset() :]  # (flat: contiguous views)
        C = dev(self.C0.clone()) if fill is None else torch.full_like(self.C0, fill, device=DEV)
        before = counts()
        ops.gemm(0, self.op_b, self.M, self.N, self.K, A, A_full.shape[1], B, B_full.shape[1], C, C.shape[1], bias=dev(self.bias),
                 act=self.act, slope=self.slope, gate=gate, ldg=0 if gate is None else gate.shape[1], accumulate=self.accumulate)  # fmt: skip
        after = counts()
        took = (after[0] - before[0], after[1] - before[1])
        assert took == ((0, 1) if expect_path == 1 else (1, 0)), f"path counts moved by {took}"
        return C.cpu()

    def check(self, C, what="", elementwise=True):
        got = C[:, : self.N].double()
        err = (got - self.ref).abs()
        bound = (self.K + 3) * U * self.mag
        worst = float((err / bound.clamp(min=1e-300)).max())
        r = rel_l2(got, self.ref)
        print(f"{what} M={self.M} N={self.N} K={self.K} op_b={self.op_b}: rel_l2 {r:.3e}, worst err / bound {worst:.3f}")
        assert r < 2e-6, (what, r)
        assert not elementwise or bool((err <= bound).all()), (what, worst)

    def check_fresh(self, what=""):
        """Non-accumulating: onto NaN and onto zeros, equal results, padding columns untouched, and the bounds."""
        c_nan, c_zero = self.run(fill=float("nan")), self.run(fill=0.0)
        assert torch.equal(c_nan[:, : self.N], c_zero[:, : self.N]), what
        assert bool(c_nan[:, self.N :].isnan().all()) and bool((c_zero[:, self.N :] == 0).all()), what
        self.check(c_nan, what)
        return c_nan


@pytest.mark.parametrize("op_b", [0, 1])
def test_every_shape_plain_product_with_bias(op_b):
    for n, (M, N, K) in enumerate(itertools.product(MS, NS, KS)):
        Case(M, N, K, op_b, seed=1000 * op_b + n, pc=0 if n % 2 else 4).check_fresh("shape")


@pytest.mark.parametrize("op_b", [0, 1])
@pytest.mark.parametrize("act", [ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LEAKY])
@pytest.mark.parametrize("bias", [False, True])
def test_epilogue_and_leading_dimensions(op_b, act, bias):
    """lda > K, ldb wider than the used columns (op_b = 1: W + offset inside a wider matrix, as the decoder's data gradient reads
    `post_w[0] + R`), ldc > N; with and without the gate mask."""
    for n, (M, N, K) in enumerate([(33, 48, 64), (300, 272, 256), (17, 256, 192), (1, 16, 16)]):
        for gate in (False, True):
            Case(M, N, K, op_b, seed=77 + n, bias=bias, act=act, gate=gate, pa=4, pb=8, pc=12, b_off=16 if op_b else 0).check_fresh("epilogue")


@pytest.mark.parametrize("op_b", [0, 1])
def test_unaligned_weight_gate_and_output_rows(op_b):
    """Only A has to be 16-byte aligned: odd leading dimensions and offsets of B, of the gate and of C take the 4-byte accesses."""
    for n, (M, N, K) in enumerate([(33, 48, 64), (300, 272, 256)]):
        c = Case(M, N, K, op_b, seed=5 + n, act=ops.ACT_LEAKY, gate=True, pb=3, pc=5, b_off=1)
        c.gate = torch.cat([c.gate, torch.ones(M, 1)], 1)  # ldg = N + 5
        c.check_fresh("unaligned")


@pytest.mark.parametrize("op_b", [0, 1])
def test_accumulate_onto_random_contents(op_b):
    for n, (M, N, K) in enumerate([(15, 16, 16), (33, 48, 192), (300, 272, 256), (300, 256, 64)]):
        for gate in (False, True):
            c = Case(M, N, K, op_b, seed=300 + n, act=ops.ACT_NONE, gate=gate, accumulate=True, pc=8)
            C = c.run()
            assert torch.equal(C[:, N:], c.C0[:, N:])  # padding columns untouched
            c.check(C, "accumulate")
            assert torch.equal(c.run(), C)  # bit-identical run to run


@pytest.mark.parametrize("op_b", [0, 1])
def test_bit_identical_to_the_staged_tiles(op_b):
    """Both paths run one fp32 fma chain per output in ascending k, so the same product gives the same bits on either: routing
    a product to the new path changes no result.  (The row threshold decides the path; everything else is the same call.)"""
    lib = _hip.load()
    for n, (M, N, K) in enumerate([(300, 272, 256), (1000, 768, 192), (33, 48, 64), (17, 16, 16)]):
        for kw in (dict(act=ops.ACT_LEAKY), dict(gate=True, bias=False), dict(accumulate=True, bias=False, pc=4)):
            c = Case(M, N, K, op_b, seed=900 + n, **kw)
            fill = None if c.accumulate else float("nan")
            new = c.run(fill=fill)
            lowered = lib.blvm_gemm_ws_min_rows(2**31 - 1)
            try:
                old = c.run(fill=fill, expect_path=0)
            finally:
                lib.blvm_gemm_ws_min_rows(lowered)
            assert torch.equal(new[:, :N], old[:, :N]), (M, N, K, kw)


@pytest.mark.parametrize("op_b", [0, 1])
def test_twice_is_bit_identical(op_b):
    for n, (M, N, K) in enumerate([(300, 272, 256), (300, 256, 192), (33, 48, 64), (4000, 256, 256)]):
        c = Case(M, N, K, op_b, seed=500 + n, act=ops.ACT_LEAKY, gate=True)
        assert torch.equal(c.check_fresh("twice"), c.run(fill=0.0))


def test_rows_above_the_threshold_route_without_help():
    """The built-in threshold: a product with the flagship's shape class takes the new path, a short one stays staged."""
    lib = _hip.load()
    lowered = lib.blvm_gemm_ws_min_rows(-1)
    try:
        builtin = lib.blvm_gemm_ws_min_rows(-1)
        Case(builtin, 256, 256, 0, seed=9).check_fresh("at the threshold")
        c = Case(builtin - 1, 256, 256, 0, seed=10)
        c.check(c.run(fill=float("nan"), expect_path=0), "below the threshold")
    finally:
        lib.blvm_gemm_ws_min_rows(lowered)


@pytest.mark.parametrize("op_b", [0, 1])
def test_products_outside_the_predicate_stay_staged_and_correct(op_b):
    for what, kw in [("K = 272", dict(M=300, N=256, K=272)), ("K = 50", dict(M=300, N=256, K=50)), ("N = 70", dict(M=300, N=70, K=64)),
                     ("lda % 4 != 0", dict(M=300, N=48, K=64, pa=1)), ("A not 16-byte aligned", dict(M=300, N=48, K=64, pa=3, a_off=1))]:  # fmt: skip
        c = Case(op_b=op_b, seed=40, act=ops.ACT_LEAKY, gate=True, pc=4, **kw)
        c_nan, c_zero = c.run(fill=float("nan"), expect_path=0), c.run(fill=0.0, expect_path=0)
        assert torch.equal(c_nan[:, : c.N], c_zero[:, : c.N]), what
        c.check(c_nan, what, elementwise=False)  # (the staged tiles are held to what they were held to before)


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("op_b", [0, 1])
def test_16_bit_operand_modes_stay_staged(mode, op_b):
    """Products of the ROUNDED operands accumulated in fp32 (tests/test_gpu_bf16.py, test_gpu_f16.py): float64 of the rounded
    operands, rel_l2 < 2e-6 as there."""
    dt = torch.bfloat16 if mode == "bf16" else torch.float16
    c = Case(300, 256, 256, op_b, seed=60, act=ops.ACT_LEAKY)
    Bt = (c.B.t() if op_b == 0 else c.B).to(dt).double()
    ref = c.A.to(dt).double() @ Bt + c.bias.double()
    ref = torch.where(ref > 0, ref, c.slope * ref)
    _hip.set_operand_dtype(mode)
    try:
        C = c.run(fill=float("nan"), expect_path=0)
    finally:
        _hip.set_operand_dtype("f32")
    assert rel_l2(C[:, : c.N], ref) < 2e-6
