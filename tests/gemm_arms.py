"""The kernels ("arms") of the K6 GEMM as include/blvm_hip.h numbers them (`blvm_gemm_arm`, `blvm_wgrad_group_route`,
`blvm_gemm_arm_counts`), and ONE table of cases that reaches every arm: tests/test_gemm_arms_cpu.py asserts on the host that every
case takes the arm it names and that the table covers what `coverage_wanted()` lists; tests/test_gpu_gemm_arms.py runs every case,
asserts the launch counters and compares each output element with float64.  Here so that files without a GPU can share them.

Shapes are the smallest that reach an arm through the conditions production shapes meet: a wide tile needs M, N >= 128 and
(128-tiles of M) x (128-tiles of N) x split >= 192 -- 5000 x 640 and 5000 x 576 are 40 x 5 = 200 tiles, 5184 x 638 is 41 x 5 -- with
N > 256, and, in fp32 with op_a = 0 and no split, a K the weight-stationary path declines (K > 256 or K % 16 != 0).  No case becomes
`big` through a requested split: every wide case is wide at split 1 already.

Not in the table: the column-sum rider (a bias gradient summed from the staged A tiles) on an (op_a, op_b) = (1, 0) product.  The
ABI gives a caller no way to ask for it: `blvm_gemm_f32` has no column-sum argument, `blvm_wgrad_f32` / `blvm_wgrad_group_f32`
request it on the weight-gradient form (1, 1) only, and that form never takes a wide tile.  The rider is covered where it can
run, on the 64 x 64 tile and on the ring (the grouped cases with db below; tests/test_gpu_wgrad_tiles.py, test_gpu_parity.py)."""
import dataclasses
from typing import Optional, Tuple

import torch

F32, BF16, F16 = 0, 1, 2
MODE_NAMES = ("f32", "bf16", "f16")
T64, T128, T128X192, T192X128 = 0, 1, 2, 3
TILE_DIMS = ((64, 64), (128, 128), (128, 192), (192, 128))
WS, STAGED, WGRAD_EXACT, WGRAD_SLICED, WGRAD_GROUP, GEMM_GROUP, ARMS = 0, 1, 13, 14, 15, 16, 17
NONE = ARMS  # the routing functions' answer "nothing is launched"
WS_MIN_ROWS = 256  # the library's built-in row threshold (csrc/gemm_ws.hip; test_gemm_route_cpu.py reads it back)
LAYOUTS = ((0, 0), (0, 1), (1, 0), (1, 1))
WIDE_LAYOUTS = LAYOUTS[:3]  # the weight-gradient layout (1, 1) never takes a wide tile
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
SLOPE = 0.01
SENTINEL = -123.456  # what the padding columns of C hold
BASE_ADDR = 0x7F0000001000  # an aligned address for the host-only routing calls


def staged(tile, mode=F32):
    return STAGED + 3 * tile + mode


def arm_name(arm):
    if STAGED <= arm < WGRAD_EXACT:
        bm, bn = TILE_DIMS[(arm - STAGED) // 3]
        return f"staged {bm}x{bn} {MODE_NAMES[(arm - STAGED) % 3]}"
    return {WS: "weight-stationary", WGRAD_EXACT: "wgrad exact", WGRAD_SLICED: "wgrad sliced", WGRAD_GROUP: "wgrad group",
            GEMM_GROUP: "gemm group", NONE: "no launch"}[arm]  # fmt: skip


def arm_tile(arm):
    """(rows, columns) of an arm's output tile, for the failure report."""
    if STAGED <= arm < WGRAD_EXACT:
        return TILE_DIMS[(arm - STAGED) // 3]
    return {WS: (16, 16), GEMM_GROUP: (64, 64)}.get(arm, (128, 128))


@dataclasses.dataclass(frozen=True)
class Case:
    """One call of blvm_gemm_f32.  lda / ldb / ldc None: the dense value; ldc_pad columns of SENTINEL behind every row of C;
    a_off / b_off: the operand starts that many floats past a 16-byte boundary; gate: an [M, N] gate with ldg = N + gate_pad."""

    name: str
    op_a: int
    op_b: int
    M: int
    N: int
    K: int
    arm: int
    mode: int = F32
    lda: Optional[int] = None
    ldb: Optional[int] = None
    ldc_pad: int = 4
    a_off: int = 0
    b_off: int = 0
    bias: bool = False
    act: int = ACT_NONE
    gate: bool = False
    gate_pad: int = 8
    acc: bool = False
    split: int = 1
    edges: Tuple[str, ...] = ()

    @property
    def a_shape(self):  # rows, columns of A as stored
        return (self.K, self.M) if self.op_a else (self.M, self.K)

    @property
    def b_shape(self):
        return (self.K, self.N) if self.op_b else (self.N, self.K)

    @property
    def ld_a(self):
        return self.lda if self.lda is not None else max(self.a_shape[1], 1)

    @property
    def ld_b(self):
        return self.ldb if self.ldb is not None else max(self.b_shape[1], 1)

    @property
    def ldc(self):
        return self.N + self.ldc_pad

    @property
    def ldg(self):
        return self.N + self.gate_pad if self.gate else 0

    @property
    def layout(self):
        return (self.op_a, self.op_b)

    @property
    def epilogue(self):
        """The epilogue kinds of the coverage list this case exercises."""
        out = set()
        if self.bias and self.act == ACT_LEAKY:
            out.add("bias+leaky")
        if self.gate and self.gate_pad > 0:
            out.add("gate ldg>N")
        if self.acc and self.split == 1:
            out.add("accumulate")
        if self.split > 1:
            out.add("split accumulate" if self.acc else "split fresh")
        if self.ldc_pad > 0:
            out.add("ldc>N")
        return out

    @property
    def a_vec(self):
        return self.a_off % 4 == 0 and self.ld_a % 4 == 0

    @property
    def b_vec(self):
        return self.b_off % 4 == 0 and self.ld_b % 4 == 0


EPILOGUES = ("bias+leaky", "gate ldg>N", "accumulate", "split fresh", "split accumulate", "ldc>N")
WIDE_SHAPES = {T128: (5000, 640), T128X192: (5000, 576), T192X128: (5184, 638)}  # (M = 39 * 128 + 8: a partial last row tile)


def _pad4(n):
    return (n + 3) // 4 * 4


def _wide_cases():
    """Per wide tile and layout, in fp32: four cases that carry the six epilogue kinds between them; in bf16 and fp16: one case per
    layout with the kinds rotating."""
    out = []
    tn = {T128: "128x128", T128X192: "128x192", T192X128: "192x128"}
    for tile, (M, N) in WIDE_SHAPES.items():
        for op_a, op_b in WIDE_LAYOUTS:
            tag = f"{tn[tile]}_{op_a}{op_b}"
            ld = lambda K: dict(lda=None if op_a else _pad4(K), ldb=None if op_b else _pad4(K))  # noqa: E731
            kinds = [
                # K = 264: 16 whole k-tiles and half of one; every load a 16-byte one where N allows
                ("bl", 264, dict(bias=True, act=ACT_LEAKY)),
                # K = 261 (K % 4 = 1) in rows padded to 264: 16-byte loads whose last one is cut
                ("ga", 261, dict(gate=True, acc=True, **ld(261))),
                # K = 203 dense: k-contiguous operands have an odd leading dimension, so 4-byte loads; the memset path
                ("sf", 203, dict(split=2)),
                ("sa", 520, dict(split=3, acc=True, ldc_pad=0)),
            ]
            for k, K, kw in kinds:
                out.append(Case(f"{tag}_{k}", op_a, op_b, M, N, K, staged(tile), **kw))
            for mode in (BF16, F16):
                i = (tile + 2 * op_a + op_b + mode) % 4
                k, K, kw = kinds[i]
                out.append(Case(f"{tag}_{k}_{MODE_NAMES[mode]}", op_a, op_b, M, N, K, staged(tile, mode), mode=mode, **kw))
    return out


def _edge_cases():
    W, X, Y = staged(T128), staged(T128X192), staged(T192X128)
    return [
        # a K shorter than one k-tile (16 in fp32, 32 in the 16-bit kernels) at N > 256
        Case("128x192_00_k8", 0, 0, 5000, 576, 8, X, bias=True, edges=("K<BK",)),
        Case("192x128_10_k8_bf16", 1, 0, 5184, 638, 8, staged(T192X128, BF16), mode=BF16, bias=True, act=ACT_LEAKY, edges=("K<BK",)),
        # K = 0: the output is the epilogue of zero (bias + ReLU: exact in fp32); A and B stay valid one-column buffers
        Case("128x128_00_k0", 0, 0, 5000, 640, 0, W, bias=True, act=ACT_RELU, lda=4, ldb=4, edges=("K=0",)),
        Case("64x64_01_k0", 0, 1, 100, 36, 0, staged(T64), bias=True, act=ACT_RELU, lda=4, edges=("K=0",)),
        # operands that forbid 16-byte loads: a leading dimension that is no multiple of 4, a pointer one float past alignment
        Case("128x192_00_lda_odd", 0, 0, 5000, 576, 264, X, lda=265, bias=True, act=ACT_LEAKY, edges=("A ld%4",)),
        Case("128x192_10_a_off", 1, 0, 5000, 576, 264, X, a_off=1, gate=True, edges=("A offset",)),
        Case("128x128_01_ldb_odd", 0, 1, 5000, 636, 264, W, ldb=637, gate=True, acc=True, edges=("B ld%4",)),
        Case("128x128_00_b_off", 0, 0, 5000, 636, 264, W, b_off=1, bias=True, act=ACT_LEAKY, edges=("B offset",)),
        Case("192x128_10_lda_odd", 1, 0, 5184, 638, 264, Y, lda=5185, bias=True, act=ACT_LEAKY, edges=("A ld%4",)),
        Case("192x128_01_b_off", 0, 1, 5184, 640, 264, Y, b_off=1, ldb=644, split=2, edges=("B offset",)),
        Case("192x128_00_a_off_f16", 0, 0, 5184, 638, 264, staged(T192X128, F16), mode=F16, a_off=1, lda=268, acc=True, edges=("A offset",)),
        Case("128x192_01_ldb_odd_bf16", 0, 1, 5000, 576, 264, staged(T128X192, BF16), mode=BF16, ldb=577, bias=True, act=ACT_LEAKY,
             edges=("B ld%4",)),  # fmt: skip
        # 16-bit kernels with K a multiple of 16 that fp32 would route weight-stationary
        Case("128x192_00_k256_bf16", 0, 0, 5000, 576, 256, staged(T128X192, BF16), mode=BF16, bias=True, act=ACT_LEAKY, edges=("K%16=0",)),
    ]


def _small_cases():
    S = staged(T64)
    out = [Case(f"64x64_{a}{b}_bl", a, b, 130, 70, 50, S, bias=True, act=ACT_LEAKY) for a, b in LAYOUTS]
    out += [
        # the weight-gradient layout at a shape every other layout runs wide: stays on 64 x 64 (K < 1024: not on the ring either)
        Case("64x64_11_wide_shape", 1, 1, 5000, 640, 264, S, acc=True),
        Case("64x64_11_wide_shape_bf16", 1, 1, 5000, 576, 264, staged(T64, BF16), mode=BF16, acc=True),
        Case("64x64_11_wide_shape_f16", 1, 1, 5184, 638, 264, staged(T64, F16), mode=F16, split=2),
        Case("64x64_11_split", 1, 1, 96, 80, 4099, S, split=16, acc=True),
        Case("64x64_00_f16", 0, 0, 130, 70, 50, staged(T64, F16), mode=F16, gate=True),
        Case("64x64_10_bf16", 1, 0, 130, 70, 50, staged(T64, BF16), mode=BF16, gate=True, acc=True),
        # narrow output with a short reduction (K <= 256 and N <= 256) at a tile count that would be wide otherwise; K % 16 != 0
        Case("64x64_00_narrow", 0, 0, 12290, 256, 100, S, bias=True, act=ACT_LEAKY),
        # weight-stationary, once per op_b (its widths and epilogues are tests/test_gpu_gemm_ws.py's)
        Case("ws_00", 0, 0, 272, 48, 48, WS, bias=True, act=ACT_LEAKY),
        Case("ws_01", 0, 1, 272, 48, 48, WS, gate=True, acc=True),
        # the ring through gemm_f32: M N >= 512^2, rows >= 1024; no split keeps the exact body, a split takes the sliced one
        Case("wgrad_exact", 1, 1, 512, 516, 1037, WGRAD_EXACT),
        Case("wgrad_sliced", 1, 1, 512, 516, 1037, WGRAD_SLICED, split=8, acc=True),
    ]
    return out


CASES = _wide_cases() + _edge_cases() + _small_cases()
assert len({c.name for c in CASES}) == len(CASES)


@dataclasses.dataclass(frozen=True)
class GroupCase:
    """One call of blvm_wgrad_group_f32 over `rows` rows.  jobs: (M = N_out, N = K_in, d_off, has_db); d_off floats past a 16-byte
    boundary for D.  arm: the grouped launch (NONE: there is none); joins: per job, 1 in the grouped launch, 0 through gemm_f32 (its
    arm in `fallback`, in job order)."""

    name: str
    rows: int
    jobs: Tuple[Tuple[int, int, int, bool], ...]
    arm: int
    joins: Tuple[int, ...]
    fallback: Tuple[int, ...] = ()
    mode: int = F32


GROUP_CASES = [
    # two full-tile jobs: 100 % of the 128 x 128 tile area -> the ring; 1037 rows leave a ragged last stage
    GroupCase("group_ring", 1037, ((256, 256, 0, True), (256, 128, 0, False)), WGRAD_GROUP, (1, 1)),
    # 256 x 64 + 2 x 256 x 256: 90 % of the tile area, under the 95 % threshold -> the 64 x 64 group kernel
    GroupCase("group_64_under_95", 1037, ((256, 64, 0, True), (256, 256, 0, True), (256, 256, 0, False)), GEMM_GROUP, (1, 1, 1)),
    # an unaligned job beside a group: it is launched through gemm_f32 and counted on the arm it takes there
    GroupCase("group_ring_and_fallback", 1037, ((256, 256, 0, False), (128, 100, 1, True), (256, 128, 0, True)), WGRAD_GROUP, (1, 0, 1),
              fallback=(staged(T64),)),  # fmt: skip
    # fewer than two jobs fit (rows < 1024): no grouped launch, every job through gemm_f32
    GroupCase("group_none_short_rows", 1000, ((256, 256, 0, True), (128, 132, 0, False)), NONE, (0, 0), fallback=(staged(T64), staged(T64))),
    # a single fitting job that the ring takes through gemm_f32 (M N >= 512^2; the chosen split is 5: the sliced body)
    GroupCase("group_none_single_ring", 1037, ((512, 512, 0, True),), NONE, (0,), fallback=(WGRAD_SLICED,)),
    # the 16-bit modes never group
    GroupCase("group_none_bf16", 1037, ((256, 256, 0, True), (256, 128, 0, False)), NONE, (0, 0),
              fallback=(staged(T64, BF16), staged(T64, BF16)), mode=BF16),  # fmt: skip
]


def pick_split(M, N, K):
    """gemm_pick_split of csrc/common.h: the split blvm_wgrad_f32 and the grouped entry point's per-job path request."""
    tiles = ((M + 63) // 64) * ((N + 63) // 64)
    return max(1, min((768 + tiles - 1) // tiles, (K + 255) // 256))


def predict(lib, c, **override):
    """blvm_gemm_arm for a case (or any request spelled with the same field names)."""
    f = {**{k: getattr(c, k) for k in ("op_a", "op_b", "M", "N", "K", "a_off", "b_off", "split", "bias", "act", "gate", "mode")},
         "lda": c.ld_a, "ldb": c.ld_b, "colsum": False, "min_rows": WS_MIN_ROWS, **override}  # fmt: skip
    return lib.blvm_gemm_arm(f["op_a"], f["op_b"], f["M"], f["N"], f["K"], BASE_ADDR + 4 * f["a_off"], f["lda"], BASE_ADDR + 4 * f["b_off"],
                             f["ldb"], f["split"], int(f["bias"]), f["act"], int(f["gate"]), int(f["colsum"]), f["mode"], f["min_rows"])  # fmt: skip


def coverage_wanted():
    """What the table must reach, generated from the arm numbering: {item: description}.  An item is (arm, layout or None, epilogue
    kind or None)."""
    want = {}
    for tile in (T128, T128X192, T192X128):
        for layout in WIDE_LAYOUTS:
            want[(staged(tile), layout, None)] = "every wide tile in fp32 with every layout it can get"
            for e in EPILOGUES:
                want[(staged(tile), layout, e)] = "every epilogue kind per wide tile and layout in fp32"
    for layout in LAYOUTS:
        want[(staged(T64), layout, None)] = "64 x 64 in all four layouts"
    for arm in (WS, WGRAD_EXACT, WGRAD_SLICED, WGRAD_GROUP, GEMM_GROUP):
        want[(arm, None, None)] = "every other arm"
    for op_b in (0, 1):
        want[(WS, (0, op_b), None)] = "weight-stationary with either op_b"
    for mode in (BF16, F16):
        want[(staged(T64, mode), None, None)] = "every staged tile in bf16 and in fp16"
        for tile in (T128, T128X192, T192X128):
            for layout in WIDE_LAYOUTS:
                want[(staged(tile, mode), layout, None)] = "every wide tile in bf16 and in fp16 with every layout it can get"
    return want


def coverage_reached(cases=None, groups=None):
    cases = CASES if cases is None else cases
    groups = GROUP_CASES if groups is None else groups
    got = set()
    for c in cases:
        got.add((c.arm, None, None))
        if not c.edges:  # (a case that is there for an edge is not what the coverage of a layout or an epilogue rests on)
            got.add((c.arm, c.layout, None))
            got.update((c.arm, c.layout, e) for e in c.epilogue)
    for g in groups:  # (nor is a job that falls back to gemm_f32 what the coverage of that arm rests on)
        if g.arm != NONE:
            got.add((g.arm, None, None))
    return got


# ---- inputs and the float64 reference (CPU tensors; the GPU test uploads them) -----------------------------------------------------


def _strided(rows, cols, ld, off, g, fill=None):
    """A [rows, cols] view, row stride ld, starting `off` floats into a fresh buffer; normal values (or `fill` everywhere)."""
    buf = torch.full((off + max(rows, 1) * ld + 4,), 0.0 if fill is None else fill)
    if fill is None:
        buf.normal_(generator=g)
    return buf, buf[off : off + max(rows, 1) * ld].view(max(rows, 1), ld)[:rows, :cols]


def make_inputs(c, seed=0):
    """{A, B, C (the [M, ldc] buffer, C0 or zeros in front of the sentinel columns), bias, gate}: fp32 CPU tensors from a seeded
    generator; A and B are views at the case's leading dimension and offset into `A_buf`, `B_buf`."""
    g = torch.Generator().manual_seed(1000 + seed)
    d = {}
    d["A_buf"], d["A"] = _strided(*c.a_shape, c.ld_a, c.a_off, g)
    d["B_buf"], d["B"] = _strided(*c.b_shape, c.ld_b, c.b_off, g)
    C = torch.full((c.M, c.ldc), SENTINEL)
    # a destination that is accumulated into holds values; any other holds garbage the kernel must overwrite
    C[:, : c.N] = torch.randn(c.M, c.N, generator=g) * (3.0 if c.acc else 1e3)
    d["C"] = C
    d["bias"] = torch.randn(c.N, generator=g) if c.bias else None
    d["gate"] = torch.randn(c.M, c.ldg, generator=g) if c.gate else None
    return d


def rounded(t, mode):
    """What the kernels of an operand mode multiply, widened exactly."""
    return (t.to(torch.bfloat16) if mode == BF16 else t.half() if mode == F16 else t).double()


def reference(c, d):
    """-> (ref [M, N] float64, scale [M, N] = sum_k |a||b| of the operands as multiplied)."""
    A, B = rounded(d["A"], c.mode), rounded(d["B"], c.mode)
    a = A.t() if c.op_a else A
    b = B if c.op_b else B.t()
    ref, scale = a @ b, a.abs() @ b.abs()
    slope = float(torch.tensor(SLOPE, dtype=torch.float32))  # the slope as the kernels hold it
    if c.bias:
        ref = ref + d["bias"].double()
    if c.act == ACT_RELU:
        ref = ref.clamp_min(0)
    elif c.act == ACT_LEAKY:
        ref = torch.where(ref > 0, ref, slope * ref)
    if c.gate:
        ref = ref * torch.where(d["gate"][:, : c.N] > 0, 1.0, slope).double()
    if c.acc:
        ref = ref + d["C"][:, : c.N].double()
    return ref, scale


TOL = 2e-6  # per element: |got - ref| <= TOL * (sum_k |a||b| + 1e-3 max|ref|), tests/test_gpu_wgrad_tiles.py::_check


def element_bound(ref, scale):
    return TOL * (scale + 1e-3 * ref.abs().max())


def rel_l2_bar(c):
    """The whole-tensor bars of tests/test_gpu_parity.py: 2e-6, 3e-6 with accumulate or a split (also test_gpu_wgrad_sliced.py's)."""
    return 3e-6 if (c.acc or c.split > 1) else 2e-6
