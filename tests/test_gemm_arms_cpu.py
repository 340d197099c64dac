"""CPU: which kernel every K6 request takes (`blvm_gemm_arm`, `blvm_wgrad_group_route`: the host functions `blvm_gemm_f32` and
`blvm_wgrad_group_f32` dispatch through) -- the case table of tests/gemm_arms.py arm by arm, what the table covers, the benchmark's
shapes, and every routing condition broken at its edge, one at a time.  No device is touched."""
import ctypes
import dataclasses

import pytest

import gemm_arms as G
from blvm import _hip
from gemm_arms import BF16, F16, F32, T64, T128, T128X192, T192X128, Case, staged


def lib():
    return _hip.load()


def arm(op_a, op_b, M, N, K, colsum=False, min_rows=G.WS_MIN_ROWS, **kw):
    """The arm of a dense, aligned request without epilogue (fields of `Case` override)."""
    return G.predict(lib(), Case("probe", op_a, op_b, M, N, K, -1, **kw), colsum=colsum, min_rows=min_rows)


def group_route(g):
    n = len(g.jobs)
    ints, addrs = (ctypes.c_int * n), (ctypes.c_size_t * n)
    joins = ints(*([7] * n))
    got = lib().blvm_wgrad_group_route(n, ints(*[j[0] for j in g.jobs]), ints(*[j[1] for j in g.jobs]), g.rows,
                                       addrs(*[G.BASE_ADDR + 4 * j[2] for j in g.jobs]), ints(*[j[0] for j in g.jobs]),
                                       addrs(*[G.BASE_ADDR] * n), ints(*[j[1] for j in g.jobs]), ints(*[1] * n), g.mode, joins)  # fmt: skip
    return got, tuple(joins)


# ---- the table -----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c.name)
def test_every_case_takes_the_arm_it_names(c):
    got = G.predict(lib(), c)
    assert got == c.arm, f"{c.name}: routed to {G.arm_name(got)}, the table says {G.arm_name(c.arm)}"
    if staged(T128) <= c.arm < G.WGRAD_EXACT:  # a wide case is wide at split 1 already, not through the split it requests
        assert ((c.M + 127) // 128) * ((c.N + 127) // 128) >= 192, c.name


@pytest.mark.parametrize("g", G.GROUP_CASES, ids=lambda g: g.name)
def test_every_group_case_takes_the_arm_it_names(g):
    got, joins = group_route(g)
    assert (got, joins) == (g.arm, g.joins)
    fallback = [arm(1, 1, M, N, g.rows, a_off=off, split=G.pick_split(M, N, g.rows), mode=g.mode, colsum=db)
                for (M, N, off, db), j in zip(g.jobs, joins) if j == 0]  # fmt: skip
    assert tuple(fallback) == g.fallback


def test_group_route_reports_jobs_without_dw_and_the_job_limit():
    n = 22  # more than the 20 jobs a group holds: the last two go one by one
    ints, addrs = (ctypes.c_int * n), (ctypes.c_size_t * n)
    has_dw = [1] * n
    has_dw[3] = 0
    joins = ints()
    got = lib().blvm_wgrad_group_route(n, ints(*[128] * n), ints(*[128] * n), 2048, addrs(*[G.BASE_ADDR] * n), ints(*[128] * n),
                                       addrs(*[G.BASE_ADDR] * n), ints(*[128] * n), ints(*has_dw), F32, joins)  # fmt: skip
    assert got == G.WGRAD_GROUP
    assert list(joins) == [1, 1, 1, -1] + [1] * 17 + [0]
    assert lib().blvm_wgrad_group_route(0, None, None, 2048, None, None, None, None, None, F32, None) == G.NONE


def test_table_covers_every_arm_layout_and_epilogue():
    want, got = G.coverage_wanted(), G.coverage_reached()
    missing = [f"{G.arm_name(a)} layout {l} {e or ''}: {why}" for (a, l, e), why in want.items() if (a, l, e) not in got]
    assert not missing, "the case table does not reach:\n  " + "\n  ".join(missing)
    assert len(want) == 9 * 7 + 4 + 5 + 2 + 2 * (1 + 9)
    assert {a for a, l, e in got if l is None} == set(range(G.ARMS))  # every arm there is has a case
    # the weight-gradient layout never goes wide, in the table ...
    assert not [c.name for c in G.CASES if c.layout == (1, 1) and staged(T128) <= c.arm < G.WGRAD_EXACT]
    assert [c.name for c in G.CASES if c.layout == (1, 1) and c.M >= 5000 and c.arm in (staged(T64), staged(T64, BF16), staged(T64, F16))]


def test_table_covers_the_edges():
    cases = G.CASES
    wide = [c for c in cases if staged(T128) <= c.arm < G.WGRAD_EXACT]
    tags = {t for c in wide for t in c.edges}
    assert tags >= {"K<BK", "K=0", "A ld%4", "A offset", "B ld%4", "B offset"}
    for c in cases:  # the tags say what the fields say: one operand at a time loses its 16-byte loads, by what the tag names
        if "A offset" in c.edges or "A ld%4" in c.edges:
            assert ((c.a_off % 4 != 0, c.ld_a % 4 != 0) == ("A offset" in c.edges, "A ld%4" in c.edges)) and c.b_vec, c.name
        if "B offset" in c.edges or "B ld%4" in c.edges:
            assert ((c.b_off % 4 != 0, c.ld_b % 4 != 0) == ("B offset" in c.edges, "B ld%4" in c.edges)) and c.a_vec, c.name
        if "K<BK" in c.edges:
            assert 0 < c.K < (16 if c.mode == F32 else 32) and c.N > 256, c.name
        if "K=0" in c.edges:
            assert c.K == 0, c.name
    # a partial last tile in the dimension the 192 rule leaves free; on 192 x 128 an N that is no multiple of 4
    assert any(c.arm == staged(T128X192) and c.M % 128 == 8 for c in wide)
    assert any(c.arm == staged(T192X128) and c.N % 4 != 0 and c.N % 128 != 0 for c in wide)
    assert any(c.arm == staged(T128) and c.M % 128 and c.N % 128 for c in wide)
    for tile in (T128, T128X192, T192X128):
        ks = {c.K for c in wide if c.arm == staged(tile)}
        assert any(k % 4 for k in ks) and any(k % 16 and k % 4 == 0 for k in ks), (tile, ks)
    # every case is small enough for a float64 reference
    assert max(c.M * c.N * max(c.K, 1) for c in cases) <= 3e9


WIDE_BLOCK = [c.name for c in G.CASES if staged(T128) <= c.arm < G.WGRAD_EXACT and not c.edges]


@pytest.mark.parametrize("victim", WIDE_BLOCK + ["ws_00", "ws_01", "wgrad_exact", "wgrad_sliced", "64x64_10_bl",
                                                 "group_64_under_95"])  # fmt: skip
def test_coverage_notices_a_deleted_row(victim):
    """Every row of the wide-tile blocks (four epilogue rows per tile and layout in fp32, one row per tile, layout and 16-bit mode)
    and every row that alone holds an arm or a layout is needed: without it the coverage list is no longer met.  (Rows that are
    there for an edge are held by test_table_covers_the_edges.)"""
    assert len(WIDE_BLOCK) == 9 * 4 + 9 * 2 and any(c.name == victim for c in [*G.CASES, *G.GROUP_CASES])
    got = G.coverage_reached([c for c in G.CASES if c.name != victim], [g for g in G.GROUP_CASES if g.name != victim])
    assert [k for k in G.coverage_wanted() if k not in got], f"deleting {victim} leaves the coverage list satisfied"


# ---- what the benchmark runs --------------------------------------------------------------------------------------------------------

VRNN_ROWS, C4_ROWS = 16000, 398848
BENCH = [
    # the VRNN rows of the table at gemm_ws_route (csrc/gemm_ws.hip)
    ("enc L1 forward", dict(op_a=0, op_b=0, M=VRNN_ROWS, N=256, K=64, bias=True, act=2), G.WS),
    ("enc L2 forward", dict(op_a=0, op_b=0, M=VRNN_ROWS, N=256, K=256, bias=True, act=2), G.WS),
    ("XQ forward", dict(op_a=0, op_b=0, M=VRNN_ROWS, N=256, K=256), G.WS),
    ("XG forward", dict(op_a=0, op_b=0, M=VRNN_ROWS, N=1536, K=256), G.WS),
    ("dec L3 forward", dict(op_a=0, op_b=0, M=VRNN_ROWS, N=1920, K=256), G.WS),
    ("dec L2 data gradient", dict(op_a=0, op_b=1, M=VRNN_ROWS, N=256, K=256, gate=True), G.WS),
    ("d_enc from DQ0", dict(op_a=0, op_b=1, M=VRNN_ROWS, N=256, K=256, acc=True), G.WS),
    ("dec L1 data gradient", dict(op_a=0, op_b=1, M=VRNN_ROWS, N=768, K=256), G.WS),
    # the weight-gradient shapes of the table at gemm_arm (csrc/gemm.hip), split as blvm_wgrad_f32 chooses it
    ("wgrad 1536x512x16000", dict(op_a=1, op_b=1, M=1536, N=512, K=VRNN_ROWS, acc=True, split=0), G.WGRAD_SLICED),
    ("wgrad 256x256x16000", dict(op_a=1, op_b=1, M=256, N=256, K=VRNN_ROWS, acc=True, split=0), staged(T64)),
    ("wgrad 768x256x16000", dict(op_a=1, op_b=1, M=768, N=256, K=VRNN_ROWS, acc=True, split=0), staged(T64)),
    ("wgrad 256x256x64000", dict(op_a=1, op_b=1, M=256, N=256, K=64000, acc=True, split=0), G.WGRAD_SLICED),
    ("wgrad 384x192x49152", dict(op_a=1, op_b=1, M=384, N=192, K=49152, acc=True, split=0), G.WGRAD_SLICED),
    ("wgrad 192x192x98304", dict(op_a=1, op_b=1, M=192, N=192, K=98304, acc=True, split=0), staged(T64)),
    # CW-VAE C4: the 1x1 convolutions C -> 4C -> C over 398 848 rows (C = 192)
    ("C4 C->4C forward", dict(op_a=0, op_b=0, M=C4_ROWS, N=768, K=192, bias=True, act=2), G.WS),
    ("C4 4C->C data gradient", dict(op_a=0, op_b=1, M=C4_ROWS, N=768, K=192, gate=True), G.WS),
    ("C4 4C->C forward", dict(op_a=0, op_b=0, M=C4_ROWS, N=192, K=768, bias=True, act=2), staged(T128X192)),
    ("C4 C->4C data gradient", dict(op_a=0, op_b=1, M=C4_ROWS, N=192, K=768, gate=True), staged(T128X192)),
    ("C4 C->4C weight gradient", dict(op_a=1, op_b=1, M=768, N=192, K=C4_ROWS, acc=True, split=0), G.WGRAD_SLICED),
    ("C4 4C->C weight gradient", dict(op_a=1, op_b=1, M=192, N=768, K=C4_ROWS, acc=True, split=0), G.WGRAD_SLICED),
]


@pytest.mark.parametrize("what,req,want", BENCH, ids=[b[0] for b in BENCH])
def test_benchmark_shapes_run_arms_the_table_runs(what, req, want):
    req = dict(req)
    if req.get("split") == 0:
        req["split"] = G.pick_split(req["M"], req["N"], req["K"])
    got = arm(**req)
    assert got == want, f"{what}: {G.arm_name(got)}, pinned {G.arm_name(want)}"
    assert (want, None, None) in G.coverage_reached()
    if staged(T128) <= want < G.WGRAD_EXACT:  # a wide tile: with this layout and this epilogue
        e = "bias+leaky" if req.get("bias") else "gate ldg>N"
        assert (want, (req["op_a"], req["op_b"]), e) in G.coverage_reached()


# ---- every routing condition at its edge ----------------------------------------------------------------------------------------------

W, X, Y, S = staged(T128), staged(T128X192), staged(T192X128), staged(T64)


def test_the_192_tile_threshold():
    # 191 / 192 tiles of 128 x 128 at split 1: 3 column tiles x 63 / 64 row tiles, 1 x 191 / 192 ...
    for M, N, want in [(63 * 128, 384, S), (63 * 128 + 1, 384, W), (64 * 128, 384, W), (191 * 128, 640, W), (38 * 128, 640, S),
                       (38 * 128 + 1, 640, W), (39 * 128, 640, W), (48 * 128, 512, W), (48 * 128 - 128, 512, S)]:  # fmt: skip
        assert arm(0, 0, M, N, 300) == want, (M, N)
    # both dimensions need a whole tile's worth
    assert arm(0, 0, 127, 128 * 200, 300) == S and arm(0, 0, 128, 128 * 192, 300) == W and arm(0, 0, 128 * 192, 127, 300) == S
    # the split counts as requested (the code's rule; no case of the table leans on it)
    assert arm(1, 0, 4 * 128, 3 * 128, 4096, split=15) == S and arm(1, 0, 4 * 128, 3 * 128, 4096, split=16) == W


def test_short_reduction_on_a_narrow_output_stays_on_64x64():
    big = dict(M=12800, mode=BF16)  # (the 16-bit modes: no weight-stationary path in the way)
    for N, K, want in [(256, 256, S + 1), (256, 257, W + 1), (257, 256, W + 1), (256, 0, S + 1), (272, 16, W + 1), (128, 256, S + 1)]:
        assert arm(0, 0, N=N, K=K, **big) == want, (N, K)
    assert arm(0, 0, 12800, 256, 264) == W and arm(0, 0, 12800, 256, 250) == S and arm(0, 0, 12800, 256, 256) == G.WS
    assert arm(0, 0, 12800, 256, 256, a_off=1) == S  # (declined by the weight-stationary path: still K <= 256, N <= 256)


def test_the_192_wide_tiles():
    M = 12800
    for N, want in [(192, X), (384, W), (576, X), (768, W), (960, X), (190, W), (640, W)]:
        assert arm(0, 0, M, N, 300) == want, N
    # 192 x 128 only where 128 x 192 does not apply, and only for M % 192 == 0 with M % 128 != 0
    for M, N, want in [(192 * 67, 640, Y), (192 * 66, 640, W), (192 * 67, 576, X), (192 * 67 + 4, 640, W), (192 * 67, 384, Y)]:
        assert arm(1, 0, M, N, 300) == want, (M, N)
    for layout in G.WIDE_LAYOUTS:
        assert arm(*layout, 12800, 576, 300) == X and arm(*layout, 192 * 67, 640, 300) == Y
    for mode in (F32, BF16, F16):
        assert arm(1, 0, 12800, 576, 300, mode=mode) == X + mode and arm(1, 0, 192 * 67, 640, 300, mode=mode) == Y + mode


def test_the_weight_gradient_layout_never_goes_wide():
    for M, N, K, split in [(12800, 576, 300, 1), (192 * 67, 640, 300, 1), (12800, 640, 300, 1), (12800, 640, 300, 64), (512, 512, 1000, 200)]:
        for mode in (F32, BF16, F16):
            assert arm(1, 1, M, N, K, split=split, mode=mode) == S + mode, (M, N, K, split, mode)


def test_wgrad_wins_and_wgrad_fits():
    # M N >= 512^2 ...
    for M, N, want in [(512, 512, G.WGRAD_EXACT), (512, 508, S), (256, 1024, G.WGRAD_EXACT), (256, 1020, S)]:
        assert arm(1, 1, M, N, 2048) == want, (M, N)
    # ... or K >= 32768 with max(M, N) >= 256
    for M, N, K, want in [(256, 128, 32768, G.WGRAD_EXACT), (256, 128, 32767, S), (252, 128, 32768, S), (128, 256, 32768, G.WGRAD_EXACT)]:
        assert arm(1, 1, M, N, K) == want, (M, N, K)
    # a split request takes the sliced body, no split the exact one
    assert [arm(1, 1, 512, 512, 2048, split=s) for s in (0, 1, 2, 9)] == [G.WGRAD_EXACT, G.WGRAD_EXACT, G.WGRAD_SLICED, G.WGRAD_SLICED]
    # wgrad_fits: K >= 1024, M and N and both leading dimensions multiples of 4, both operands aligned
    ok = dict(op_a=1, op_b=1, M=512, N=516, K=1024)
    assert arm(**ok) == G.WGRAD_EXACT
    for broken in [dict(K=1023), dict(M=514, N=520), dict(M=520, N=514), dict(lda=513), dict(ldb=517), dict(a_off=1), dict(b_off=2)]:
        assert arm(**{**ok, **broken}) == S, broken
    assert arm(**{**ok, "lda": 516, "ldb": 520}) == G.WGRAD_EXACT
    # an epilogue or a 16-bit mode keeps the form on the staged tile
    for broken in [dict(bias=True), dict(act=1), dict(gate=True), dict(mode=BF16), dict(mode=F16)]:
        assert arm(**{**ok, **broken}) == S + broken.get("mode", 0), broken
    assert arm(**ok, colsum=True) == G.WGRAD_EXACT  # (the bias gradient rides on the ring as well)


def test_weight_stationary_arm_agrees_with_its_own_predicate():
    for kw in [dict(), dict(K=264), dict(K=250), dict(split=2), dict(a_off=1), dict(lda=258), dict(N=250), dict(M=255), dict(mode=BF16), dict(op_a=1)]:
        req = {**dict(op_a=0, op_b=0, M=16000, N=256, K=256), **kw}
        c = Case("probe", arm=-1, **req)
        ws = lib().blvm_gemm_ws_route(c.op_a, c.M, c.N, c.K, G.BASE_ADDR + 4 * c.a_off, c.ld_a, c.split, 0, c.mode, G.WS_MIN_ROWS)
        assert (G.predict(lib(), c) == G.WS) == bool(ws), kw
    assert arm(0, 0, 16000, 256, 256, colsum=True) == S and arm(0, 0, 16000, 256, 256, min_rows=16001) == S


def test_empty_products_launch_nothing():
    assert arm(0, 0, 0, 64, 64) == G.NONE and arm(0, 0, 64, 0, 64) == G.NONE and arm(0, 0, 64, 64, 0) == S


def test_group_conditions_at_their_edges():
    base = G.GroupCase("g", 1024, ((256, 256, 0, True), (256, 128, 0, True)), G.WGRAD_GROUP, (1, 1))
    assert group_route(base) == (G.WGRAD_GROUP, (1, 1))
    assert group_route(dataclasses.replace(base, rows=1023)) == (G.NONE, (0, 0))
    assert group_route(dataclasses.replace(base, jobs=((256, 256, 0, True), (256, 126, 0, True)))) == (G.NONE, (0, 0))
    assert group_route(dataclasses.replace(base, jobs=((256, 256, 1, True), (256, 128, 0, True)))) == (G.NONE, (0, 0))
    assert group_route(dataclasses.replace(base, mode=F16)) == (G.NONE, (0, 0))
    # the 95 % rule: 256 x 256 + 256 x 244 fill 500 / 512 = 97.7 % of four + four tiles, 256 x 228 94.5 %
    assert group_route(dataclasses.replace(base, jobs=((256, 256, 0, True), (256, 244, 0, True))))[0] == G.WGRAD_GROUP
    assert group_route(dataclasses.replace(base, jobs=((256, 256, 0, True), (256, 228, 0, True))))[0] == G.GEMM_GROUP


def test_arm_counts_is_a_host_side_read():
    n = G.ARMS
    a, b = (ctypes.c_ulonglong * n)(*[2**63 + 7] * n), (ctypes.c_ulonglong * n)(*[2**63 + 9] * n)
    assert lib().blvm_gemm_arm_counts(a) == 0 and lib().blvm_gemm_arm_counts(b) == 0
    assert list(a) == list(b) and max(a) < 2**63
    assert lib().blvm_gemm_arm_counts(None) != 0 and b"null" in lib().blvm_last_error()
    assert lib().blvm_version() >= 202
    c = _hip.CONSTANTS
    assert (c["BLVM_GEMM_ARM_WS"], c["BLVM_GEMM_ARM_STAGED"], c["BLVM_GEMM_ARM_WGRAD_EXACT"], c["BLVM_GEMM_ARM_WGRAD_SLICED"],
            c["BLVM_GEMM_ARM_WGRAD_GROUP"], c["BLVM_GEMM_ARM_GEMM_GROUP"], c["BLVM_GEMM_ARMS"]) == (
        G.WS, G.STAGED, G.WGRAD_EXACT, G.WGRAD_SLICED, G.WGRAD_GROUP, G.GEMM_GROUP, G.ARMS)  # fmt: skip
