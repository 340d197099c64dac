"""GPU: the sliced weight-gradient tile (csrc/gemm.hip wgrad_tile<true>): every fp32 operand split in registers into three bf16
slices (csrc/bf16_slice.h), a 16-row stage as six v_mfma_f32_32x32x16_bf16 per 32 x 32 output with fp32 accumulation, the terms
a1 b2, a2 b1, a2 b2 dropped.

Routing (gemm.hip, unchanged by the sliced body): a grouped launch takes the tile when >= 2 jobs fit it (16-byte aligned, M, N and
leading dimensions multiples of 4, rows >= 1024) and fill >= 95 % of their 128 x 128 tile area; the single-problem entry points take
it for M N >= 512^2 with split_k != 1 (an unsplit request keeps the exact fp32 body).  The groups below are composed to meet those
rules, so the small outputs the tile must handle (one tile, clamped edge columns, 256 x 64) ride beside a large job; the tile's own
split is min(512 / tiles, rows / 512), so a group of more than 256 tiles runs unsplit (plain epilogue) and a small one at rows >= 2048
split 4 (atomic epilogue).  test_infinite_operand_gives_nan pins that these launches are on the sliced body at all."""
import functools

import numpy as np
import pytest
import torch

from blvm import _hip, ops

gpu = pytest.mark.gpu  # (the NumPy replay of the exact cases below needs no GPU and runs everywhere)
DEV = "cuda:0"
BOUND = 3e-6  # rel-L2 against float64, the bound of the existing weight-gradient tests


def _rel_l2(x, ref):
    return float((x.double() - ref).norm() / ref.norm())


def _rand(rows, cols, seed, ld=None, scale=1.0):
    """[rows, cols] normal data, optionally as a view of a wider (ld) buffer."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    buf = torch.randn(rows, ld or cols, device=DEV, generator=g) * scale
    return buf[:, :cols]


# ---- exact-integer cases -----------------------------------------------------------------------------------------------------------
def _np_slices(x):
    """NumPy replay of slice3: hi / mid / lo as float32 arrays."""
    x = np.asarray(x, dtype=np.float32)
    trunc = lambda v: (v.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)  # noqa: E731
    hi = trunc(x)
    r = (x - hi).astype(np.float32)
    mid = trunc(r)
    lo = (r - mid).astype(np.float32)
    return hi, mid, lo


KEPT = [(0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0)]  # the kernel's term order
DROPPED = [(1, 2), (2, 1), (2, 2)]
ROWS_X, MX = 1024, 128


def _ints(rng, bits, shape):
    """Signed integers with exactly `bits` significant bits and the lowest bit set: every slice the width allows is non-zero."""
    mag = rng.integers(1 << (bits - 1), 1 << bits, size=shape, dtype=np.int64) | 1
    if bits > 16:
        mag |= 1 << 8  # a set bit in the middle slice whatever the random bits are
    return (mag * rng.choice([-1, 1], size=shape)).astype(np.float32)


def _exact_case(name, seed):
    """(D [rows, M], Act [rows, N]) with one operand a selection matrix (one non-zero per column, on distinct rows), the expected
    dW as int64, the value pairs (a, b) of every output, and the kept terms each case must make non-zero."""
    rng = np.random.default_rng(seed)
    rows = rng.permutation(ROWS_X)[:MX]  # the row that carries output column / row c: all 16 k positions, both splits
    wide_bits, sel_bits, terms = {
        "a24_b1": (24, 1, [(0, 0), (1, 0), (2, 0)]),
        "a1_b24": (24, 1, [(0, 0), (0, 1), (0, 2)]),
        "a12_b12": (12, 12, [(0, 0), (0, 1), (1, 0), (1, 1)]),
        "a16_b8": (16, 8, [(0, 0), (1, 0)]),
        "a8_b16": (16, 8, [(0, 0), (0, 1)]),
    }[name]
    full = _ints(rng, wide_bits, (ROWS_X, MX))  # the dense operand: arbitrary on every row (rows the selection skips multiply zeros)
    sel = np.zeros((ROWS_X, MX), dtype=np.float32)
    sval = _ints(rng, sel_bits, MX) if sel_bits > 1 else rng.choice([-1.0, 1.0], size=MX).astype(np.float32)
    sel[rows, np.arange(MX)] = sval
    swap = name in ("a1_b24", "a8_b16")  # the selection matrix is D (the a operand) here, Act otherwise
    D, A = (sel, full) if swap else (full, sel)
    picked = full[rows, :].astype(np.int64)  # [c, j]: the dense operand's row that meets selection column c
    if swap:
        want = sval.astype(np.int64)[:, None] * picked  # dW[m, n] = D[k_m, m] Act[k_m, n]
        a_vals, b_vals = np.broadcast_to(sval[:, None], picked.shape), full[rows, :]
    else:
        want = (picked * sval.astype(np.int64)[:, None]).T  # dW[m, n] = D[k_n, m] Act[k_n, n]
        a_vals, b_vals = full[rows, :].T, np.broadcast_to(sval[None, :], (MX, MX))
    return D, A, want, np.ascontiguousarray(a_vals), np.ascontiguousarray(b_vals), terms


EXACT = ["a24_b1", "a1_b24", "a12_b12", "a16_b8", "a8_b16"]


@functools.lru_cache(maxsize=None)
def _exact_cases():
    return {n: _exact_case(n, 500 + i) for i, n in enumerate(EXACT)}


@pytest.mark.parametrize("name", EXACT)
def test_exact_reference_needs_only_the_kept_terms(name):
    """CPU part of the exact cases: for the chosen inputs the six kept slice products sum to a b exactly (in the kernel's order, every
    partial sum below 2^24), the three dropped ones are all zero, and the terms this case is there for are non-zero."""
    _, _, want, a, b, terms = _exact_cases()[name]
    sa, sb = _np_slices(a), _np_slices(b)
    for s in (*sa, *sb):
        assert not (s.view(np.uint32) & np.uint32(0xFFFF)).any(), "a slice is not bf16-exact"
    acc = np.zeros(a.shape, dtype=np.float32)
    for i, j in KEPT:
        acc = (acc + (sa[i] * sb[j]).astype(np.float32)).astype(np.float32)
        assert np.abs(acc.astype(np.float64)).max() < 2**24
    assert np.array_equal(acc.astype(np.int64), a.astype(np.int64) * b.astype(np.int64))
    assert np.array_equal(acc.astype(np.int64), want)
    for i, j in DROPPED:
        assert not (sa[i] * sb[j]).any(), f"dropped term a{i} b{j} is not zero"
    for i, j in terms:
        assert (sa[i] * sb[j]).all(), f"kept term a{i} b{j} is zero somewhere"
    covered = {t for n in EXACT for t in _exact_cases()[n][5]}
    assert covered == set(KEPT)


@gpu
def test_exact_integer_products_bit_for_bit():
    """All five exact cases as one grouped launch (5 full tiles, rows 1024: split 2, atomic adds of exact integers onto zeros)."""
    cases = _exact_cases()
    jobs = []
    for n in EXACT:
        D, A = (torch.from_numpy(x).to(DEV) for x in cases[n][:2])
        jobs.append((D, A, torch.zeros(MX, MX, device=DEV), None))
    ops.wgrad_group(jobs, ROWS_X)
    torch.cuda.synchronize()
    for n, (_, _, dW, _) in zip(EXACT, jobs):
        got = dW.cpu().numpy()
        want = cases[n][2].astype(np.float32)
        assert np.array_equal(got, want), f"{n}: {int((got != want).sum())} of {want.size} outputs differ from the integer reference"


@gpu
def test_infinite_operand_gives_nan():
    """The documented non-finite behaviour, which also tells the sliced body from the exact one: x - hi is inf - inf for an infinite
    operand, so its output row is NaN (the exact fp32 chain would give +-inf); every other output stays finite."""
    rows = 1024
    jobs = []
    for i in range(2):
        D, A = _rand(rows, 128, 900 + i).clone(), _rand(rows, 128, 910 + i)
        jobs.append((D, A, torch.zeros(128, 128, device=DEV), None))
    jobs[0][0][517, 3] = float("inf")
    ops.wgrad_group(jobs, rows)
    torch.cuda.synchronize()
    dW = jobs[0][2]
    assert bool(torch.isnan(dW[3]).all()), "an infinite operand must give NaN on the sliced tile"
    keep = torch.ones(128, dtype=torch.bool, device=DEV)
    keep[3] = False
    assert bool(torch.isfinite(dW[keep]).all()) and bool(torch.isfinite(jobs[1][2]).all())


# ---- random data against float64 ---------------------------------------------------------------------------------------------------
def _group_jobs(rows, big, scale=1.0, ones=True):
    """(D, Act, dW0, db0) of a group on the sliced tile: a big square job with ld > width, one full tile accumulating onto ones,
    132 x 36 (clamped edge columns in M and N), 256 x 64 without db, and a job without dW."""
    shapes = [(big, big, True, 8), (128, 128, True, 0), (132, 36, True, 4), (256, 64, False, 0)]
    jobs = []
    for i, (M, N, bias, extra) in enumerate(shapes):
        D = _rand(rows, M, 10 * i + 1, ld=M + extra, scale=scale)
        A = _rand(rows, N, 10 * i + 2, ld=N + 2 * extra)
        dW0 = torch.ones(M, N, device=DEV) if (ones and i == 1) else torch.zeros(M, N, device=DEV)
        jobs.append((D, A, dW0, torch.zeros(M, device=DEV) if bias else None))
    jobs.append((_rand(rows, 64, 77, scale=scale), _rand(rows, 32, 78), None, torch.zeros(64, device=DEV)))
    return jobs


def _check_group(jobs, rows):
    refs = []
    for D, A, dW, db in jobs:
        w = None if dW is None else D.double().t() @ A.double() + dW.double()
        b = None if db is None else D.double().sum(0) + db.double()
        refs.append((w, b))
    ops.wgrad_group(jobs, rows)
    torch.cuda.synchronize()
    for i, ((D, A, dW, db), (w, b)) in enumerate(zip(jobs, refs)):
        if dW is not None:
            e = _rel_l2(dW, w)
            print(f"rows {rows} job {i} {tuple(dW.shape)} rel_l2 dW {e:.3e}")
            assert e < BOUND, f"job {i} {tuple(dW.shape)}: rel_l2 {e:.3e}"
        if db is not None:
            e = _rel_l2(db, b)
            print(f"rows {rows} job {i} rel_l2 db {e:.3e}")
            assert e < BOUND, f"job {i} db: rel_l2 {e:.3e}"


@gpu
@pytest.mark.parametrize("rows", [1024, 1037])
def test_group_unsplit_whole_and_ragged_stages(rows):
    """261 tiles: the tile's split is 1 (plain read-add-store epilogue); 1024 rows are 64 whole stages, 1037 leave a ragged stage of
    13 rows."""
    _check_group(_group_jobs(rows, 2048), rows)


@gpu
def test_group_split_atomic_epilogue():
    """69 tiles at 2051 rows: split 4, k ranges of 33 stages, the last one 29 stages and 3 rows; atomic epilogue."""
    _check_group(_group_jobs(2051, 1024), 2051)


@gpu
@pytest.mark.parametrize("scale", [1e-20, 1e15])
def test_group_scaled_operands(scale):
    """The random case with D scaled: slices keep the operand's exponent, nothing under- or overflows at these sizes."""
    _check_group(_group_jobs(2051, 1024, scale=scale, ones=False), 2051)


@gpu
@pytest.mark.parametrize("M,N,rows,split_k", [(512, 516, 2051, 0), (644, 412, 1037, 8), (512, 512, 1024, 0)])
def test_single_problem_entry_points(M, N, rows, split_k):
    """blvm_wgrad_f32 (with db) and blvm_gemm_f32 (op_a = op_b = 1) at M N >= 512^2 with a split requested: ragged M and N, ld larger
    than the width, accumulation onto ones."""
    D, A = _rand(rows, M, 31, ld=M + 4), _rand(rows, N, 32, ld=N + 8)
    ref = D.double().t() @ A.double() + 1.0
    dW = torch.ones(M, N + 4, device=DEV)[:, :N]
    db = torch.zeros(M, device=DEV)
    lib = _hip.load()  # (strided views: the pointers travel as addresses, the leading dimensions beside them)
    _hip.check(lib.blvm_wgrad_f32(M, N, rows, D.data_ptr(), D.stride(0), A.data_ptr(), A.stride(0), dW.data_ptr(), dW.stride(0),
                                  db.data_ptr(), split_k, ops.stream_ptr()), "blvm_wgrad_f32")  # fmt: skip
    C = torch.ones(M, N, device=DEV)
    _hip.check(lib.blvm_gemm_f32(1, 1, M, N, rows, D.data_ptr(), D.stride(0), A.data_ptr(), A.stride(0), C.data_ptr(), N, None, 0, 0.0,
                                 None, 0, 1, max(split_k, 2), ops.stream_ptr()), "blvm_gemm_f32")  # fmt: skip
    torch.cuda.synchronize()
    e_w, e_c, e_b = _rel_l2(dW, ref), _rel_l2(C, ref), _rel_l2(db, D.double().sum(0))
    print(f"{M}x{N}x{rows}: rel_l2 wgrad {e_w:.3e} gemm {e_c:.3e} db {e_b:.3e}")
    assert e_w < BOUND and e_c < BOUND and e_b < BOUND


@gpu
@pytest.mark.parametrize("split_k", [0, 8])
def test_single_problem_takes_the_sliced_body(split_k):
    """Pins the routing that test_single_problem_entry_points relies on: blvm_wgrad_f32 and blvm_gemm_f32 at 512 x 512 with a split
    (chosen there: 9, or requested) give NaN, not inf, for an infinite operand, so both run the sliced body."""
    M = N = 512
    rows = 1024
    D, A = _rand(rows, M, 41).clone(), _rand(rows, N, 42)
    D[300, 5] = float("inf")
    dW, C = torch.zeros(M, N, device=DEV), torch.zeros(M, N, device=DEV)
    lib = _hip.load()
    _hip.check(lib.blvm_wgrad_f32(M, N, rows, D.data_ptr(), M, A.data_ptr(), N, dW.data_ptr(), N, None, split_k, ops.stream_ptr()),
               "blvm_wgrad_f32")  # fmt: skip
    _hip.check(lib.blvm_gemm_f32(1, 1, M, N, rows, D.data_ptr(), M, A.data_ptr(), N, C.data_ptr(), N, None, 0, 0.0, None, 0, 1,
                                 max(split_k, 2), ops.stream_ptr()), "blvm_gemm_f32")  # fmt: skip
    torch.cuda.synchronize()
    keep = torch.ones(M, dtype=torch.bool, device=DEV)
    keep[5] = False
    for out in (dW, C):
        assert bool(torch.isnan(out[5]).all()), "an infinite operand must give NaN on the sliced tile"
        assert bool(torch.isfinite(out[keep]).all())
