"""GPU: every kernel ("arm") the K6 GEMM chooses among, run once per case of tests/gemm_arms.py and compared element by element
with float64.

`blvm_gemm_f32` and `blvm_wgrad_group_f32` pick one of 17 kernels per call (include/blvm_hip.h numbers them).  For every case:
the launch counters (`blvm_gemm_arm_counts`, incremented beside each kernel launch) must move by exactly one, on the arm that the
host routing function (`blvm_gemm_arm` / `blvm_wgrad_group_route`) predicts and the table names, so a routing change cannot move a
case onto another kernel unnoticed (tests/test_gemm_arms_cpu.py asserts the same predictions and the table's coverage without a GPU).

Reference: the float64 product of the same operands plus the epilogue; in the 16-bit modes the operands are first rounded to the
type (bias, gate and C are not).  Inputs are drawn in fp32 from a seeded generator and widened exactly.

Acceptance, with the project's existing bars: per element |got - ref| <= 2e-6 (sum_k |a||b| + 1e-3 max|ref|), the form and value of
test_gpu_wgrad_tiles.py::_check, and relative L2 over the output <= 2e-6, or 3e-6 with accumulate or a split (test_gpu_parity.py;
3e-6 is also test_gpu_wgrad_sliced.py's bar for the sliced body).  A plain fp32 `torch.matmul` of the same inputs with the epilogue
in fp32, evaluated on the CPU for every case of the table, stays inside the per-element bound with a worst ratio of 0.21 (K = 0:
0, exact), so no case needs an exemption; the kernels' own worst ratio on an MI355X is 0.20 (fp32 128 x 192), 0.10 in the 16-bit
modes, 0.03 on the sliced body.  Without tolerance: the sentinel columns behind every row of C keep their bits, the
output is finite, and a second run of an unsplit case gives the same bits.  A miss reports the worst element's row and column,
its tile and its position inside the tile, and the ratio to the bound; all misses of a case are collected before asserting."""
import contextlib
import ctypes

import pytest
import torch

import gemm_arms as G
from blvm import _hip, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _require_hip():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    lib = _hip.load()
    assert lib.blvm_device_ok() == 1, "libblvm_hip: no gfx950 device visible"
    before = lib.blvm_gemm_ws_min_rows(-1)  # the built-in row threshold, whatever an earlier module left
    assert lib.blvm_gemm_ws_min_rows(-1) == G.WS_MIN_ROWS
    yield
    lib.blvm_gemm_ws_min_rows(before)
    torch.cuda.synchronize()
    _hip.check_async()


@contextlib.contextmanager
def operand_mode(mode):
    _hip.set_operand_dtype(G.MODE_NAMES[mode])
    try:
        yield
    finally:
        _hip.set_operand_dtype("f32")


def arm_counts():
    buf = (ctypes.c_ulonglong * G.ARMS)()
    _hip.check(_hip.load().blvm_gemm_arm_counts(buf), "blvm_gemm_arm_counts")
    return list(buf)


@contextlib.contextmanager
def expect_arms(what, want):
    """The launches inside the block: exactly `want` = {arm: launches}, and no other arm moved."""
    before = arm_counts()
    yield
    delta = {a: n - b for a, (n, b) in enumerate(zip(arm_counts(), before)) if n != b}
    took = ", ".join(f"{G.arm_name(a)} x{n}" for a, n in delta.items()) or "nothing"
    print(f"{what}: launched {took}")
    assert delta == want, f"{what}: expected {', '.join(f'{G.arm_name(a)} x{n}' for a, n in want.items())}; the counters report {took}"


class Checks:
    """Collects every figure of a case (printed) and every miss; `done()` asserts there was none."""

    def __init__(self, tag):
        self.tag, self.failures = tag, []

    def elements(self, name, got, ref, scale, tile, l2_bar, tol=G.TOL):
        got = got.detach().double().cpu()
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        if not bool(torch.isfinite(got).all()):
            self.failures.append(f"{name}: {int((~torch.isfinite(got)).sum())} non-finite values")
            return
        ratio = (got - ref).abs() / (tol * (scale + 1e-3 * ref.abs().max())).clamp_min(1e-300)
        if ratio.numel() == 0:
            return
        k = int(ratio.argmax())
        r, c = (k // ratio.shape[1], k % ratio.shape[1]) if ratio.dim() == 2 else (k, 0)
        worst = float(ratio.flatten()[k])
        where = f"row {r}, column {c} (tile {r // tile[0]}, {c // tile[1]}; {r % tile[0]}, {c % tile[1]} inside it)"
        l2 = float((got - ref).norm() / (ref.norm() + 1e-30))
        print(f"{self.tag} {name}: worst element ratio {worst:.3f} at {where}; rel_l2 {l2:.3e} (bar {l2_bar:.0e})")
        if worst > 1.0:
            bad = ratio > 1.0
            rows = torch.nonzero(bad.any(1) if ratio.dim() == 2 else bad).flatten().tolist()
            self.failures.append(f"{name}: {int(bad.sum())} elements past the bound, worst {worst:.2f} x the bound at {where}: got "
                                 f"{float(got.flatten()[k]):.8g}, want {float(ref.flatten()[k]):.8g}; rows {rows[:8]}{'...' if len(rows) > 8 else ''}")  # fmt: skip
        if l2 > l2_bar:
            self.failures.append(f"{name}: rel_l2 {l2:.3e} > {l2_bar:.0e}")

    def exact(self, name, ok):
        if not bool(ok):
            self.failures.append(f"{name}: not bit for bit")

    def done(self):
        torch.cuda.synchronize()
        assert not self.failures, f"{self.tag}:\n  " + "\n  ".join(self.failures)


def _launch(c, dev):
    ops.gemm(c.op_a, c.op_b, c.M, c.N, c.K, dev["A"], c.ld_a, dev["B"], c.ld_b, dev["C"], c.ldc, bias=dev["bias"], act=c.act, slope=G.SLOPE,
             gate=dev["gate"], ldg=c.ldg, accumulate=c.acc, split_k=c.split)  # fmt: skip


def _upload(c, d):
    """Device copies with the case's offsets and leading dimensions: the views are rebuilt on the uploaded buffers."""
    dev = {}
    for k, shape, ld, off in (("A", c.a_shape, c.ld_a, c.a_off), ("B", c.b_shape, c.ld_b, c.b_off)):
        buf = d[k + "_buf"].to(DEV)
        dev[k + "_buf"] = buf
        dev[k] = buf[off:]  # (ops.gemm takes the address; the leading dimension travels beside it)
        assert (dev[k].data_ptr() % 16 == 0) == (off % 4 == 0), "the allocator's alignment"
    dev["C"] = d["C"].to(DEV)
    dev["bias"] = None if d["bias"] is None else d["bias"].to(DEV)
    dev["gate"] = None if d["gate"] is None else d["gate"].to(DEV)
    return dev


@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c.name)
def test_gemm_case_runs_its_arm_and_matches_float64(c):
    lib = _hip.load()
    assert G.predict(lib, c) == c.arm, "the routing function and the table disagree (tests/test_gemm_arms_cpu.py)"
    d = G.make_inputs(c, seed=G.CASES.index(c))
    ref, scale = G.reference(c, d)
    dev = _upload(c, d)
    chk = Checks(f"{c.name} [{G.arm_name(c.arm)}]")
    with operand_mode(c.mode):
        with expect_arms(c.name, {c.arm: 1}):
            _launch(c, dev)
        torch.cuda.synchronize()
        out = dev["C"].clone()
        if c.split == 1:  # one fp32 fma chain per output in a fixed order: a second run gives the same bits
            dev["C"].copy_(d["C"])
            _launch(c, dev)
            torch.cuda.synchronize()
            chk.exact("second run", torch.equal(dev["C"].view(torch.int32), out.view(torch.int32)))
    chk.elements("C", out[:, : c.N], ref, scale, G.arm_tile(c.arm), G.rel_l2_bar(c))
    chk.exact("sentinel columns", torch.equal(out[:, c.N :].cpu().view(torch.int32), d["C"][:, c.N :].view(torch.int32)))
    for k in ("A", "B"):  # the operands are read only
        chk.exact(f"{k} unchanged", torch.equal(dev[k + "_buf"].cpu(), d[k + "_buf"]))
    chk.done()


@pytest.mark.parametrize("g", G.GROUP_CASES, ids=lambda g: g.name)
def test_group_case_runs_its_arms_and_matches_float64(g):
    gen = torch.Generator().manual_seed(5000 + G.GROUP_CASES.index(g))
    host, jobs = [], []
    for M, N, off, has_db in g.jobs:
        Dbuf = torch.randn(off + g.rows * M + 4, generator=gen)
        A = torch.randn(g.rows, N, generator=gen)
        dW0, db0 = torch.randn(M, N, generator=gen) * 3.0, torch.randn(M, generator=gen)
        host.append((Dbuf[off : off + g.rows * M].view(g.rows, M), A, dW0, db0 if has_db else None))
        Dd = Dbuf.to(DEV)[off : off + g.rows * M].view(g.rows, M)
        assert (Dd.data_ptr() % 16 == 0) == (off % 4 == 0)
        jobs.append((Dd, A.to(DEV), dW0.to(DEV), db0.to(DEV) if has_db else None))
    want = {}
    for a in ([g.arm] if g.arm != G.NONE else []) + list(g.fallback):
        want[a] = want.get(a, 0) + 1
    chk = Checks(f"{g.name} [{', '.join(G.arm_name(a) for a in want)}]")
    with operand_mode(g.mode):
        with expect_arms(g.name, want):
            ops.wgrad_group(jobs, g.rows)
        torch.cuda.synchronize()
    for i, ((D, A, dW0, db0), (_, _, dW, db), joined) in enumerate(zip(host, jobs, g.joins)):
        Dr, Ar = G.rounded(D, g.mode), G.rounded(A, g.mode)
        arm = g.arm if joined else g.fallback[sum(1 for j in g.joins[:i] if j == 0)]
        chk.elements(f"job {i} dW {tuple(dW.shape)}", dW, Dr.t() @ Ar + dW0.double(), Dr.abs().t() @ Ar.abs(), G.arm_tile(arm), 3e-6)
        if db is not None:  # the bias gradient stays an fp32 sum of the unrounded values in every mode
            chk.elements(f"job {i} db", db, D.double().sum(0) + db0.double(), D.double().abs().sum(0), (G.arm_tile(arm)[0], 1), 3e-6)
    chk.done()
