"""K9, the fused CTC loss (csrc/ctc.hip) through `ops.ctc_loss` and the C ABI, against torch itself on the CPU in float64:
`log_softmax(2)` + `ctc_loss(reduction="none", zero_infinity=False)`, the gradient taken with respect to the logits.

Bound.  fp32 log-space CTC loses accuracy with T by itself, so no absolute bar is fixed: for every case the test evaluates the same
torch composition in fp32 on the CPU and takes ITS error against float64 on the same inputs; the kernel's error against float64 may be
at most 4 times that (a different summation order of equally long fp32 log-sum-exp chains), never below the project's K4 bars of
1e-5 for values and 2e-5 for gradients.  Relative L2, per tensor AND per batch row.  A row whose reference is zero (no frames)
must be exactly zero, an infinite reference must be +inf, and the gradient is exactly 0.0 at and past a row's input length.
Every figure is printed before it is asserted."""
import pytest
import torch
import torch.nn.functional as F

from blvm import _hip, ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLOOR_VALUE, FLOOR_GRAD, TIMES = 1e-5, 2e-5, 4.0


@pytest.fixture(scope="module", autouse=True)
def _require_hip():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert _hip.load().blvm_device_ok() == 1, "libblvm_hip: no gfx950 device visible"


def torch_ctc(logits, targets, il, tl, blank, dtype, upstream=None):
    """(nll [B], d logits [T,B,C]) of the torch composition on the CPU in `dtype`; upstream [B] weights the rows (None: ones)."""
    x = logits.detach().to(dtype).clone().requires_grad_(True)
    nll = F.ctc_loss(x.log_softmax(2), targets, il, tl, blank=blank, reduction="none", zero_infinity=False)
    w = torch.ones_like(nll) if upstream is None else upstream.to(dtype)
    finite = torch.isfinite(nll.detach())
    (nll[finite] * w[finite]).sum().backward()  # (an infinite row is checked by itself: its gradient is not compared)
    return nll.detach(), x.grad


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def rel(a, r):
    return float((a.double() - r.double()).norm() / r.double().norm())


def compare(name, got, got32, ref, floor, row_dim):
    """got (kernel) and got32 (torch fp32) against ref (float64): per tensor and per slice along row_dim."""
    rows = [(name, got, got32, ref)]
    rows += [(f"{name}[row {b}]", got.select(row_dim, b), got32.select(row_dim, b), ref.select(row_dim, b)) for b in range(ref.shape[row_dim])]
    for label, g, g32, r in rows:
        if not bool(torch.isfinite(r).all()):
            continue
        if float(r.double().norm()) == 0.0:
            assert float(g.double().abs().max()) == 0.0 if g.numel() else True, f"{label}: reference is zero, kernel is not"
            continue
        e, e32 = rel(g, r), rel(g32, r)
        bar = max(TIMES * e32, floor)
        print(f"{label}: kernel {e:.3e}  torch fp32 {e32:.3e}  bar {bar:.3e}")
        assert e <= bar, f"{label}: relative error {e:.3e} above {bar:.3e} (torch fp32: {e32:.3e})"


def run_case(logits, targets, il, tl, blank, upstream=None):
    """The kernel through ops (autograd) on the device; checks it against the float64 composition; returns (nll, grad) on the CPU."""
    il_t, tl_t = torch.tensor(il), torch.tensor(tl)
    ref_nll, ref_g = torch_ctc(logits, targets, il_t, tl_t, blank, torch.float64, upstream)
    f32_nll, f32_g = torch_ctc(logits, targets, il_t, tl_t, blank, torch.float32, upstream)
    x = logits.detach().to(DEV).clone().requires_grad_(True)
    nll = ops.ctc_loss(x, targets, il_t, tl_t, blank=blank)
    w = torch.ones_like(nll) if upstream is None else upstream.to(DEV)
    (nll * w).sum().backward()
    nll, g = nll.detach().cpu(), x.grad.cpu()
    inf_rows = torch.isinf(ref_nll)
    assert torch.equal(torch.isinf(nll) & (nll > 0), inf_rows), f"+inf rows differ: kernel {nll}, reference {ref_nll}"
    fin = ~inf_rows
    if bool(fin.any()):
        compare("nll", nll[fin], f32_nll[fin], ref_nll[fin], FLOOR_VALUE, 0)
        compare("d_logits", g[:, fin], f32_g[:, fin], ref_g[:, fin], FLOOR_GRAD, 1)
    for b, n in enumerate(il):
        assert float(g[n:, b].abs().max() if n < g.shape[0] else 0.0) == 0.0, f"row {b}: gradient not exactly zero past its {n} frames"
        if bool(inf_rows[b]) and n > 0:
            assert not bool(torch.isfinite(g[:n, b]).any()), f"row {b}: an infeasible row's gradient must be non-finite over its frames"
    return nll, g


def random_case(T, B, C, L, blank, seed):
    gen = torch.Generator().manual_seed(seed)
    logits = torch.randn(T, B, C, generator=gen)
    labels = [c for c in range(C) if c != blank]
    targets = torch.tensor(labels)[torch.randint(len(labels), (B, L), generator=gen)]
    return logits, targets


@pytest.mark.parametrize("blank_last", [False, True], ids=["blank0", "blank_last"])
@pytest.mark.parametrize("C", [7, 62, 130])
@pytest.mark.parametrize("L", [31, 32, 64])
def test_state_counts_and_class_counts(L, C, blank_last):
    """S = 2L+1 = 63, 65, 129 states: within a wavefront's lanes, one past, and two per lane; C below, near and above a wavefront."""
    T, blank = 2 * L + 3, (C - 1 if blank_last else 0)
    logits, targets = random_case(T, 2, C, L, blank, seed=L * 1000 + C)
    run_case(logits, targets, [T, T - 2], [L, L - 1], blank)


def repeated_case():
    logits, targets = random_case(9, 3, 7, 5, 0, seed=5)
    targets[0] = 3  # five times the same label: 5 + 4 frames at least
    return logits, targets


def test_repeated_labels_at_minimal_length():
    logits, targets = repeated_case()
    run_case(logits, targets, [9, 9, 7], [5, 5, 3], 0)


def test_infeasible_row_leaves_the_others_alone():
    logits, targets = repeated_case()
    nll_ok, g_ok = run_case(logits, targets, [9, 9, 7], [5, 5, 3], 0)
    nll, g = run_case(logits, targets, [8, 9, 7], [5, 5, 3], 0)
    assert float(nll[0]) == float("inf")
    assert not bool(torch.isfinite(g[:8, 0]).any())
    assert torch.equal(bits(nll[1:]), bits(nll_ok[1:])) and torch.equal(bits(g[:, 1:]), bits(g_ok[:, 1:]))


@pytest.mark.parametrize("lens", [([12, 9, 7, 1, 1], [5, 3, 0, 0, 1]), ([12, 0, 0, 5, 10], [4, 0, 1, 2, 0])], ids=["one_frame", "no_frames"])
def test_ragged_rows(lens):
    il, tl = lens
    logits, targets = random_case(12, 5, 7, 5, 0, seed=11)
    nll, g = run_case(logits, targets, il, tl, 0)
    for b in range(5):
        if il[b] == 0:
            assert float(nll[b]) == (0.0 if tl[b] == 0 else float("inf")) and float(g[:, b].abs().max()) == 0.0


def test_long_sequence():
    """Error growth with T and long scratch strides."""
    logits, targets = random_case(600, 2, 62, 40, 0, seed=600)
    run_case(logits, targets, [600, 571], [40, 33], 0)


def test_upstream_gradient():
    tl = [6, 4, 5]
    logits, targets = random_case(20, 3, 7, 6, 0, seed=3)
    run_case(logits, targets, [20, 17, 12], tl, 0, upstream=torch.full((3,), 1.0 / sum(tl)))


# ---- through the C ABI: loss-only mode, determinism, the caller-owned-buffer contract -------------------------------------------------


def abi_call(logits, targets, il, tl, blank, want_grad=True, fill=0.0):
    T, B, C = logits.shape
    lib = _hip.load()
    f32 = dict(device=DEV, dtype=torch.float32)
    nll = torch.full((B,), fill, **f32)
    g = torch.full((T, B, C), fill, **f32) if want_grad else None
    scratch = torch.full((lib.blvm_ctc_scratch_floats(T, B, C, targets.shape[1]),), fill, **f32)
    _hip.check(
        lib.blvm_ctc_loss(_hip.ptr(logits), _hip.ptr(targets), _hip.ptr(il), _hip.ptr(tl), T, B, C, targets.shape[1], blank, None,
                          _hip.ptr(nll), _hip.ptr(g), _hip.ptr(scratch), _hip.stream_ptr()),
        "blvm_ctc_loss",
    )  # fmt: skip
    torch.cuda.synchronize()
    return nll, g


@pytest.fixture(scope="module")
def abi_inputs():
    logits, targets = random_case(70, 4, 62, 33, 61, seed=70)  # 67 states: two per lane
    i32 = dict(device=DEV, dtype=torch.int32)
    return logits.to(DEV), targets.to(**i32), torch.tensor([70, 69, 40, 0], **i32), torch.tensor([33, 20, 0, 2], **i32), 61


def test_loss_only_mode_gives_the_same_bits(abi_inputs):
    nll, _ = abi_call(*abi_inputs)
    nll_only, _ = abi_call(*abi_inputs, want_grad=False)
    assert torch.equal(bits(nll), bits(nll_only))
    with torch.no_grad():
        nll_ops = ops.ctc_loss(abi_inputs[0], abi_inputs[1], abi_inputs[2], abi_inputs[3], blank=abi_inputs[4])
    assert torch.equal(bits(nll), bits(nll_ops))


def test_two_calls_are_bit_identical(abi_inputs):
    a, b = abi_call(*abi_inputs), abi_call(*abi_inputs)
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))


def test_results_do_not_depend_on_buffer_contents(abi_inputs):
    a, b = abi_call(*abi_inputs, fill=0.0), abi_call(*abi_inputs, fill=float("nan"))
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))
    assert bool(torch.isfinite(b[0][:3]).all()) and bool(torch.isfinite(b[1][:, :3]).all())


def test_label_out_of_range_poisons_its_row_only(abi_inputs):
    logits, targets, il, tl, blank = abi_inputs
    bad = targets.clone()
    bad[1, 3] = 62
    bad[2, 0] = -7  # behind row 2's (empty) target: not a label
    nll_ok, g_ok = abi_call(logits, targets, il, tl, blank)
    nll, g = abi_call(logits, bad, il, tl, blank)
    assert bool(torch.isnan(nll[1])) and bool(torch.isnan(g[:69, 1]).all()) and float(g[69:, 1].abs().max()) == 0.0
    keep = [0, 2, 3]
    assert torch.equal(bits(nll[keep]), bits(nll_ok[keep])) and torch.equal(bits(g[:, keep]), bits(g_ok[:, keep]))


def test_shapes_the_design_cannot_hold_are_refused(abi_inputs):
    logits, targets, il, tl, blank = abi_inputs
    lib = _hip.load()
    for kw in (dict(Lmax=513), dict(C=4097), dict(blank=62), dict(C=1)):
        a = dict(T=70, B=4, C=62, Lmax=33, blank=blank)
        a.update(kw)
        rc = lib.blvm_ctc_loss(_hip.ptr(logits), _hip.ptr(targets), _hip.ptr(il), _hip.ptr(tl), a["T"], a["B"], a["C"], a["Lmax"], a["blank"],
                               None, _hip.ptr(logits), None, _hip.ptr(logits), _hip.stream_ptr())  # fmt: skip
        assert rc == -1, f"{kw}: expected BLVM_EINVAL, got {rc}"


def test_cpu_tensor_is_refused():
    with pytest.raises(_hip.BlvmHipError):
        ops.ctc_loss(torch.zeros(3, 1, 4), torch.zeros(1, 1, dtype=torch.int64), [3], [1])
