"""GPU: the weight-gradient tile (csrc/gemm.hip wgrad_tile: dW[M, N] (+)= D^T Act with D [rows, M], Act [rows, N], both row-major,
staged by LDS-DMA) against float64, through the grouped launch (blvm_wgrad_group_f32) and through blvm_gemm_f32 (op_a = op_b = 1).

Operands the tile cannot take (not 16-byte aligned, rows < 1024) go to the register-staged 64 x 64 tile; both paths are checked, and
an unsplit launch of the two must agree bit for bit: they run the same MFMA k order per output."""
import pytest
import torch

from blvm import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
X = H = Z = 256
R = 512


def _chain_shapes():
    """(M, N, bias) of the VRNN chain's grouped weight gradients at the headline configuration (vrnn.hip)."""
    j = [(3 * R, X, True), (3 * R, H, False), (3 * R, R, True), (H, Z, True)]
    j += [(H, H, True)] * 3 + [(2 * Z, H, True)] * 2 + [(H, H, True)] * 4
    j += [(H, R, True), (H, R, False), (H, X, True)]
    return j


def _ref(D, A, dW0=None, db0=None):
    w = D.double().t() @ A.double()
    if dW0 is not None:
        w += dW0.double()
    b = D.double().sum(0)
    if db0 is not None:
        b += db0.double()
    scale = D.double().abs().t() @ A.double().abs()  # sum |d a| per output: the size of an fp32 sum's rounding error
    return w, b, scale


def _check(dW, ref, scale, tol=2e-6):
    err = (dW.double() - ref).abs()
    bound = tol * (scale + ref.abs().max() * 1e-3)
    worst = float((err / bound).max())
    assert worst <= 1.0, f"dW error {float(err.max()):.3e} exceeds {tol:g} * sum|d a| (worst ratio {worst:.2f})"


def _data(rows, M, N, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(rows, M, device=DEV, generator=g), torch.randn(rows, N, device=DEV, generator=g)


@pytest.mark.parametrize("rows", [16000, 16000 - 5])
def test_chain_group_matches_float64(rows):
    shapes = _chain_shapes()
    jobs, refs = [], []
    for i, (M, N, bias) in enumerate(shapes):
        D, A = _data(rows, M, N, 100 + i)
        dW0 = torch.randn(M, N, device=DEV) * 10  # accumulates into a non-zero gradient
        db0 = torch.randn(M, device=DEV) if bias else None
        jobs.append((D, A, dW0.clone(), db0.clone() if bias else None))
        refs.append(_ref(D, A, dW0, db0))
    ops.wgrad_group(jobs, rows)
    torch.cuda.synchronize()
    for (D, A, dW, db), (w, b, scale), (M, N, bias) in zip(jobs, refs, shapes):
        _check(dW, w, scale)
        if bias:
            bs = D.double().abs().sum(0)
            assert float(((db.double() - b).abs() / (bs * 2e-6 + 1e-6)).max()) <= 1.0, f"db mismatch at {M}x{N}"


@pytest.mark.parametrize("M,N,rows", [(516, 520, 3001), (644, 412, 4000), (200, 132, 16000)])
def test_ragged_tiles_accumulate(M, N, rows):
    """M and N that are not multiples of the 128 tile, through gemm_f32 (the first two take wgrad_tile there: M N >= 512^2) and through
    a group of two (which fills under 95 % of its 128 x 128 tile area: the 64 x 64 group kernel)."""
    D, A = _data(rows, M, N, 7)
    dW0 = torch.randn(M, N, device=DEV)
    w, _, scale = _ref(D, A, dW0)
    for split in (1, 8):
        C = dW0.clone()
        ops.gemm(1, 1, M, N, rows, D, M, A, N, C, N, accumulate=True, split_k=split)
        torch.cuda.synchronize()
        _check(C, w, scale)
    D2, A2 = _data(rows, 64, 100, 8)
    w2, b2, s2 = _ref(D2, A2)
    jobs = [(D, A, dW0.clone(), None), (D2, A2, torch.zeros(64, 100, device=DEV), torch.zeros(64, device=DEV))]
    ops.wgrad_group(jobs, rows)
    torch.cuda.synchronize()
    _check(jobs[0][2], w, scale)
    _check(jobs[1][2], w2, s2)
    assert float(((jobs[1][3].double() - b2).abs() / (D2.double().abs().sum(0) * 2e-6 + 1e-6)).max()) <= 1.0


def test_ragged_group_on_dma_tile():
    """A group that fills >= 95 % of its 128 x 128 tile area (so wgrad_group_kernel runs it) with a ragged M, bias gradients and a
    non-zero dW, at a split and at a ragged row count."""
    for rows in (16000, 6001):
        shapes = [(1532, 512), (1536, 256)]
        jobs, refs = [], []
        for i, (M, N) in enumerate(shapes):
            D, A = _data(rows, M, N, 40 + i)
            dW0, db0 = torch.randn(M, N, device=DEV), torch.randn(M, device=DEV)
            jobs.append((D, A, dW0.clone(), db0.clone()))
            refs.append(_ref(D, A, dW0, db0))
        ops.wgrad_group(jobs, rows)
        torch.cuda.synchronize()
        for (D, A, dW, db), (w, b, scale) in zip(jobs, refs):
            _check(dW, w, scale)
            assert float(((db.double() - b).abs() / (D.double().abs().sum(0) * 2e-6 + 1e-6)).max()) <= 1.0


def test_bias_gradient_rides_on_gemm_f32():
    from blvm import _hip

    M, N, rows = 512, 640, 5000  # (a shape gemm_f32 gives to wgrad_tile)
    D, A = _data(rows, M, N, 11)
    dW = torch.zeros(M, N, device=DEV)
    db = torch.full((M,), 0.5, device=DEV)
    _hip.check(_hip.load().blvm_wgrad_f32(M, N, rows, ops.ptr(D), M, ops.ptr(A), N, ops.ptr(dW), N, ops.ptr(db), 0, ops.stream_ptr()),
               "blvm_wgrad_f32")  # fmt: skip
    torch.cuda.synchronize()
    w, b, scale = _ref(D, A)
    _check(dW, w, scale)
    assert float(((db.double() - 0.5 - b).abs() / (D.double().abs().sum(0) * 2e-6 + 1e-6)).max()) <= 1.0


def _unaligned_copy(t):
    """The same values at an address 4 bytes past a 16-byte boundary (the DMA-staged tile declines it)."""
    buf = torch.empty(t.numel() + 4, device=DEV)
    u = buf[1 : 1 + t.numel()].view(t.shape)
    u.copy_(t)
    assert u.data_ptr() % 16 != 0
    return u


@pytest.mark.parametrize("rows", [4096, 4000 - 3])
def test_unaligned_fallback_and_unsplit_bits(rows):
    M, N = 512, 516  # (gemm_f32 takes wgrad_tile from M N >= 512^2 on)
    D, A = _data(rows, M, N, 21)
    Du = _unaligned_copy(D)
    w, _, scale = _ref(D, A)
    C_new = torch.empty(M, N, device=DEV)
    C_old = torch.empty(M, N, device=DEV)
    ops.gemm(1, 1, M, N, rows, D, M, A, N, C_new, N, accumulate=False, split_k=1)
    ops.gemm(1, 1, M, N, rows, Du, M, A, N, C_old, N, accumulate=False, split_k=1)
    torch.cuda.synchronize()
    _check(C_old, w, scale)
    _check(C_new, w, scale)
    assert torch.equal(C_new, C_old), "unsplit DMA-staged tile differs from the register-staged tile"
    # a group whose only job is unaligned takes the fallback too
    jobs = [(Du, A, torch.zeros(M, N, device=DEV), torch.zeros(M, device=DEV))]
    ops.wgrad_group(jobs, rows)
    torch.cuda.synchronize()
    _check(jobs[0][2], w, scale)


def test_short_reduction_fallback():
    M, N, rows = 256, 256, 1000  # rows < 1024: the 64 x 64 tile
    D, A = _data(rows, M, N, 31)
    jobs = [(D, A, torch.zeros(M, N, device=DEV), None), (A, D, torch.zeros(N, M, device=DEV), None)]
    ops.wgrad_group(jobs, rows)
    torch.cuda.synchronize()
    w, _, scale = _ref(D, A)
    _check(jobs[0][2], w, scale)
    _check(jobs[1][2], w.t(), scale.t())
