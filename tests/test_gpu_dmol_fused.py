"""GPU (MI355X): the fused DMoL backward (dz + dW + db in one launch, no d_par) against the unfused launches it replaces and the CPU
oracle, and the one-launch ELBO assembly against the torch expression it replaces.

Bars: dz bit-identical to blvm_act_bwd_f32 applied to blvm_dmol_bwd's d_dec (same MFMA chain, same select and multiply); dW / db
whole-tensor rel-L2 against the float64 oracle <= max(4 x the fp32 oracle's, 1e-5) (test_dmol_forward_backward_vs_oracle's bar); two
fused runs bit-identical (fixed-order reduction).  ELBO: 1e-12 relative for the float64 quantities, the float32 vectors exactly the
float32 rounding of the float64 reference.
"""
import pytest
import torch

import blvm_oracle as O
from blvm import _hip, ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NOT_APPLICABLE = _hip.CONSTANTS["BLVM_NOT_APPLICABLE"]
BINS = 2**16


@pytest.fixture(scope="module", autouse=True)
def _require_hip():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert _hip.load().blvm_device_ok() == 1, "libblvm_hip: no gfx950 device visible"


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _inputs(B, T, S, ragged, seed):
    g = torch.Generator().manual_seed(seed)
    Tp = (T + S - 1) // S
    x, x_sl = O.synth_batch(B, T, seed=seed, ragged=ragged)
    x[0, 0], x[1, 1] = 1.0, -1.0
    dec_bm = torch.randn(B, Tp * S, 30, generator=g) * 1.5  # batch-major frames; the sign pattern stands for the activation's
    W, b = torch.randn(30, 30, generator=g) * 0.3, torch.randn(30, generator=g) * 0.1
    gb = torch.randn(B, generator=g)
    return Tp, x, x_sl, dec_bm, W, b, gb


def _oracle_head_grads(dt, dec_bm, W, b, x, x_sl, gb, T):
    d0 = dec_bm.to(dt)
    W0, b0 = (t.to(dt).clone().requires_grad_(True) for t in (W, b))
    lgt, lc, ls = O.dmol_head(d0[:, :T], W0, b0)
    ll = O.dmol_ll(x.to(dt).unsqueeze(-1), lgt, lc, ls, BINS)
    lp = (ll * O.sequence_mask(x_sl, T, torch.float64)).sum(1)
    (lp * gb.double()).sum().backward()
    return W0.grad, b0.grad


def _unfused(dec, W, b, y, x_sl, gb, B, T, Tp, S, slope):
    lib = _hip.load()
    d_dec, d_par, dz = torch.empty_like(dec), torch.empty_like(dec), torch.empty_like(dec)
    _hip.check(lib.blvm_dmol_bwd(_hip.ptr(dec), 1, _hip.ptr(W), _hip.ptr(b), _hip.ptr(y), _hip.ptr(x_sl), _hip.ptr(gb), B, T, Tp, S, 10,
                                 BINS, -7.0, _hip.ptr(d_dec), _hip.ptr(d_par), _hip.stream_ptr()), "blvm_dmol_bwd")  # fmt: skip
    _hip.check(lib.blvm_act_bwd_f32(_hip.ptr(d_dec), _hip.ptr(dec), slope, _hip.ptr(dz), dz.numel(), _hip.stream_ptr()), "blvm_act_bwd_f32")
    return d_dec, dz


def _fused(dec, W, b, y, x_sl, gb, B, T, Tp, S, slope, ws, grads=True):
    lib = _hip.load()
    dz = torch.empty_like(dec)
    dW, db = (torch.full_like(W, 7.0), torch.full_like(b, 7.0)) if grads else (None, None)  # (written, not accumulated)
    rc = lib.blvm_dmol_bwd_fused(_hip.ptr(dec), 1, _hip.ptr(W), _hip.ptr(b), _hip.ptr(y), _hip.ptr(x_sl), _hip.ptr(gb), B, T, Tp, S, 10,
                                 BINS, -7.0, slope, _hip.ptr(dz), _hip.ptr(dW), _hip.ptr(db), _hip.ptr(ws) if grads else None,
                                 _hip.stream_ptr())  # fmt: skip
    return rc, dz, dW, db


@pytest.mark.parametrize("B,T,S,ragged", [
    pytest.param(64, 16000, 64, False, id="False"),
    pytest.param(64, 16000, 64, True, id="True"),
    # several 64-frame units per stack row, T ending half a row early: chunk boundaries inside a row, a last unit wholly past T
    (3, 5 * 128 - 64, 128, True),
    (3, 3 * 256 - 128, 256, True),
    (400, 3 * 256 - 128, 256, True),  # the chunk count capped by the chip's fill: 2 chunks of 6 units
])
def test_fused_backward_vs_unfused_and_oracle(B, T, S, ragged):
    """[64,16000], S = 64, time-major: full-length and ragged lengths; S = 128 and 256 (two and four units per row), ragged."""
    slope = 0.01
    Tp, x, x_sl, dec_bm, W, b, gb = _inputs(B, T, S, ragged, seed=21 + int(ragged))
    dec = dec_bm.view(B, Tp, S * 30).transpose(0, 1).contiguous().view(Tp * B, S * 30).to(DEV)
    Wd, bd, y, xs, gd = W.to(DEV), b.to(DEV), x.to(DEV), x_sl.to(DEV, torch.int32), gb.to(DEV)
    lib = _hip.load()
    ws_floats = lib.blvm_dmol_bwd_fused_workspace_floats(B, Tp, S)
    assert ws_floats > 0
    ws = torch.zeros(ws_floats, device=DEV)

    d_dec, dz_ref = _unfused(dec, Wd, bd, y, xs, gd, B, T, Tp, S, slope)
    rc, dz, dW, db = _fused(dec, Wd, bd, y, xs, gd, B, T, Tp, S, slope, ws)
    assert rc == 0
    assert torch.equal(dz, dz_ref), "dz differs from blvm_act_bwd_f32(blvm_dmol_bwd's d_dec)"
    # no activation in front of the head (negative slope): the plain d_dec; and without dW / db
    rc, dz_plain, _, _ = _fused(dec, Wd, bd, y, xs, gd, B, T, Tp, S, -1.0, ws, grads=False)
    assert rc == 0 and torch.equal(dz_plain, d_dec)
    # same inputs, same workspace (its tickets are zero again): bit-identical dW / db
    rc, dz2, dW2, db2 = _fused(dec, Wd, bd, y, xs, gd, B, T, Tp, S, slope, ws)
    assert rc == 0 and torch.equal(dz2, dz) and torch.equal(dW2, dW) and torch.equal(db2, db)
    assert int(ws[:256].view(torch.int32).abs().sum()) == 0, "tickets not back at zero"

    tW, tb = _oracle_head_grads(torch.float64, dec_bm, W, b, x, x_sl, gb, T)
    rW, rb = _oracle_head_grads(torch.float32, dec_bm, W, b, x, x_sl, gb, T)
    for name, got, r32, tr in (("dW", dW, rW, tW), ("db", db, rb, tb)):
        e, e32 = rel_l2(got, tr), rel_l2(r32, tr)
        print(f"[dmol_fused B={B} T={T} S={S} ragged={ragged}] {name}: rel-L2 vs float64 oracle {e:.3e} (fp32 oracle {e32:.3e}, bar {max(4 * e32, 1e-5):.3e})")
        assert e <= max(4 * e32, 1e-5), (name, e, e32)


def test_fallback_when_rows_path_does_not_apply():
    """S = 5: the fused entry point declines (nothing launched) and the autograd pair takes the general kernels — same numbers as the
    separate MLP and head nodes."""
    B, Tp, S = 3, 7, 5
    T = Tp * S - 2
    _, x, x_sl, dec_bm, W, b, gb = _inputs(B, T, S, True, seed=5)
    dec = dec_bm.view(B, Tp, S * 30).transpose(0, 1).contiguous().view(Tp * B, S * 30).to(DEV)
    Wd, bd, y, xs, gd = W.to(DEV), b.to(DEV), x.to(DEV), x_sl.to(DEV, torch.int32), gb.to(DEV)
    assert _hip.load().blvm_dmol_bwd_fused_workspace_floats(B, Tp, S) == 0
    rc, dz, _, _ = _fused(dec, Wd, bd, y, xs, gd, B, T, Tp, S, 0.01, None, grads=False)
    assert rc == NOT_APPLICABLE
    _check_pair_equals_separate_nodes(B, T, Tp, S, x, x_sl, W, b, gb, rows_path=False)


def _check_pair_equals_separate_nodes(B, T, Tp, S, x, x_sl, W, b, gb, rows_path):
    torch.manual_seed(S)
    lins = [torch.nn.Linear(24, 40), torch.nn.Linear(40, S * 30)]
    for l in lins:
        l.to(DEV)
    xin = torch.randn(Tp * B, 24)
    y, xs, coef = x.to(DEV), x_sl.to(DEV, torch.int32), gb.double().to(DEV)
    got = []
    for fused in (False, True):
        for l in lins:
            l.zero_grad()
        xd = xin.to(DEV).requires_grad_(True)
        Wd, bd = W.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        if fused:
            dec, lp = ops.mlp_dmol_log_prob(xd, lins, Wd, bd, y, xs, 1, B, T, Tp, S, ops.ACT_LEAKY, 0.01, 10, BINS, -7.0)
            assert not dec.requires_grad
        else:
            dec = ops.mlp(xd, lins, ops.ACT_LEAKY, 0.01)
            lp = ops.dmol_log_prob(dec, Wd, bd, y, xs, 1, B, T, Tp, S, 10, BINS, -7.0)
        (lp * coef).sum().backward()
        got.append([lp.detach().clone(), xd.grad.clone(), Wd.grad.clone(), bd.grad.clone()] + [p.grad.clone() for l in lins for p in l.parameters()])
    (lp0, dx0, dW0, db0, *lin0), (lp1, dx1, dW1, db1, *lin1) = got
    # the same kernels either way.  Exact where no atomics are involved (the data gradient chain; the fused kernel's dW / db); the
    # float64 log_prob sums and the split-K weight gradients add in an order that varies from launch to launch, so those are held to
    # a few ulps of their format's sums: 1e-12 (float64) and 1e-5 whole-tensor (fp32, the suite's bar for fp32 gradient sums).
    torch.testing.assert_close(lp1, lp0, rtol=1e-12, atol=0)
    assert torch.equal(dx1, dx0)
    if rows_path:
        assert torch.equal(dW1, dW0) and torch.equal(db1, db0)
    for a, c in zip([dW1, db1] + lin1, [dW0, db0] + lin0):
        assert rel_l2(a, c) <= 1e-5


@pytest.mark.parametrize("S,Tp", [(64, 6), (128, 3), (256, 2)])
def test_autograd_pair_equals_separate_nodes_on_rows_path(S, Tp):
    """S % 64 == 0: MLP(head_gates) + fused head == MLP + head (whose backward is the same kernel without the gate) + blvm_act_bwd_f32.
    T ends 9 frames before the end of the last 64-frame unit."""
    B = 5
    T = Tp * S - 9
    _, x, x_sl, _, W, b, gb = _inputs(B, T, S, True, seed=6)
    _check_pair_equals_separate_nodes(B, T, Tp, S, x, x_sl, W, b, gb, rows_path=True)


@pytest.mark.parametrize("B,kl_raw", [(64, False), (100, True)])
def test_elbo_kernels_vs_torch_expression(B, kl_raw):
    g = torch.Generator().manual_seed(B)
    lp = -(torch.rand(B, generator=g, dtype=torch.float64) * 4e4 + 1e3)
    kld = torch.rand(B, generator=g, dtype=torch.float64) * 300
    kfn = kld + torch.rand(B, generator=g, dtype=torch.float64) * 50
    beta, n_frames, g_up = 0.7, float(B * 16000 - 123), 3.5
    w_elbo = torch.randn(B, generator=g, dtype=torch.float64)
    # the torch expression the kernels replace, float64 on the CPU
    ref_in = [t.clone().requires_grad_(True) for t in (lp, kld, kfn)]
    r_elbo = ref_in[0] - ref_in[1]
    r_loss = -(ref_in[0] - beta * ref_in[2]).sum() / n_frames
    r_sums = torch.stack([r_loss.detach(), r_elbo.detach().sum(), lp.sum(), (kld if kl_raw else kfn).sum()])
    (r_loss * g_up + (r_elbo * w_elbo).sum()).backward()

    dev_in = [t.to(DEV).requires_grad_(True) for t in (lp, kld, kfn)]
    loss, elbo, sums = ops.elbo_assemble(*dev_in, beta, n_frames, kl_raw=kl_raw)
    assert loss.dtype == elbo.dtype == sums.dtype == torch.float64 and loss.dim() == 0 and not sums.requires_grad
    torch.testing.assert_close(loss.detach().cpu(), r_loss.detach(), rtol=1e-12, atol=0)
    torch.testing.assert_close(elbo.detach().cpu(), r_elbo.detach(), rtol=1e-12, atol=0)
    torch.testing.assert_close(sums.cpu(), r_sums, rtol=1e-12, atol=0)
    (loss * g_up + (elbo * w_elbo.to(DEV)).sum()).backward()
    for d, r in zip(dev_in, ref_in):
        torch.testing.assert_close(d.grad.cpu(), r.grad, rtol=1e-12, atol=0)

    # the float32 vectors the DMoL / chain backward kernels read: exactly the float32 rounding of the float64 reference
    lib = _hip.load()
    g64 = torch.empty(3, B, device=DEV, dtype=torch.float64)
    g32 = torch.empty(3, B, device=DEV, dtype=torch.float32)
    g_loss = torch.tensor(g_up, device=DEV, dtype=torch.float64)
    _hip.check(lib.blvm_elbo_bwd(_hip.ptr(g_loss), _hip.ptr(w_elbo.to(DEV)), beta, n_frames, B, _hip.ptr(g64), _hip.ptr(g32), _hip.stream_ptr()), "blvm_elbo_bwd")
    for i, r in enumerate((ref_in[0].grad, ref_in[2].grad, ref_in[1].grad)):  # g_b | c_fn | c_raw
        assert torch.equal(g32[i].cpu(), r.to(torch.float32))
        assert torch.equal(g64[i].cpu(), r)
    # the loss gradient alone (what a training step sends): c_raw is zero
    _hip.check(lib.blvm_elbo_bwd(_hip.ptr(g_loss), None, beta, n_frames, B, _hip.ptr(g64), _hip.ptr(g32), _hip.stream_ptr()), "blvm_elbo_bwd")
    t = torch.tensor(g_up, dtype=torch.float64) / n_frames
    assert torch.equal(g32[0].cpu(), (-t).to(torch.float32).expand(B)) and torch.equal(g32[1].cpu(), (t * beta).to(torch.float32).expand(B))
    assert float(g32[2].abs().sum()) == 0.0


def test_elbo_backward_vectors_reach_the_consumers_without_a_cast():
    """The float64 gradient the ELBO node returns is recognised by `_grad_f32`, which hands out the kernel's own float32 copy; any other
    tensor takes the cast."""
    B = 64
    ins = [torch.rand(B, device=DEV, dtype=torch.float64).requires_grad_(True) for _ in range(3)]
    seen = {}

    class Probe(torch.autograd.Function):
        @staticmethod
        def forward(ctx, t):
            return t.clone()

        @staticmethod
        def backward(ctx, g):
            seen["g"], seen["f32"] = g, ops._grad_f32(g)
            return g

    loss, _, _ = ops.elbo_assemble(Probe.apply(ins[0]), ins[1], ins[2], 1.0, 1000.0)
    (loss * 2.0).backward()
    twin = ops._F32_TWINS[seen["g"].data_ptr()][2]
    assert seen["f32"].data_ptr() == twin.data_ptr() and seen["f32"].dtype == torch.float32
    assert torch.equal(seen["f32"], seen["g"].to(torch.float32))
    other = seen["g"].clone()
    assert ops._grad_f32(other).data_ptr() != twin.data_ptr()
