"""GPU: the placement of the static walk's launches (csrc/vrnn_static.h Place; bits 32 and 64 of `blvm_pchain_tune`) decides WHICH
workgroup computes a tile, never what the tile reads or in which order it sums.  So under every placement — 0 the program's
TileIter mode, 1 plain TileIter, 2 plain TileIter behind the block-index permutation `place_wg` — the VRNN static forward and
backward walks must reproduce the interpreter (`blvm_pchain_static(0)`) bit for bit: loss, per-utterance ELBO and KL, z, h_n, d_h0
and d_enc.

Batches: 49 and 64 (four row tiles: the permutation applies), 17, 33 and 48 (it does not: the launch falls back to placement 1, or
under the default bits to placement 0; tests/host/static_place_test.hip pins which is which).  T' = 3 and 5 at the full widths
H = Z = 256, R = 512, free nats 0 and 2, a row that ends inside step 1 and an empty row on either side of the first tile edge.
Every static case must have run on the static kernels (`blvm_pchain_static(-2)`), and no launch may abort."""
import pytest
import torch

from blvm import _hip
from blvm.models import VRNNAudio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 64   # samples per frame, as bench.py
H = 256  # the static walk is built for H = Z = 256 (R = 512)
EXACT = ["loss", "elbo", "kl", "z", "h_n", "d_h0", "d_enc"]
BASE = 20  # the program's own bits: XCD-aware TileIter mode, canary polls
# placement 2 falls back to 1 where the permutation does not apply (bits 32 | 64); bit 64 alone — the default — falls back to 0
PLACES = {0: BASE, 1: BASE | 32, 2: BASE | 32 | 64, "default": BASE | 64}


def _lib():
    lib = _hip.load()
    assert lib.blvm_device_ok() == 1
    return lib


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(23)
    return VRNNAudio(likelihood="DMoL", input_size=S, hidden_size=H, latent_size=H, residual_posterior=True).to(DEV)


def _batch(B, TP):
    g = torch.Generator().manual_seed(1000 * TP + B)
    T_ = TP * S
    x = (torch.rand(B, T_, generator=g) * 2 - 1).to(DEV)
    x_sl = torch.randint(T_ // 2, T_ + 1, (B,), generator=g, dtype=torch.int64)
    x_sl[0] = T_
    x_sl[1] = S + S // 2      # ends inside step 1
    x_sl[B - 1] = T_ - 1      # (the last row tile's last row is alive)
    x_sl[15] = 0              # an empty row on either side of the first tile edge
    x_sl[16] = 0
    eps = torch.randn(TP, B, H, generator=g).to(DEV)
    h0 = (torch.rand(B, 2 * H, generator=g) * 2 - 1).to(DEV)
    return x, x_sl, eps, h0


def _step(m, batch, free_nats, static, tune):
    """One forward and backward; returns the compared tensors and how many programs ran on the static kernels."""
    lib = _lib()
    was = lib.blvm_pchain_static(1 if static else 0)
    lib.blvm_pchain_tune(tune)
    n0 = lib.blvm_pchain_static(-2)
    cell = m.vrnn.vrnn_cell
    seq, got = cell.sequence, {}

    def tapped(enc, *a, **kw):
        enc.register_hook(lambda g: got.__setitem__("d_enc", g.detach().clone()))
        return seq(enc, *a, **kw)

    try:
        cell.sequence = tapped
        x, x_sl, eps, h0 = batch
        h = h0.clone().requires_grad_(True)
        m.zero_grad(set_to_none=True)
        loss, _, out = m(x, x_sl, beta=1.0, free_nats=free_nats, eps=eps, h0=h)
        loss.backward()
        torch.cuda.synchronize()
        got.update(loss=loss.detach().clone(), elbo=out.elbo.detach().clone(), kl=out.kl.detach().clone(), z=out.z.detach().clone(),
                   h_n=out.h_n.detach().clone(), d_h0=h.grad.detach().clone())
        launches = lib.blvm_pchain_static(-2) - n0
    finally:
        del cell.sequence  # (back to the class's method)
        lib.blvm_pchain_static(was)
        lib.blvm_pchain_tune(-1)  # (back to the environment's or the default bits)
    assert _hip.take_async_errors() == (0, 0)
    return got, launches


@pytest.mark.timeout(120)
@pytest.mark.parametrize("TP", [3, 5])
@pytest.mark.parametrize("B", [17, 33, 48, 49, 64])
def test_static_walk_is_placement_independent(model, B, TP):
    batch = _batch(B, TP)
    for free_nats in (0.0, 2.0):
        ref, n_ref = _step(model, batch, free_nats, False, BASE)
        assert n_ref == 0  # the interpreter ran the reference
        for k in EXACT:
            assert bool(torch.isfinite(ref[k]).all()), k
        assert float(ref["d_h0"].abs().max()) > 0 and float(ref["d_enc"].abs().max()) > 0
        for place, tune in PLACES.items():
            got, n = _step(model, batch, free_nats, True, tune)
            assert n == 2, f"place {place}: the forward and the backward must run on the static kernels"
            for k in EXACT:
                assert torch.equal(got[k], ref[k]), f"B={B} T'={TP} free_nats={free_nats} place={place}: {k} differs from the interpreter"
