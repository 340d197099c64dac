"""GPU: poll pacing of the resident tiles (csrc/pchain.h "poll pacing") changes WHEN a tile's operand poll is issued, never what it
reads: a returned fragment set without a sentinel word is complete whatever the timing.  So every paced form must reproduce the
interpreter bit for bit.

- The resident chain probe under every kind of pacing setting its entry accepts — off; a first-poll delay on the waves that leave a
  tile at its barrier alone (0, the tuned 8 and a long one); the epilogue waves' delay alone; both (the VRNN walks' 8 : 4, the
  probe's best 8 : 8 and 12 : 12, and a long pair) — against `blvm_pchain_chain_probe`, at B = 1, 8, 17, 64 and N = K = 256, 512
  over 64 links.  (The entry has no denser-cadence setting: that mechanism was not built)
- The VRNN static walk (its lock-step visits paced at compile time) against the interpreter, toggled with `blvm_pchain_static`: loss,
  per-utterance ELBO and KL, z, h_n, d_h0 and d_enc bit-identical at B = 1, 17, 64 with free nats 0 and 2, a row that ends inside
  step 1 and an empty row on either side of a tile edge.
No launch may abort: `_hip.take_async_errors()` is (0, 0) after every case."""
import pytest
import torch

from blvm import _hip
from blvm._hip import check, ptr, stream_ptr
from blvm.models import VRNNAudio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LINKS = 64
# (early, epi) first-poll delays in s_sleep units: off | the delay of the waves that leave a tile at its barrier alone, at 8 (the
# tuned value) and at 40 (far past the producers' stores; 0 is "off") | the epilogue waves' delay alone | both: 8:4 is what the VRNN
# walks are built with, 8:8 the probe's best at K = 256, 12:12 at K = 512 | both long
PACINGS = [(0, 0), (8, 0), (40, 0), (0, 4), (8, 4), (8, 8), (12, 12), (40, 24)]


def _lib():
    lib = _hip.load()
    assert lib.blvm_device_ok() == 1
    return lib


_chain_ref = {}


def _chain_inputs(B, N):
    g = torch.Generator().manual_seed(1000 * B + N)
    W = ((torch.rand(N, N, generator=g) * 2 - 1) * 2.45 / N ** 0.5).to(DEV)
    b = ((torch.rand(N, generator=g) * 2 - 1) * 0.1).to(DEV)
    x0 = (torch.rand(B, N, generator=g) * 2 - 1).to(DEV)
    return W, b, x0


def _chain(fn, B, N):
    lib = _lib()
    W, b, x0 = _chain_inputs(B, N)
    rows = (B + 15) // 16 * 16
    W16 = torch.empty(N * N, device=DEV)
    x16 = torch.empty((LINKS + 1) * rows * N, device=DEV)
    xs = torch.full((LINKS, B, N), float("nan"), device=DEV)
    check(lib.blvm_pchain_rows_to_t16(ptr(W), N, N, N, ptr(W16), stream_ptr()), "t16 W")
    check(lib.blvm_pchain_rows_to_t16(ptr(x0), N, B, N, ptr(x16), stream_ptr()), "t16 x")
    check(fn(ptr(W16), ptr(b), ptr(x16), ptr(xs), B, N, LINKS, 0, stream_ptr()), "chain probe")
    torch.cuda.synchronize()
    assert _hip.take_async_errors() == (0, 0)
    return xs


def _interpreter_chain(B, N):
    """The interpreter's chain, computed once per shape and shared by the pacing cases."""
    if (B, N) not in _chain_ref:
        _chain_ref[B, N] = _chain(_lib().blvm_pchain_chain_probe, B, N)
    return _chain_ref[B, N]


@pytest.mark.timeout(60)
@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("B", [1, 8, 17, 64])
def test_paced_chain_probe_matches_interpreter(B, N):
    lib = _lib()
    ref = _interpreter_chain(B, N)
    assert bool(torch.isfinite(ref).all()) and float(ref[-1].abs().max()) > 0  # (the chain is alive at its last link)
    plain = _chain(lib.blvm_pchain_static_chain_probe, B, N)
    assert torch.equal(plain, ref)
    for early, epi in PACINGS:
        fn = lambda W16, b, x16, xs, B_, N_, L, nwg, s, e=early, p=epi: lib.blvm_pchain_static_chain_probe_paced(W16, b, x16, xs, B_, N_, L, nwg, e, p, s)
        got = _chain(fn, B, N)
        assert torch.equal(got, ref), f"B={B} N={N} early={early} epi={epi}: the paced chain differs from the interpreter"


def test_paced_probe_refuses_bad_delays():
    lib = _lib()
    t = torch.zeros(16, device=DEV)
    for early, epi in ((-1, 0), (0, 65)):
        assert lib.blvm_pchain_static_chain_probe_paced(ptr(t), ptr(t), ptr(t), ptr(t), 8, 256, 4, 0, early, epi, stream_ptr()) != 0
    assert _hip.take_async_errors() == (0, 0)


# ---- the VRNN static walk ------------------------------------------------------------------------------------------------------
S = 64   # samples per frame, as bench.py
H = 256  # the static walk is built for H = Z = 256 (R = 512)
TP = 6
EXACT = ["loss", "elbo", "kl", "z", "h_n", "d_h0", "d_enc"]


def _model():
    torch.manual_seed(21)
    return VRNNAudio(likelihood="DMoL", input_size=S, hidden_size=H, latent_size=H, residual_posterior=True).to(DEV)


def _batch(B):
    g = torch.Generator().manual_seed(100 + B)
    T_ = TP * S
    x = (torch.rand(B, T_, generator=g) * 2 - 1).to(DEV)
    x_sl = torch.randint(T_ // 2, T_ + 1, (B,), generator=g, dtype=torch.int64)
    x_sl[0] = T_
    if B > 1:
        x_sl[B - 1] = S + S // 2  # ends inside step 1
    if B > 16:  # an empty row on either side of the first tile edge
        x_sl[15] = 0
        x_sl[16] = 0
    eps = torch.randn(TP, B, H, generator=g).to(DEV)
    h0 = (torch.rand(B, 2 * H, generator=g) * 2 - 1).to(DEV)
    return x, x_sl, eps, h0


def _step(m, batch, free_nats, static):
    lib = _lib()
    was = lib.blvm_pchain_static(1 if static else 0)
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
    assert _hip.take_async_errors() == (0, 0)
    return got, launches


@pytest.fixture(scope="module")
def model():
    return _model()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("free_nats", [0.0, 2.0])
@pytest.mark.parametrize("B", [1, 17, 64])
def test_paced_static_walk_matches_interpreter(model, B, free_nats):
    batch = _batch(B)
    st, n_st = _step(model, batch, free_nats, True)
    it, n_it = _step(model, batch, free_nats, False)
    assert (n_st, n_it) == (2, 0)  # the forward and the backward ran on the static kernels, and only with the selector on
    for k in EXACT:
        assert bool(torch.isfinite(st[k]).all()), k
        assert torch.equal(st[k], it[k]), f"{k}: static and interpreter differ"
    assert float(st["d_h0"].abs().max()) > 0 and float(st["d_enc"].abs().max()) > 0
