"""GPU: the static-walk VRNN kernels with register-resident weights (csrc/vrnn_static.hip) against the interpreter (csrc/pchain.hip).

A workgroup of the static walk loads the weight fragments of the one tile it owns of every critical-path link once per launch, in
front of its step loop, and skips the load where the deal gives it no tile.  The arithmetic and its order are the interpreter's, so
the comparison is `test_gpu_vrnn_static.py`'s: loss, ELBO, KL, z and h_n bit-identical, gradients at most 1e-6 relative apart (the
weight gradients are summed with float atomics on either path).  Here: every row-tile count with full and ragged last row tiles,
weights that change between launches, two models in one process, and a carried state."""
import pytest
import torch

from blvm import _hip
from blvm.models import VRNNAudio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 64   # samples per frame, as bench.py
H = 256  # the static walk is built for H = Z = 256 (R = 512)
TP = 5
EXACT = ["loss", "elbo", "kl", "z", "h_n"]


def _lib():
    lib = _hip.load()
    assert lib.blvm_device_ok() == 1
    return lib


def _model(seed):
    torch.manual_seed(seed)
    return VRNNAudio(likelihood="DMoL", input_size=S, hidden_size=H, latent_size=H, residual_posterior=True).to(DEV)


def _batch(B, seed, Tp=TP):
    g = torch.Generator().manual_seed(seed + 1)
    T_ = Tp * S
    x = (torch.rand(B, T_, generator=g) * 2 - 1).to(DEV)
    x_sl = torch.randint(T_ // 2, T_ + 1, (B,), generator=g, dtype=torch.int64)  # ragged
    x_sl[0] = T_
    eps = torch.randn(Tp, B, H, generator=g).to(DEV)
    return x, x_sl, eps


def _run(m, batch, static, backward=True, **kw):
    """One forward (+ backward) of `m` on the chosen path; returns the step's results and the number of static launches."""
    lib = _lib()
    was = lib.blvm_pchain_static(1 if static else 0)
    n0 = lib.blvm_pchain_static(-2)
    try:
        x, x_sl, eps = batch
        m.zero_grad(set_to_none=True)
        loss, _, out = m(x, x_sl, beta=1.0, free_nats=2.0, eps=eps, **kw)
        if backward:
            loss.backward()
        torch.cuda.synchronize()
        res = {"loss": loss.detach().clone(), "elbo": out.elbo.detach().clone(), "kl": out.kl.detach().clone(), "z": out.z.detach().clone(),
               "h_n": out.h_n.detach().clone()}
        if backward:
            for k, p in m.named_parameters():
                res["grad." + k] = p.grad.detach().clone()
        launches = lib.blvm_pchain_static(-2) - n0
    finally:
        lib.blvm_pchain_static(was)
    assert _hip.take_async_errors() == (0, 0)
    return res, launches


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _assert_same(static, interp):
    assert static.keys() == interp.keys()
    bad = [k for k in EXACT if not torch.equal(static[k], interp[k])]
    assert not bad, f"static and interpreter differ in {bad}"
    assert all(bool(torch.isfinite(static[k]).all()) for k in static)
    loose = [(k, _rel(static[k], interp[k])) for k in interp if k not in EXACT and not torch.equal(static[k], interp[k])]
    bad = [x for x in loose if x[1] > 1e-6]
    assert not bad, bad[:8]


@pytest.mark.timeout(120)
@pytest.mark.parametrize("B", [1, 15, 17, 33, 48, 64])
def test_resident_static_walk_matches_interpreter(B):
    """Every row-tile count (1 .. 4) with a full and a ragged last row tile: workgroups without a tile of a link skip its load."""
    m, batch = _model(0), _batch(B, 0)
    st, n_st = _run(m, batch, True)
    it, n_it = _run(m, batch, False)
    _assert_same(st, it)
    assert (n_st, n_it) == (2, 0)  # the forward and the backward ran on the static kernels, and only with the selector on


@pytest.mark.timeout(120)
def test_weights_are_read_at_every_launch():
    """Two training steps with an SGD update of every parameter in between: the second static step must see the updated weights."""
    m, batch = _model(3), _batch(33, 3)
    first, n = _run(m, batch, True)
    assert n == 2
    with torch.no_grad():
        for p in m.parameters():
            p.add_(p.grad, alpha=-0.05)
    st, n_st = _run(m, batch, True)
    it, n_it = _run(m, batch, False)
    _assert_same(st, it)
    assert (n_st, n_it) == (2, 0)
    assert not torch.equal(st["z"], first["z"]) and not torch.equal(st["loss"], first["loss"])  # (the update did change the step)


@pytest.mark.timeout(120)
def test_two_models_back_to_back():
    """Two models with different seeds in one process: nothing of the first launch's weights survives into the second."""
    batch = _batch(17, 5)
    res = []
    for seed in (11, 12):
        m = _model(seed)
        st, n_st = _run(m, batch, True)
        it, n_it = _run(m, batch, False)
        _assert_same(st, it)
        assert (n_st, n_it) == (2, 0)
        res.append(st)
    assert not torch.equal(res[0]["z"], res[1]["z"])


@pytest.mark.timeout(120)
def test_carried_state():
    """A forward from a non-zero h0."""
    m, batch = _model(7), _batch(48, 7)
    h0 = (torch.rand(48, 2 * H, generator=torch.Generator().manual_seed(9)) * 2 - 1).to(DEV)
    with torch.no_grad():
        st, n_st = _run(m, batch, True, backward=False, h0=h0)
        it, n_it = _run(m, batch, False, backward=False, h0=h0)
        zero, _ = _run(m, batch, True, backward=False)
    _assert_same(st, it)
    assert (n_st, n_it) == (1, 0)
    assert not torch.equal(st["h_n"], zero["h_n"])  # (the state did reach the step)


def _backward_walk_outputs(m, batch, h0, static):
    """What the backward walk itself hands back, with no atomic sum behind it: the gradient wrt the initial state (the GRU-backward
    tile of the last backward step writes it) and wrt the encoder output (a plain product of the walk's last posterior gradient)."""
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
        x, x_sl, eps = batch
        h = h0.clone().requires_grad_(True)
        m.zero_grad(set_to_none=True)
        loss, _, _ = m(x, x_sl, beta=1.0, free_nats=2.0, eps=eps, h0=h)
        loss.backward()
        torch.cuda.synchronize()
        got["d_h0"] = h.grad.detach().clone()
        launches = lib.blvm_pchain_static(-2) - n0
    finally:
        del cell.sequence  # (back to the class's method)
        lib.blvm_pchain_static(was)
    assert _hip.take_async_errors() == (0, 0)
    return got, launches


@pytest.mark.timeout(120)
@pytest.mark.parametrize("B", [17, 64])
def test_backward_walk_outputs_are_bit_identical(B):
    """The weight gradients are summed with float atomics and can only be held to 1e-6; what the backward walk writes itself is
    deterministic and must not move by a bit: d_h0 and d_enc depend on every link of every backward step."""
    m, batch = _model(13), _batch(B, 13, Tp=12)
    h0 = (torch.rand(B, 2 * H, generator=torch.Generator().manual_seed(14)) * 2 - 1).to(DEV)
    st, n_st = _backward_walk_outputs(m, batch, h0, True)
    it, n_it = _backward_walk_outputs(m, batch, h0, False)
    again, _ = _backward_walk_outputs(m, batch, h0, False)
    assert (n_st, n_it) == (2, 0)
    for k in ("d_h0", "d_enc"):
        assert bool(torch.isfinite(st[k]).all()) and float(st[k].abs().max()) > 0
        assert torch.equal(it[k], again[k]), f"{k}: the interpreter differs from itself"
        assert torch.equal(st[k], it[k]), f"{k}: static and interpreter differ, rel {_rel(st[k], it[k]):.3e}"
