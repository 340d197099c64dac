"""GPU: the static-walk VRNN kernels (csrc/vrnn_static.hip) against the interpreter (csrc/pchain.hip) in one process.

`blvm_pchain_static(0)` sends the VRNN programs to the interpreter, `blvm_pchain_static(1)` (the default) to the static walk where
the program has its shape (B <= 64 on 16-row tiles, fp32, H = Z = 256, R = 512).  The tiles, their deal and their summation order are
the same, so every result must be bit-identical; where the static kernels do not apply the selector must change nothing."""
import time

import pytest
import torch

from blvm import _hip
from blvm.models import VRNNAudio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 64  # samples per frame, as bench.py
SENTINEL = torch.tensor([-1], dtype=torch.int32).view(torch.float32)  # bits 0xFFFFFFFF


def _lib():
    lib = _hip.load()
    assert lib.blvm_device_ok() == 1
    return lib


def _step(static, B, Tp, H=256, ragged=True, seed=0):
    """One forward + backward; returns every result the step produces (loss, per-utterance ELBO / KL, z, h_n, gradients)."""
    lib = _lib()
    was = lib.blvm_pchain_static(1 if static else 0)
    n0 = lib.blvm_pchain_static(-2)
    try:
        torch.manual_seed(seed)
        m = VRNNAudio(likelihood="DMoL", input_size=S, hidden_size=H, latent_size=H, residual_posterior=True).to(DEV)
        g = torch.Generator().manual_seed(seed + 1)
        T_ = Tp * S
        x = (torch.rand(B, T_, generator=g) * 2 - 1).to(DEV)
        if ragged:
            x_sl = torch.randint(T_ // 2, T_ + 1, (B,), generator=g, dtype=torch.int64)
            x_sl[0] = T_
        else:
            x_sl = torch.full((B,), T_, dtype=torch.int64)
        eps = torch.randn(Tp, B, H, generator=g).to(DEV)
        loss, _, out = m(x, x_sl, beta=1.0, free_nats=2.0, eps=eps)
        loss.backward()
        torch.cuda.synchronize()
        res = {"loss": loss.detach().clone(), "elbo": out.elbo.detach().clone(), "kl": out.kl.detach().clone(), "z": out.z.detach().clone(),
               "h_n": out.h_n.detach().clone()}
        for k, p in m.named_parameters():
            res["grad." + k] = p.grad.detach().clone()
        res["static_launches"] = lib.blvm_pchain_static(-2) - n0  # (kept out of the comparisons)
    finally:
        lib.blvm_pchain_static(was)
    assert _hip.take_async_errors() == (0, 0)
    return res


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _same(static, interp, again):
    """static vs interpreter: the step's outputs bit-identical; every gradient bit-identical or at most 1e-6 relative apart (the
    weight gradients are summed by split-K GEMMs and bias reductions with float atomics, whose order is not fixed: they vary from
    run to run on either path, the interpreter against itself included)."""
    launches = static.pop("static_launches"), interp.pop("static_launches"), again.pop("static_launches")
    assert static.keys() == interp.keys() == again.keys()
    exact = ["loss", "elbo", "kl", "z", "h_n"]
    assert all(torch.equal(interp[k], again[k]) for k in exact)
    bad = [k for k in exact if not torch.equal(static[k], interp[k])]
    assert not bad, f"static and interpreter differ in {bad}"
    loose = [(k, _rel(static[k], interp[k]), _rel(again[k], interp[k])) for k in interp if k not in exact and not torch.equal(static[k], interp[k])]
    bad = [x for x in loose if x[1] > 1e-6]
    assert not bad, bad[:8]
    if loose:
        print("gradients that differ (static vs interpreter, interpreter vs itself):", loose[:8])
    return launches


@pytest.mark.timeout(300)
@pytest.mark.parametrize("B,Tp,ragged", [(64, 250, False), (64, 40, True), (50, 40, True), (16, 250, True), (1, 30, False)])
def test_static_walk_matches_interpreter(B, Tp, ragged):
    launches = _same(_step(True, B, Tp, ragged=ragged), _step(False, B, Tp, ragged=ragged), _step(False, B, Tp, ragged=ragged))
    assert launches == (2, 0, 0)  # the forward and the backward ran on the static kernels, and only with the selector on


@pytest.mark.timeout(300)
@pytest.mark.parametrize("case", ["B65", "bf16", "H128"])
def test_selector_is_a_no_op_where_the_static_walk_does_not_apply(case):
    lib = _lib()
    kw = dict(B=65, Tp=20) if case == "B65" else dict(B=16, Tp=20, H=128) if case == "H128" else dict(B=16, Tp=20)
    old = lib.blvm_get_operand_dtype()
    if case == "bf16":
        lib.blvm_set_operand_dtype(1)
    try:
        assert _same(_step(True, **kw), _step(False, **kw), _step(False, **kw)) == (0, 0, 0)
    finally:
        lib.blvm_set_operand_dtype(old)


@pytest.mark.timeout(120)
def test_planted_sentinel_aborts_the_static_walk():
    """0xFFFFFFFF in a prior weight reaches a hand-off slab of the static forward; its bounded spins give up and the launch is counted."""
    lib = _lib()
    assert lib.blvm_pchain_static(-1) == 1  # the default: the static walk
    torch.manual_seed(0)
    m = VRNNAudio(likelihood="DMoL", input_size=S, hidden_size=256, latent_size=256, residual_posterior=True).to(DEV)
    B, T_ = 8, 12 * S
    x = (torch.rand(B, T_, generator=torch.Generator().manual_seed(1)) - 0.5).to(DEV)
    x_sl = torch.full((B,), T_, dtype=torch.int64)
    _hip.take_async_errors()
    n0 = lib.blvm_pchain_static(-2)
    with torch.no_grad():
        m.vrnn.vrnn_cell.prior[2].weight[3, 5] = SENTINEL.to(DEV)[0]
    t0 = time.time()
    loss, _, _ = m(x, x_sl, beta=1.0, free_nats=2.0)
    loss.backward()
    torch.cuda.synchronize()
    dt = time.time() - t0
    n, code = _hip.take_async_errors()
    print(f"static walk, planted sentinel: {n} aborted launch(es), code step {code >> 4} link {code & 15}, loss {float(loss.detach())}, {dt:.2f} s")
    assert lib.blvm_pchain_static(-2) - n0 == 2  # both launches were the static kernels
    assert n >= 1, (n, code)  # an aborted launch is counted (a NaN loss alone would not show it)
    assert (code & 15) < 10 and ((code >> 4) & 0xFFFFFF) <= 12, code  # the abort code names a link of the programs and a step of the sequence
    assert dt < 60
    assert _hip.take_async_errors() == (0, 0)
