"""The fp32 VRNN step program (K1, `ops.vrnn_sequence`) and SRNN latent chain (K3, `ops.srnn_latent_chain`) per row against float64,
on every dispatch arm.

Contract.  With fp32 operands a chain is an fp32 evaluation of the float64 oracle and nothing else: no operand is rounded, so the
oracle (`links16.vrnn_oracle` / `srnn_oracle`, mode "f32") runs free and only the free-nats decision is taken from the kernel's
stored statistics.  Cases, inputs, kinks, bars and `judge`: tests/chains32.py; that every bar, share and mutation holds for the
float32 stand-in in the kernel's place: tests/test_chains32_cpu.py.

  * Values: EVERY (t, b) row of phi and h (decin), z / zs, mu_q, sd_q, mu_p, sd_p and every element of kld and kld_fn at relative
    L2 <= 1e-5; the initial state is stored as given (zeros for None) and the phi part of decin row T' is zero, exactly.
  * Gradients of (out * w).sum() + (0.3 kld + 0.7 kld_fn).sum() with free nats on: per tensor, and per batch row for d_enc, d_h0 /
    d_d, d_a, d_z0, at the recorded bars of tests/golden/chains32_bars.json (2e-5 throughout: the stand-in's worst is 1.7e-6).
  * Forward at T' = 6, backward at T' = 3, and both at T' = 1 on one case per arm (no recurrent gradient product; the d_h0 / d_z0
    tail reads step 0 directly); ragged lengths through x_sl with stride 3.
  * The arm: `blvm_vrnn_path_counts` / `blvm_srnn_path_counts` and `blvm_pchain_static(-2)` report exactly the increments of
    `chains32.expected_counts`: static walk (H = Z = 256, R = 512, B <= 64), interpreter program on 16-row tiles, row-group
    program (B = 65: the last group is one tile holding one row; B = 150), launch per link on 16-row tiles, on 32x32 tiles (B = 257
    / 129: the last tile holds one row) and on both inside one sequence (R = 80).
  * No persistent launch gave up on a spin.

Measured on an MI355X, worst over an arm's cases: value row / KL element / gradient tensor (share of its bar) / batch row of an
input's gradient (share of its bar).  All 112 cases pass on their asserted arm.
  VRNN static walk             2.2e-7 / 3.1e-6 / 1.6e-6 (0.08) / 6.8e-7 (0.03)
  VRNN interpreter             2.3e-7 / 2.0e-6 / 7.8e-7 (0.04) / 1.1e-6 (0.06)
  VRNN row groups              2.0e-7 / 2.1e-6 / 7.9e-7 (0.04) / 7.0e-7 (0.04)
  VRNN per link, engine off    1.8e-7 / 2.0e-6 / 7.8e-7 (0.04) / 1.1e-6 (0.06)
  VRNN per link, B = 257       2.3e-7 / 3.1e-6 / 7.3e-7 (0.04) / 1.8e-6 (0.09)
  SRNN engine program          2.6e-7 / 4.1e-6 / 6.7e-7 (0.03) / 1.3e-6 (0.07)
  SRNN per link, B = 129       1.9e-7 / 2.0e-6 / 4.9e-7 (0.02) / 1.1e-6 (0.06)
  SRNN per link, engine off    1.6e-7 / 1.3e-6 / 2.4e-7 (0.01) / 3.0e-7 (0.02)
The kernels sit where the float32 stand-in sits (its worst gradient tensor over all cases and seeds: 1.7e-6), 600 times under the
1e-3 per-tensor bar of the model-level tests.  The widths H = 64, Z = 48, R = 96 at B = 257 keep every link on 32x32 tiles (no
link of the VRNN is Z wide: the head and dz kernels take the Z-wide products); a sequence that mixes both tile sizes needs a 3R or
R that is no multiple of 32, the R = 80 case (per step one 16-row link launch and six on 32x32 tiles, each way).
"""
import contextlib
import ctypes

import pytest
import torch

import blvm_oracle as O
import chains32 as C
import links16 as L
from blvm import _hip, ops
from test_gpu_rnn_sequences import Checks

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _require_hip():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert _hip.load().blvm_device_ok() == 1, "libblvm_hip: no gfx950 device visible"


@contextlib.contextmanager
def arm_of(c):
    """The engine setting of the case and the static selector on; both restored afterwards."""
    lib = _hip.load()
    before, static = lib.blvm_pchain_max_batch(), lib.blvm_pchain_static(-1)
    try:
        lib.blvm_pchain_configure(128 if c.engine else 0, 0)
        lib.blvm_pchain_static(1)
        yield
    finally:
        lib.blvm_pchain_static(static)
        lib.blvm_pchain_configure(before, 0)


def counts(c):
    lib = _hip.load()
    n = 7 if c.family == "vrnn" else 6
    buf = (ctypes.c_ulonglong * n)()
    _hip.check(getattr(lib, f"blvm_{c.family}_path_counts")(buf), "path_counts")
    return list(buf), lib.blvm_pchain_static(-2)


@contextlib.contextmanager
def expect_arm(c, Tp, backward, what):
    want, want_static = C.expected_counts(c, Tp, backward)
    before, static = counts(c)
    yield
    after, static2 = counts(c)
    delta = [a - b for a, b in zip(after, before)]
    names = C.VRNN_COUNTERS if c.family == "vrnn" else C.SRNN_COUNTERS
    print(f"{what}: " + ", ".join(f"{names[k]} x{n}" for k, n in enumerate(delta) if n) + f", static-walk launches x{static2 - static}")
    assert delta == want and static2 - static == want_static, (
        f"{what}: expected {dict(zip(names, want))} and {want_static} static-walk launches, the counters report {dict(zip(names, delta))} and {static2 - static}")  # fmt: skip


def run(c, Tp, inp, free_nats, backward, tag):
    """-> the kernel's result dict (stored tensors, kld, kld_fn; backward: d_<input>, d_<parameter>), every arm asserted."""
    names = C.grad_names(c)
    dev = {n: inp[n].to(DEV).requires_grad_(backward) for n in names}
    x_sl = inp["lens"].to(DEV, torch.int32)
    _hip.take_async_errors()
    with arm_of(c):
        with expect_arm(c, Tp, False, tag + " forward"):
            if c.family == "vrnn":
                res = ops.vrnn_sequence(dev["enc"], dev.get("h0"), inp["eps"].to(DEV), x_sl, [dev[n] for n in O.VRNN_SEQ_PARAMS], c.X, c.H, c.Z, c.R,
                                        c.residual, C.STRIDE, free_nats)  # fmt: skip
                got = dict(zip(("decin", "kld", "kld_fn") + L.VRNN_STATS, res))
                out = got["decin"]
            else:
                res = ops.srnn_latent_chain(dev["d"], dev["a"], dev.get("z0"), inp["eps"].to(DEV), x_sl, [dev[n] for n in O.SRNN_CHAIN_PARAMS], c.H, c.Z, c.R,
                                            c.residual, C.STRIDE, free_nats)  # fmt: skip
                got = dict(zip(("zs", "kld", "kld_fn", "mu_q", "sd_q", "mu_p", "sd_p"), res))
                out = got["zs"][1:]
            torch.cuda.synchronize()
        if backward:
            with expect_arm(c, Tp, True, tag + " backward"):
                ((out * inp["w"].to(DEV)).sum() + (C.COEF[0] * got["kld"] + C.COEF[1] * got["kld_fn"]).sum()).backward()
                torch.cuda.synchronize()
            got.update({"d_" + n: dev[n].grad for n in names})
    return {k: v.detach().cpu() for k, v in got.items()}


def _report(ck, c, Tp, got, ref, inp, entry):
    fails, fig = C.judge(c, Tp, got, ref, inp, entry)
    grads = "" if entry is None else (f"; worst gradient tensor {fig['tensor']:.3e} ({fig['tensor_share']:.2f} of its bar), worst batch row "
                                      f"{fig['grad_row']:.3e} ({fig['grad_row_share']:.2f} of its bar)")  # fmt: skip
    print(f"{ck.tag} summary: worst value row {fig['row']:.3e} ({fig['row'] / L.BAR_VALUE:.2f} of its bar), worst KL element {fig['kl']:.3e}{grads}")
    ck.failures += fails
    ck.done()


def _forward(ct):
    c, Tp = ct
    inp, free_nats, _ = C.inputs(c, Tp)
    tag = C.case_id(ct)
    got = run(c, Tp, inp, free_nats, False, tag)
    ref = C.oracle(c, inp, forced_stats=got, free_nats=free_nats)
    _report(Checks(tag), c, Tp, got, ref, inp, None)


@pytest.mark.parametrize("ct", [ct for ct in C.FWD_CASES if ct[0].family == "vrnn"], ids=C.case_id)
def test_vrnn_forward_rows(ct):
    """Every stored (t, b) row and every KL element of the VRNN step program against the free-running float64 oracle, at 1e-5."""
    _forward(ct)


@pytest.mark.parametrize("ct", [ct for ct in C.FWD_CASES if ct[0].family == "srnn"], ids=C.case_id)
def test_srnn_forward_rows(ct):
    """The same for the SRNN latent chain."""
    _forward(ct)


@pytest.mark.parametrize("ct", C.BWD_CASES, ids=C.case_id)
def test_chain_backward_rows(ct):
    """Every gradient of both chains per tensor, and per batch row for the inputs' gradients, at the recorded bars; the forward values
    of the same run at theirs."""
    c, Tp = ct
    inp, free_nats, _, entry = C.backward_case(ct)
    tag = C.case_id(ct)
    got = run(c, Tp, inp, free_nats, True, tag)
    ref = C.oracle(c, inp, backward=True, forced_stats=got, free_nats=free_nats)
    _report(Checks(tag), c, Tp, got, ref, inp, entry)
