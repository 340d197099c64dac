"""Every dispatch arm of the single-layer LSTM (K4) and GRU (K2) sequence entry points, forward and backward, against float64.

`blvm_lstm_seq_fwd/_bwd` and `blvm_gru_seq_fwd/_bwd` (csrc/rnn.hip) each choose one of three implementations per call: the
register-resident persistent kernels (csrc/seqchain.hip), a program of the persistent-chain interpreter (csrc/pchain.hip) or one
launch per step.  `blvm_rnn_path_counts` says which one a call took; every case here asserts it (`REGS` / `PROGRAM` / `PER_STEP`
below are the arms with the engine on — with `blvm_pchain_configure(0, .)` every case runs one launch per step), so a change
of the dispatch conditions cannot silently move a case onto another kernel.

References: LSTM — `blvm_oracle.lstm_sequence_ref` (the contract of include/blvm_hip.h as a float64 time loop, pinned against
`nn.LSTM` in tests/test_rnn_reference_cpu.py; unlike packing it takes unsorted lengths, length 0 and no lengths); GRU — `nn.GRU`
in float64 between two `blvm_oracle.reverse_sequences`.  All parameters and inputs are generated in fp32 and widened exactly.

Bounds (the project's bars for these kernels against float64; the reference loop evaluated in fp32 differs from float64 by
1.1e-7 (out) to 2.4e-7 (gradients), so the bars sit 40 to 80 times above the reference's own rounding): relative L2 <= 1e-5 for
out, h_n, c_n and <= 2e-5 for every gradient, per tensor AND per batch row of out, d_x, h_n, c_n, d_h0, d_c0 (a wrong last row of
a ragged tile fails by its index instead of being averaged away); a row whose reference norm is below 1e-12 must be exactly zero.
Without tolerance: out is 0 past a row's length; a row of length 0 returns its initial state bit for bit and has zero d_x, d_h0
and d_c0.  After each case no persistent launch has given up on a spin."""
import contextlib
import copy
import ctypes
import functools

import pytest
import torch

import blvm_oracle as O
from blvm import _hip, ops
from rnn_arms import PER_STEP, PROGRAM, REGS, sorted_lens, unsorted_lens, zero_row

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR_VALUE, BAR_GRAD = 1e-5, 2e-5
ARM_NAMES = ("register-resident", "interpreter program", "one launch per step")
LSTM_FWD, LSTM_BWD, GRU_FWD, GRU_BWD = 0, 1, 2, 3


@pytest.fixture(scope="module", autouse=True)
def _require_hip():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert _hip.load().blvm_device_ok() == 1, "libblvm_hip: no gfx950 device visible"


@pytest.fixture(params=[True, False], ids=["engine_on", "engine_off"])
def engine(request):
    """Both settings of the execution switch of K1-K5 (`chain_path` of test_gpu_buffer_contract.py), restored afterwards."""
    lib = _hip.load()
    before = lib.blvm_pchain_max_batch()
    lib.blvm_pchain_configure(128 if request.param else 0, 0)
    try:
        yield request.param
    finally:
        lib.blvm_pchain_configure(before, 0)


def path_counts():
    buf = (ctypes.c_ulonglong * 12)()
    _hip.check(_hip.load().blvm_rnn_path_counts(buf), "blvm_rnn_path_counts")
    return list(buf)


@contextlib.contextmanager
def expect_path(op, arm, what):
    """Exactly one call of entry point `op` inside the block, on arm `arm`, and no other sequence entry point ran."""
    before = path_counts()
    yield
    delta = [a - b for a, b in zip(path_counts(), before)]
    want = [0] * 12
    want[op * 3 + arm] = 1
    took = [f"op {k // 3} on {ARM_NAMES[k % 3]} x{n}" for k, n in enumerate(delta) if n]
    print(f"{what}: {', '.join(took)}")
    assert delta == want, f"{what}: expected one call of op {op} on the {ARM_NAMES[arm]} arm, the counters report {took}"


class Checks:
    """Collects every figure of a case (printed) and every miss; `done()` asserts there was none."""

    def __init__(self, tag):
        self.tag, self.failures = tag, []

    def close(self, name, got, ref, bar, row_dim=None):
        got, ref = got.detach().double().cpu(), ref.detach().double()
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        if not bool(torch.isfinite(got).all()):
            self.failures.append(f"{name}: non-finite values")
            return
        err = float((got - ref).norm() / (ref.norm() + 1e-30))
        worst = ""
        if row_dim is not None:
            g2, r2 = got.movedim(row_dim, 0).reshape(got.shape[row_dim], -1), ref.movedim(row_dim, 0).reshape(ref.shape[row_dim], -1)
            rn = r2.norm(dim=1)
            rel = (g2 - r2).norm(dim=1) / rn.clamp_min(1e-300)
            for b in range(g2.shape[0]):
                if float(rn[b]) < 1e-12:
                    if not bool((g2[b] == 0).all()):
                        self.failures.append(f"{name} row {b}: the reference row is zero, got max |x| = {float(g2[b].abs().max()):.3e}")
                elif float(rel[b]) > bar:
                    self.failures.append(f"{name} row {b}: rel_l2 {float(rel[b]):.3e} > {bar:.0e}")
            live = rn >= 1e-12
            if bool(live.any()):
                k = int(torch.where(live, rel, torch.zeros_like(rel)).argmax())
                worst = f", worst row {k}: {float(rel[k]):.3e}"
        print(f"{self.tag} {name}: rel_l2 {err:.3e}{worst} (bar {bar:.0e})")
        if err > bar:
            self.failures.append(f"{name}: rel_l2 {err:.3e} > {bar:.0e}")

    def exact(self, name, ok):
        if not bool(ok):
            self.failures.append(f"{name}: not exact")

    def done(self):
        torch.cuda.synchronize()
        errs = _hip.take_async_errors()
        if errs != (0, 0):
            self.failures.append(f"a persistent launch gave up on a bounded spin: {errs}")
        assert not self.failures, f"{self.tag}:\n  " + "\n  ".join(self.failures)


# ----------------------------------------------------------------------------------------------------------------------
# lengths
# ----------------------------------------------------------------------------------------------------------------------


def test_length_patterns():
    for T_, B in ((6, 21), (5, 37), (4, 129), (5, 16), (5, 17), (4, 128), (1, 21), (3, 21)):
        lens = unsorted_lens(T_, B)
        z = zero_row(B)
        assert int(lens[0]) == T_ and int(lens[z]) == 0 and int((lens == 0).sum()) == 1 and z >= 16 * ((B - 1) // 16)
        assert int((lens == 1).sum()) >= 1 and int(lens.max()) == T_
        assert T_ < 3 or not bool((lens[:-1] >= lens[1:]).all())
        rev = unsorted_lens(T_, B, with_zero=False)
        assert int(rev.min()) == 1 and int(rev[0]) == T_ and int(rev[B - 1]) == 1
        s = sorted_lens(T_, B)
        assert bool((s[:-1] >= s[1:]).all()) and int(s[0]) == T_ and int(s.min()) >= 1
    assert unsorted_lens(5, 1).tolist() == [5] and zero_row(17) == 16 and zero_row(16) == 7 and zero_row(21) == 18


# ----------------------------------------------------------------------------------------------------------------------
# LSTM
# ----------------------------------------------------------------------------------------------------------------------

BOTH, NONE, H_ONLY, C_ONLY = "h0c0", "nostate", "h0only", "c0only"
UNSORTED, SORTED, NOLENS = "unsorted", "sorted", "nolens"

# (T, B, I, H, arm with the engine on)
LSTM_SHAPES = [
    (6, 21, 16, 32, PROGRAM),    # the smallest shape
    (5, 37, 24, 128, REGS),      # 1 forward / 4 backward k-chunks per wave
    (5, 37, 24, 384, REGS),      # 3 / 12 k-chunks: the only forward NCH = 3 and the once-per-XCD operand read; 72 workgroups
    (5, 21, 24, 512, PROGRAM),   # K = 512 / 2048
    (5, 21, 16, 48, PROGRAM),    # K tail
    (5, 21, 16, 272, PROGRAM),   # 17 column tiles, K tail
    (5, 1, 16, 128, REGS),       # one row
    (5, 16, 16, 128, REGS),      # one full row tile
    (5, 17, 16, 128, REGS),      # a second tile holding one row
    (4, 128, 16, 256, REGS),     # the largest engine batch; 128 workgroups
    (4, 129, 16, 256, PER_STEP),  # the first batch past it
    (1, 21, 16, 128, PER_STEP),  # T < 4 runs one launch per step even with the engine on
    (3, 21, 16, 128, PER_STEP),
]
VARIANT_SHAPES = [(6, 21, 16, 32, PROGRAM), (5, 37, 24, 384, REGS), (4, 129, 16, 256, PER_STEP)]  # one per arm
LSTM_CASES = (
    [s + (BOTH, UNSORTED) for s in LSTM_SHAPES]
    + [s + (st, UNSORTED) for s in VARIANT_SHAPES for st in (NONE, H_ONLY, C_ONLY)]
    + [s + (BOTH, ln) for s in VARIANT_SHAPES for ln in (SORTED, NOLENS)]
    + [(5, 17, 16, 128, REGS, BOTH, SORTED)]  # the unsorted pattern's length-0 row IS the one row of the second tile: also live
)


def _lens_of(kind, T_, B):
    return {UNSORTED: unsorted_lens, SORTED: sorted_lens, NOLENS: lambda *_: None}[kind](T_, B)


@functools.lru_cache(maxsize=None)
def lstm_case(T_, B, I, H, state, lens_kind):
    """fp32 inputs and the float64 reference (computed once, shared by both engine settings; treat as read-only)."""
    g = torch.Generator().manual_seed(1000 * H + 10 * B + T_)
    k = H ** -0.5
    Wih, Whh, bih, bhh = ((torch.rand(s, generator=g) * 2 - 1) * k for s in ((4 * H, I), (4 * H, H), (4 * H,), (4 * H,)))
    x = torch.randn(T_, B, I, generator=g)
    h0 = torch.randn(B, H, generator=g) * 0.5 if state in (BOTH, H_ONLY) else None
    c0 = torch.randn(B, H, generator=g) * 0.5 if state in (BOTH, C_ONLY) else None
    w = torch.randn(T_, B, H, generator=g)
    lens = _lens_of(lens_kind, T_, B)
    leaves = {n: t.double().requires_grad_(True) for n, t in dict(x=x, h0=h0, c0=c0, Wih=Wih, Whh=Whh, bih=bih, bhh=bhh).items() if t is not None}
    out, hn, cn = O.lstm_sequence_ref(leaves["x"], leaves.get("h0"), leaves.get("c0"), lens, *(leaves[n] for n in ("Wih", "Whh", "bih", "bhh")))
    (out * w.double()).sum().backward()
    ref = dict(out=out.detach(), h_n=hn.detach(), c_n=cn.detach(), **{"d_" + n: t.grad for n, t in leaves.items()})
    return dict(x=x, h0=h0, c0=c0, w=w, lens=lens, Wih=Wih, Whh=Whh, bih=bih, bhh=bhh), ref


def _lstm_id(c):
    return f"T{c[0]}-B{c[1]}-I{c[2]}-H{c[3]}-{c[5]}-{c[6]}"


@pytest.mark.parametrize("case", LSTM_CASES, ids=_lstm_id)
def test_lstm_sequence_every_arm(case, engine):
    T_, B, I, H, arm_on, state, lens_kind = case
    arm = arm_on if engine else PER_STEP
    inp, ref = lstm_case(T_, B, I, H, state, lens_kind)
    tag = f"lstm {_lstm_id(case)} [{'engine on' if engine else 'engine off'}]"
    dev = {n: inp[n].to(DEV).requires_grad_(True) for n in ("x", "h0", "c0", "Wih", "Whh", "bih", "bhh") if inp[n] is not None}
    lens = inp["lens"]
    lens_dev = lens.to(DEV, torch.int32) if lens is not None else None
    _hip.take_async_errors()
    with expect_path(LSTM_FWD, arm, tag + " forward"):
        out, hn, cn = ops.lstm_sequence(dev["x"], dev.get("h0"), dev.get("c0"), lens_dev, dev["Wih"], dev["Whh"], dev["bih"], dev["bhh"])
    with expect_path(LSTM_BWD, arm, tag + " backward"):
        (out * inp["w"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    ck = Checks(tag)
    ck.close("out", out, ref["out"], BAR_VALUE, row_dim=1)
    ck.close("h_n", hn, ref["h_n"], BAR_VALUE, row_dim=0)
    ck.close("c_n", cn, ref["c_n"], BAR_VALUE, row_dim=0)
    ck.close("d_x", dev["x"].grad, ref["d_x"], BAR_GRAD, row_dim=1)
    for n in ("h0", "c0"):
        if n in dev:
            ck.close("d_" + n, dev[n].grad, ref["d_" + n], BAR_GRAD, row_dim=0)
    for n in ("Wih", "Whh", "bih", "bhh"):
        ck.close("d_" + n, dev[n].grad, ref["d_" + n], BAR_GRAD)
    if lens is not None:
        out_c, hn_c, cn_c, dx_c = out.detach().cpu(), hn.cpu(), cn.cpu(), dev["x"].grad.cpu()
        zeros = torch.zeros(B, H)
        for b in range(B):
            n = int(lens[b])
            ck.exact(f"out[{n}:, {b}] == 0 (row past its length)", (out_c[n:, b] == 0).all())
            if n == 0:
                h_init = inp["h0"][b] if inp["h0"] is not None else zeros[b]
                c_init = inp["c0"][b] if inp["c0"] is not None else zeros[b]
                ck.exact(f"h_n[{b}] == h0[{b}] bit for bit (length 0)", torch.equal(hn_c[b].view(torch.int32), h_init.view(torch.int32)))
                ck.exact(f"c_n[{b}] == c0[{b}] bit for bit (length 0)", torch.equal(cn_c[b].view(torch.int32), c_init.view(torch.int32)))
                ck.exact(f"d_x[:, {b}] == 0 (length 0)", (dx_c[:, b] == 0).all())
                for m in ("h0", "c0"):
                    if m in dev:
                        ck.exact(f"d_{m}[{b}] == 0 (length 0)", (dev[m].grad[b] == 0).all())
    ck.done()


# ----------------------------------------------------------------------------------------------------------------------
# GRU
# ----------------------------------------------------------------------------------------------------------------------

# (T, B, I, R, arm with the engine on)
GRU_SHAPES = [
    (5, 21, 16, 64, PROGRAM),    # between the tested R = 32 and the register-resident sizes
    (5, 21, 24, 384, PROGRAM),   # 3R / 128 = 9 k-chunks per wave are not instantiated
    (5, 1, 16, 128, REGS),
    (5, 16, 16, 128, REGS),
    (5, 17, 16, 128, REGS),
    (4, 128, 16, 128, REGS),
    (4, 129, 16, 128, PER_STEP),
    (1, 21, 16, 128, PER_STEP),
    (3, 21, 16, 128, PER_STEP),
]


@functools.lru_cache(maxsize=None)
def gru_case(T_, B, I, R, reverse):
    """fp32 inputs and the float64 reference: nn.GRU, between two reverse_sequences when `reverse` (computed once; read-only)."""
    torch.manual_seed(2000 * R + 10 * B + T_)
    gru = torch.nn.GRU(I, R)
    g = torch.Generator().manual_seed(3000 * R + 10 * B + T_ + int(reverse))
    x = torch.randn(T_, B, I, generator=g)
    h0 = torch.randn(B, R, generator=g) * 0.5
    w = torch.randn(T_, B, R, generator=g)
    lens = unsorted_lens(T_, B, with_zero=False) if reverse else None
    g64 = copy.deepcopy(gru).double()
    xr, h0r = x.double().requires_grad_(True), h0.double().requires_grad_(True)
    if reverse:
        out, hn = g64(O.reverse_sequences(xr, lens), h0r.unsqueeze(0))
        out = O.reverse_sequences(out, lens)
    else:
        out, hn = g64(xr, h0r.unsqueeze(0))
    (out * w.double()).sum().backward()
    ref = dict(out=out.detach(), h_n=hn[0].detach(), d_x=xr.grad, d_h0=h0r.grad, d_Wih=g64.weight_ih_l0.grad, d_Whh=g64.weight_hh_l0.grad,
               d_bih=g64.bias_ih_l0.grad, d_bhh=g64.bias_hh_l0.grad)
    params = dict(Wih=gru.weight_ih_l0.detach(), Whh=gru.weight_hh_l0.detach(), bih=gru.bias_ih_l0.detach(), bhh=gru.bias_hh_l0.detach())
    return dict(x=x, h0=h0, w=w, lens=lens, **params), ref


def _gru_id(c):
    return f"T{c[0]}-B{c[1]}-I{c[2]}-R{c[3]}"


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reversed"])
@pytest.mark.parametrize("case", GRU_SHAPES, ids=_gru_id)
def test_gru_sequence_every_arm(case, reverse, engine):
    T_, B, I, R, arm_on = case
    arm = arm_on if engine else PER_STEP
    inp, ref = gru_case(T_, B, I, R, reverse)
    tag = f"gru {_gru_id(case)} {'reversed' if reverse else 'forward'} [{'engine on' if engine else 'engine off'}]"
    dev = {n: inp[n].to(DEV).requires_grad_(True) for n in ("x", "h0", "Wih", "Whh", "bih", "bhh")}
    lens_dev = inp["lens"].to(DEV, torch.int32) if reverse else None
    _hip.take_async_errors()
    with expect_path(GRU_FWD, arm, tag + " forward"):
        out, hn = ops.gru_sequence(dev["x"], dev["h0"], dev["Wih"], dev["Whh"], dev["bih"], dev["bhh"], lens_dev, reverse)
    with expect_path(GRU_BWD, arm, tag + " backward"):
        (out * inp["w"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    ck = Checks(tag)
    ck.close("out", out, ref["out"], BAR_VALUE, row_dim=1)
    ck.close("h_n", hn, ref["h_n"], BAR_VALUE, row_dim=0)
    ck.close("d_x", dev["x"].grad, ref["d_x"], BAR_GRAD, row_dim=1)
    ck.close("d_h0", dev["h0"].grad, ref["d_h0"], BAR_GRAD, row_dim=0)
    for n in ("Wih", "Whh", "bih", "bhh"):
        ck.close("d_" + n, dev[n].grad, ref["d_" + n], BAR_GRAD)
    ck.done()


def test_gru_strides_through_the_abi(engine):
    """`blvm_gru_seq_fwd/_bwd` called directly with every stride the ABI has, reversed: `in` with row stride I + 8; `out` and
    `d_out` inside a [T, B, R + 16] buffer at column 8; `d_in` with row stride I + 8, accumulated onto ones.  The padding columns of
    `out` and `d_in` keep their prefill exactly; the payload meets the bars against float64 (d_in: the reference + 1)."""
    T_, B, I, R = 5, 21, 24, 128
    PAD_IN, OFF, WIDE = 8, 8, R + 16
    inp, ref = gru_case(T_, B, I, R, True)
    tag = f"gru raw ABI T{T_}-B{B}-I{I}-R{R} reversed [{'engine on' if engine else 'engine off'}]"
    lib = _hip.load()
    f32 = dict(device=DEV, dtype=torch.float32)
    x_buf = torch.full((T_, B, I + PAD_IN), 7.0, **f32)
    x_buf[:, :, :I] = inp["x"].to(DEV)
    out_buf = torch.full((T_, B, WIDE), -3.0, **f32)
    dout_buf = torch.full((T_, B, WIDE), 5.0, **f32)
    dout_buf[:, :, OFF:OFF + R] = inp["w"].to(DEV)
    din_buf = torch.ones(T_, B, I + PAD_IN, **f32)
    Wih, Whh, bih, bhh, h0 = (inp[n].to(DEV).contiguous() for n in ("Wih", "Whh", "bih", "bhh", "h0"))
    lens_dev = inp["lens"].to(DEV, torch.int32)
    hn, d_h0 = torch.empty(B, R, **f32), torch.empty(B, R, **f32)
    dWih, dWhh, dbih, dbhh = torch.zeros_like(Wih), torch.zeros_like(Whh), torch.zeros_like(bih), torch.zeros_like(bhh)
    reserve = torch.empty(lib.blvm_gru_reserve_floats(T_, B, R), **f32)
    ws = torch.empty(lib.blvm_gru_bwd_workspace_floats(T_, B, R), **f32)
    # the last element written: OFF + (T-1) * B * WIDE + (B-1) * WIDE + R - 1 < T * B * WIDE
    assert OFF + R <= WIDE and out_buf.is_contiguous() and dout_buf.is_contiguous()
    p, sp = _hip.ptr, _hip.stream_ptr()
    arm = REGS if engine else PER_STEP
    _hip.take_async_errors()
    with expect_path(GRU_FWD, arm, tag + " forward"):
        _hip.check(lib.blvm_gru_seq_fwd(p(Wih), p(Whh), p(bih), p(bhh), p(x_buf), I + PAD_IN, p(h0), p(lens_dev), 1, T_, B, I, R,
                                        out_buf.data_ptr() + 4 * OFF, B * WIDE, WIDE, p(hn), p(reserve), sp), "blvm_gru_seq_fwd")
    with expect_path(GRU_BWD, arm, tag + " backward"):
        _hip.check(lib.blvm_gru_seq_bwd(p(Wih), p(Whh), p(x_buf), I + PAD_IN, p(lens_dev), 1, p(reserve), dout_buf.data_ptr() + 4 * OFF,
                                        B * WIDE, WIDE, T_, B, I, R, p(din_buf), I + PAD_IN, 1, p(d_h0), p(dWih), p(dWhh), p(dbih),
                                        p(dbhh), p(ws), sp), "blvm_gru_seq_bwd")
    torch.cuda.synchronize()
    ck = Checks(tag)
    ck.exact("padding columns of out keep their prefill", (out_buf[:, :, :OFF] == -3.0).all() and (out_buf[:, :, OFF + R:] == -3.0).all())
    ck.exact("padding columns of d_in keep their prefill", (din_buf[:, :, I:] == 1.0).all())
    ck.exact("in and d_out are not written", (x_buf[:, :, I:] == 7.0).all() and (dout_buf[:, :, :OFF] == 5.0).all() and (dout_buf[:, :, OFF + R:] == 5.0).all())
    ck.close("out", out_buf[:, :, OFF:OFF + R], ref["out"], BAR_VALUE, row_dim=1)
    ck.close("h_n", hn, ref["h_n"], BAR_VALUE, row_dim=0)
    ck.close("d_in (+1)", din_buf[:, :, :I], ref["d_x"] + 1, BAR_GRAD, row_dim=1)
    ck.close("d_h0", d_h0, ref["d_h0"], BAR_GRAD, row_dim=0)
    for n, t in (("Wih", dWih), ("Whh", dWhh), ("bih", dbih), ("bhh", dbhh)):
        ck.close("d_" + n, t, ref["d_" + n], BAR_GRAD)
    ck.done()
