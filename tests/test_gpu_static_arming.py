"""GPU: look-ahead arming of the static VRNN walks (csrc/vrnn_static.h kArmAhead) against the full host fill.

By default a static-walk launch of more than kArmAhead steps stores the sentinels of its polled slabs itself, kArmAhead steps
ahead, from workgroups that wait anyway; the host fills only the first kArmAhead steps.  Bit 128 of `blvm_pchain_tune` turns that
off: the host fills every polled slab in front of the launch, as the parent did.  Who stores a sentinel changes no operand and no
summation order, so everything the walks compute must be bit-identical between the two.

The hazard of arming is a consumer that finds STALE, valid-looking data where a sentinel should have been: the previous training
step's activations in the right layout.  So every case also runs with the buffers `blvm.ops` allocates (reserve and workspace
among them) pre-filled: with quiet NaNs, with noise, with the bytes the buffers held after an identical run, and with the bytes
they held after a run of the same shapes on other inputs (`test_gpu_buffer_contract.py`'s harness; after an identical run a missed
sentinel would find the right values, so only the run on other inputs can show one).

`ops.vrnn_sequence` forward + backward at H = Z = X = 256, R = 512 (the static kernels' widths), B = 64, 49, 17, 5 (four, four
with a one-row last, two with a one-row last, one partial row tile) x T' = kArmAhead - 1 (nothing armed), kArmAhead + 1,
2 kArmAhead + 3 and 37; the folded decoder at B = 64, T' = 2 kArmAhead + 3.  Bars: outputs bit-equal; d_enc and d_h0 bit-equal
where two runs of the off path are; everything summed with float atomics (the weight gradients, and d_enc / d_h0 where the off path
itself varies) within 1e-3 relative L2 of the float64 oracle, the bar of `test_gpu_parity.py` / `test_gpu_buffer_contract.py`."""
import contextlib
import functools

import pytest
import torch

import blvm_oracle as O
from blvm import _hip, ops
from blvm.models.vrnn import VRNNCell

from test_gpu_buffer_contract import poisoned

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AHEAD = 4  # csrc/vrnn_static.h kArmAhead
X = H = Z = 256
R = 512
STRIDE, FREE_NATS = 64, 2.0
TUNE_DEFAULT, ARM_OFF = 84, 128  # blvm_pchain_tune: the library's default bits; the bit that turns arming off
EXACT = ("decin", "kld", "kld_fn", "mu_q", "sd_q", "mu_p", "sd_p", "z")
ORACLE_BAR = 1e-3


def _lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    lib = _hip.load()
    assert lib.blvm_device_ok() == 1
    return lib


@contextlib.contextmanager
def arming(on):
    lib = _lib()
    lib.blvm_pchain_tune(TUNE_DEFAULT if on else TUNE_DEFAULT | ARM_OFF)
    try:
        yield lib
    finally:
        lib.blvm_pchain_tune(-1)  # (a negative value: the library takes its default, or BLVM_PCHAIN_TUNE, again)


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@functools.lru_cache(maxsize=None)
def _case(B, Tp, SF=0):
    """The cell, two sets of inputs of the same shapes (0: the case, 1: "another batch"), the readout weights of the scalar the
    backward starts from, and the float64 oracle's gradients for set 0 (computed once, never modified)."""
    torch.manual_seed(1000 + 10 * B + Tp)
    cell = VRNNCell(X, H, Z, R, residual_posterior=True)
    dec = [torch.nn.Linear(H + R, H), torch.nn.Linear(H, H), torch.nn.Linear(H, SF)] if SF else None
    g = torch.Generator().manual_seed(B + Tp)
    inputs = []
    for _ in (0, 1):
        enc, h0, eps = torch.randn(Tp, B, X, generator=g) * 0.5, torch.randn(B, R, generator=g) * 0.3, torch.randn(Tp, B, Z, generator=g)
        inputs.append((enc, h0, eps))
    T_ = Tp * STRIDE
    x_sl = torch.tensor([T_ - (k * T_) // (2 * B) for k in range(B)], dtype=torch.int64)  # ragged, the first row full
    w_dec = torch.randn(Tp + 1, B, H + R, generator=g) / (H + R) ** 0.5
    w_dec[Tp] = 0  # (blvm_vrnn_seq_bwd ignores the gradient of row T': the model reads h_n outside the graph)
    # float64 oracle of set 0
    sd = {"c." + k: v.detach().double().clone().requires_grad_(True) for k, v in cell.state_dict().items()}
    enc, h0, eps = (t.double().clone().requires_grad_(True) for t in inputs[0])
    h, rows, kl = h0, [], []
    for t in range(Tp):
        h_new, o = O.vrnn_cell_step(sd, enc[t], h, eps[t], True, prefix="c")
        rows.append(torch.cat([o["phi"], h], -1))
        kl.append(O.kl_gaussian(o["mu_q"], o["sd_q"], o["mu_p"], o["sd_p"]))
        h = h_new
    rows.append(torch.cat([torch.zeros(B, H, dtype=torch.float64), h], -1))
    mask = (torch.arange(Tp).unsqueeze(1) * STRIDE < x_sl.unsqueeze(0)).double().unsqueeze(-1)  # [T',B,1]
    kl = torch.stack(kl, 0)
    loss = (torch.stack(rows, 0) * w_dec.double()).sum() + 0.5 * (kl * mask).sum() + 0.25 * (O.discount_free_nats(kl, FREE_NATS) * mask).sum()
    loss.backward()
    names = [k for k, _ in cell.named_parameters()]
    ref = {"d_enc": enc.grad, "d_h0": h0.grad, **{"grad." + k: sd["c." + k].grad for k in names}}
    cell = cell.to(DEV)
    dec = [lin.to(DEV) for lin in dec] if dec else None
    inputs = [tuple(t.to(DEV) for t in inp) for inp in inputs]
    return cell, dec, inputs, x_sl.to(DEV, torch.int32), w_dec.to(DEV), ref


def _run(B, Tp, SF=0, variant=0):
    """One forward + backward of `ops.vrnn_sequence` under the switches in effect -> results, (static launches, armed launches)."""
    lib = _lib()
    cell, dec, inputs, x_sl, w_dec, _ = _case(B, Tp, SF)
    enc, h0, eps = (t.clone() for t in inputs[variant])
    enc.requires_grad_(True)
    h0.requires_grad_(True)
    cell.zero_grad(set_to_none=True)
    fold = ops.DecoderFold(dec, ops.LEAKY_SLOPE) if dec else None
    n0 = lib.blvm_pchain_static(-2), lib.blvm_pchain_static(-3)
    decin, kld, kld_fn, mu_q, sd_q, mu_p, sd_p, z = cell.sequence(enc, h0, eps, x_sl, STRIDE, FREE_NATS, decoder=fold)
    ((decin * w_dec).sum() + 0.5 * kld.sum() + 0.25 * kld_fn.sum()).backward()
    torch.cuda.synchronize()
    assert _hip.take_async_errors() == (0, 0)
    res = dict(decin=decin, kld=kld, kld_fn=kld_fn, mu_q=mu_q, sd_q=sd_q, mu_p=mu_p, sd_p=sd_p, z=z, d_enc=enc.grad, d_h0=h0.grad)
    if fold is not None:
        assert fold.given is not None and len(fold.given) == 3, "the launch did not fold the decoder"
        res.update(y1=fold.given[0], y2=fold.given[1], y3=fold.given[2])
    res.update({"grad." + k: p.grad for k, p in cell.named_parameters()})
    res = {k: v.detach().clone() for k, v in res.items()}
    for k, v in res.items():
        assert bool(torch.isfinite(v).all()), k
    return res, (lib.blvm_pchain_static(-2) - n0[0], lib.blvm_pchain_static(-3) - n0[1])


def _check(name, got, off, off_again, ref):
    """`got` (arming on, under some prefill) against the off path."""
    exact = [k for k in got if k in EXACT or k in ("y1", "y2", "y3")]
    bad = [k for k in exact if not torch.equal(got[k], off[k])]
    assert not bad, f"{name}: {bad} differ between arming on and off"
    for k in got:
        if k in exact:
            continue
        if k in ("d_enc", "d_h0") and torch.equal(off[k], off_again[k]):
            assert torch.equal(got[k], off[k]), f"{name}: {k} differs between arming on and off (the off path repeats it bit for bit)"
        else:
            e = rel_l2(got[k], ref[k])
            print(f"{name}: {k} rel_l2 vs float64 oracle {e:.3e} (off path {rel_l2(off[k], ref[k]):.3e})")
            assert e < ORACLE_BAR, (name, k, e)


def _on_against_off(monkeypatch, B, Tp, SF=0):
    ref = _case(B, Tp, SF)[5]
    want_armed = 2 if Tp > AHEAD else 0  # forward (T' steps) and backward (T' + 1 steps, T' slabs): armed when a slab lies kArmAhead ahead
    with arming(False):
        off, n = _run(B, Tp, SF)
        assert n == (2, 0), n
        off_again, n = _run(B, Tp, SF)
        assert n == (2, 0), n
    for k in off:  # the off path itself meets the bars (else the case, not the arming, is at fault)
        if k not in EXACT and k not in ("y1", "y2", "y3"):
            assert rel_l2(off[k], ref[k]) < ORACLE_BAR, k
    with arming(True):
        got, n = _run(B, Tp, SF)
        assert n == (2, want_armed), n  # the static kernels ran, armed or (T' <= kArmAhead) behind the full host fill
        _check("plain", got, off, off_again, ref)
        for mode in ("nan", "noise", "stale_same", "stale_other"):
            stale = None
            if mode.startswith("stale"):
                with poisoned(monkeypatch, "noise", record=True) as rec:
                    _run(B, Tp, SF, variant=0 if mode == "stale_same" else 1)
                stale = rec.buffers
            with poisoned(monkeypatch, "stale" if stale is not None else mode, stale=stale) as h:
                got, n = _run(B, Tp, SF)
            assert h.count > 0 and (stale is None or h.count == len(stale)), "the harness poisoned nothing"
            assert n == (2, want_armed), n
            _check(mode, got, off, off_again, ref)


@pytest.mark.parametrize("Tp", [AHEAD - 1, AHEAD + 1, 2 * AHEAD + 3, 37])
@pytest.mark.parametrize("B", [64, 49, 17, 5])
def test_arming_on_equals_the_full_host_fill(B, Tp, monkeypatch):
    """Every shape of the issue; T' = kArmAhead - 1 is the case in which nothing is armed and the full host fill runs."""
    _on_against_off(monkeypatch, B, Tp)


def test_arming_with_the_folded_decoder(monkeypatch):
    """B = 64, T' = 2 kArmAhead + 3, the benchmark's 120 column tiles of the last decoder layer: Y116, Y216 and Y1P are armed too, and
    the decoder's three activations are bit-equal."""
    _on_against_off(monkeypatch, 64, 2 * AHEAD + 3, SF=1920)


def test_bf16_mode_keeps_the_full_host_fill():
    """16-bit operands run on the interpreter: nothing is armed, and the switch changes nothing."""
    lib = _lib()
    old = lib.blvm_get_operand_dtype()
    lib.blvm_set_operand_dtype(1)
    try:
        with arming(False):
            off, n_off = _run(17, 2 * AHEAD + 3)
        with arming(True):
            on, n_on = _run(17, 2 * AHEAD + 3)
    finally:
        lib.blvm_set_operand_dtype(old)
    assert n_off == (0, 0) and n_on == (0, 0), (n_off, n_on)
    bad = [k for k in EXACT if not torch.equal(on[k], off[k])]
    assert not bad, bad
    bad = [(k, rel_l2(on[k], off[k])) for k in on if k not in EXACT and rel_l2(on[k], off[k]) > 1e-6]  # (float atomics: `test_gpu_vrnn_static.py`)
    assert not bad, bad
