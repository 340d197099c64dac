"""GPU: the decoder MLP's data gradients as a leader on the static backward walk's spare range (csrc/vrnn_static.h "decoder leader",
blvm_vrnn_seq_bwd_dec, `ops._VRNNSeqFunction` with the decoder's parameters).

At B <= 64 the backward deal leaves a spare range that owns one partial-sum tile per workgroup and step.  With the fold it also runs
dY2 = gate(dZ3 Wd3), dY1 = gate(dY2 Wd2) and dD = dY1 Wd1 of the time step two walk steps ahead; dD's phi part is the polled addend
of the spare range's partial sum, its h part a second polled addend of GB (so GA = g u, and one rounding of the state gradient
moves).  Same arithmetic as the three K6 products, another summation order: the yardstick is the float64 oracle, and the folded
path's error may be at most twice the unfolded path's on the same inputs.

`ops.vrnn_sequence` with a `DecoderFold(head_gates=True)` at H = Z = X = 256, R = 512; the scalar the backward starts from is
sum(w3 * Z3) + 0.5 sum(kld) + 0.25 sum(kld_fn), Z3 the decoder's last PRE-activation, so dZ3 = w3 (what the fused DMoL head hands
down).  T' = 5 (the shortest armed walk; the leader runs off the end after three steps) and 11; B = 64, 49 (four row tiles, the last
with one row), 17 (two, the last with one row), 5 (one partial row tile: another deal); S F = 1920 (K = 7.5 x 256, the benchmark's) and
240; ragged lengths; h0 given (B = 64, 17) and not given (B = 49, 5).  T' = 3 does not arm and must report "not folded".

Measured, rel-L2 error against the oracle, folded | unfolded (one MI355X; the largest ratio folded / unfolded over all gradients of
a case, and the gradient it belongs to):
  B=64 T'=5 SF=1920      1.00 at grad.posterior.6.params.bias: 7.864e-07 | 7.828e-07
  B=49 T'=5 SF=1920      1.01 at grad.posterior.0.bias: 5.795e-07 | 5.758e-07
  B=17 T'=5 SF=1920      1.01 at grad.prior.2.bias: 1.143e-06 | 1.130e-06
  B=5 T'=5 SF=1920       1.01 at grad.posterior.4.bias: 6.858e-07 | 6.800e-07
  B=64 T'=5 SF=240       1.01 at grad.prior.4.bias: 1.317e-06 | 1.304e-06
  B=49 T'=5 SF=240       1.01 at grad.dec5: 1.479e-07 | 1.465e-07
  B=17 T'=5 SF=240       1.04 at grad.dec5: 9.646e-08 | 9.308e-08
  B=5 T'=5 SF=240        1.04 at grad.dec5: 6.468e-08 | 6.189e-08
  B=64 T'=11 SF=1920     1.01 at grad.prior.4.bias: 1.285e-06 | 1.271e-06
  B=49 T'=11 SF=1920     1.01 at grad.posterior.4.bias: 6.742e-07 | 6.690e-07
  B=17 T'=11 SF=1920     1.01 at grad.posterior.2.bias: 5.370e-07 | 5.312e-07
  B=5 T'=11 SF=1920      1.00 at grad.prior.4.bias: 1.369e-06 | 1.363e-06
  B=64 T'=11 SF=240      1.02 at grad.dec5: 1.489e-07 | 1.455e-07
  B=49 T'=11 SF=240      1.03 at grad.posterior.2.bias: 7.163e-07 | 6.955e-07
  B=17 T'=11 SF=240      1.02 at grad.posterior.2.bias: 6.267e-07 | 6.151e-07
  B=5 T'=11 SF=240       1.11 at grad.dec5: 8.079e-08 | 7.299e-08
  B=64 T'=11 SF=1920, the chain's own outputs: d_enc 8.029e-07 | 9.735e-07; dy2 3.882e-07 | 7.913e-07; dy1 4.132e-07 | 8.339e-07; d_h0 5.178e-07 | 9.389e-07
"""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

import blvm_oracle as O
from blvm import _hip, ops
from blvm.models import VRNNAudio
from blvm.models.vrnn import VRNNCell

from test_gpu_buffer_contract import poisoned

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
X = H = Z = 256
R = 512
STRIDE, FREE_NATS, SLOPE = 64, 2.0, ops.LEAKY_SLOPE
CASES = [(B, Tp, SF) for Tp in (5, 11) for SF in (1920, 240) for B in (64, 49, 17, 5)]
EXACT = ("decin", "kld", "kld_fn", "mu_q", "sd_q", "mu_p", "sd_p", "z", "dec")  # the forward: the fold never touches it
CHAIN = ("dy2", "dy1", "d_h0")  # written once each by the launch (or by K6): no atomics


def _lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    lib = _hip.load()
    assert lib.blvm_device_ok() == 1
    return lib


@contextlib.contextmanager
def switches(fold=True, static=True):
    lib = _lib()
    was = lib.blvm_vrnn_dec_bwd_fold(int(fold)), lib.blvm_pchain_static(1 if static else 0)
    try:
        yield lib
    finally:
        lib.blvm_vrnn_dec_bwd_fold(was[0])
        lib.blvm_pchain_static(was[1])


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def with_h0(B):
    return B in (64, 17)


@functools.lru_cache(maxsize=None)
def _case(B, Tp, SF, width=H):
    """The cell and the decoder (on the device), two sets of inputs of the same shapes (0: the case, 1: "another batch"), the readout
    weights, and the float64 oracle's gradients for set 0 (computed once, never modified)."""
    torch.manual_seed(2000 + 10 * B + Tp + SF)
    cell = VRNNCell(X, H, Z, R, residual_posterior=True)
    dec = [torch.nn.Linear(H + R, width), torch.nn.Linear(width, width), torch.nn.Linear(width, SF)]
    g = torch.Generator().manual_seed(B + Tp + SF)
    inputs = []
    for _ in (0, 1):
        enc, h0, eps = torch.randn(Tp, B, X, generator=g) * 0.5, torch.randn(B, R, generator=g) * 0.3, torch.randn(Tp, B, Z, generator=g)
        inputs.append((enc, h0 if with_h0(B) else None, eps))
    T_ = Tp * STRIDE
    x_sl = torch.tensor([T_ - (k * T_) // (2 * B) for k in range(B)], dtype=torch.int64)  # ragged, the first row full
    w3 = torch.randn(Tp * B, SF, generator=g) / SF**0.5
    w_decin = torch.randn(Tp + 1, B, H + R, generator=g) / (H + R) ** 0.5  # (only where a test lets decin reach the scalar as well)
    w_decin[Tp] = 0
    ref = None
    if width == H:
        sd = {"c." + k: v.detach().double().clone().requires_grad_(True) for k, v in cell.state_dict().items()}
        dp = [t.detach().double().clone().requires_grad_(True) for lin in dec for t in (lin.weight, lin.bias)]
        enc, h0, eps = (t.double().clone().requires_grad_(True) if t is not None else None for t in inputs[0])
        h = h0 if h0 is not None else torch.zeros(B, R, dtype=torch.float64)
        rows, kl = [], []
        for t in range(Tp):
            h_new, o = O.vrnn_cell_step(sd, enc[t], h, eps[t], True, prefix="c")
            rows.append(torch.cat([o["phi"], h], -1))
            kl.append(O.kl_gaussian(o["mu_q"], o["sd_q"], o["mu_p"], o["sd_p"]))
            h = h_new
        a = torch.stack(rows, 0).reshape(Tp * B, H + R)
        z1 = F.linear(a, dp[0], dp[1])
        z2 = F.linear(F.leaky_relu(z1, SLOPE), dp[2], dp[3])
        z3 = F.linear(F.leaky_relu(z2, SLOPE), dp[4], dp[5])
        z1.retain_grad()
        z2.retain_grad()
        mask = (torch.arange(Tp).unsqueeze(1) * STRIDE < x_sl.unsqueeze(0)).double().unsqueeze(-1)  # [T',B,1]
        kl = torch.stack(kl, 0)
        loss = (z3 * w3.double()).sum() + 0.5 * (kl * mask).sum() + 0.25 * (O.discount_free_nats(kl, FREE_NATS) * mask).sum()
        loss.backward()
        ref = {"d_enc": enc.grad, "dy2": z2.grad, "dy1": z1.grad, **{"grad." + k: sd["c." + k].grad for k, _ in cell.named_parameters()},
               **{f"grad.dec{i}": dp[i].grad for i in range(6)}}
        if h0 is not None:
            ref["d_h0"] = h0.grad
    cell = cell.to(DEV)
    dec = [lin.to(DEV) for lin in dec]
    inputs = [tuple(t.to(DEV) if t is not None else None for t in inp) for inp in inputs]
    return cell, dec, inputs, x_sl.to(DEV, torch.int32), w3.to(DEV), w_decin.to(DEV), ref


def _run(B, Tp, SF, variant=0, width=H, decin_too=False):
    """One forward + backward under the switches in effect -> results, (static launches, backward calls that folded)."""
    lib = _lib()
    cell, dec, inputs, x_sl, w3, w_decin, _ = _case(B, Tp, SF, width)
    enc, h0, eps = (t.clone() if t is not None else None for t in inputs[variant])
    enc.requires_grad_(True)
    if h0 is not None:
        h0.requires_grad_(True)
    for m in (cell, *dec):
        m.zero_grad(set_to_none=True)
    fold = ops.DecoderFold(dec, SLOPE, head_gates=True)
    seen = {}
    real = ops.wgrad_group

    def spy(jobs, rows):
        if len(jobs) == 3:  # the decoder's three layers, last first: (dz, input, dW, db)
            seen.update(dy2=jobs[1][0], dy1=jobs[2][0])
        return real(jobs, rows)

    n0 = lib.blvm_pchain_static(-2), lib.blvm_vrnn_dec_bwd_fold(-2)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "wgrad_group", spy)
        decin, kld, kld_fn, mu_q, sd_q, mu_p, sd_p, z = cell.sequence(enc, h0, eps, x_sl, STRIDE, FREE_NATS, decoder=fold)
        joint = fold.dec is not None
        out = fold.dec if joint else ops.mlp_given(decin[:Tp].view(Tp * B, H + R), dec, fold.given, ops.ACT_LEAKY, SLOPE, head_gates=True) \
            if fold.given is not None else ops._MLPFunction.apply(decin[:Tp].view(Tp * B, H + R), ops.ACT_LEAKY, SLOPE, True,
                                                                  *[t for lin in dec for t in (lin.weight, lin.bias)])  # fmt: skip
        loss = (out * w3).sum() + 0.5 * kld.sum() + 0.25 * kld_fn.sum()
        if decin_too:
            loss = loss + (decin * w_decin).sum()
        loss.backward()
    torch.cuda.synchronize()
    assert _hip.take_async_errors() == (0, 0)
    res = dict(decin=decin, kld=kld, kld_fn=kld_fn, mu_q=mu_q, sd_q=sd_q, mu_p=mu_p, sd_p=sd_p, z=z, dec=out, d_enc=enc.grad, **seen)
    if h0 is not None:
        res["d_h0"] = h0.grad
    res.update({"grad." + k: p.grad for k, p in cell.named_parameters()})
    res.update({f"grad.dec{i}": p.grad for i, p in enumerate(t for lin in dec for t in (lin.weight, lin.bias))})
    res = {k: v.detach().clone() for k, v in res.items()}
    for k, v in res.items():
        assert bool(torch.isfinite(v).all()), k
    return res, (lib.blvm_pchain_static(-2) - n0[0], lib.blvm_vrnn_dec_bwd_fold(-2) - n0[1]), joint


@functools.lru_cache(maxsize=None)
def _folded(B, Tp, SF):
    with switches(fold=True, static=True):
        res, n, joint = _run(B, Tp, SF)
    assert joint and n == (2, 1), n  # the cell's node took the decoder in; static forward and backward; the backward folded
    return res


@functools.lru_cache(maxsize=None)
def _unfolded(B, Tp, SF):
    with switches(fold=False, static=True):
        res, n, joint = _run(B, Tp, SF)
    assert not joint and n == (2, 0), n
    return res


def _same_but_for_atomics(a, b, what):
    """Two paths that must compute the same thing: bit-identical in the forward and in everything written once; what is summed with
    float atomics (d_enc, the weight gradients) within 1e-6 relative, the bar of `test_gpu_vrnn_decoder_fold.py`."""
    assert a.keys() == b.keys(), what
    bad = [k for k in a if (k in EXACT or k in CHAIN) and not torch.equal(a[k], b[k])]
    assert not bad, f"{what}: {bad} differ"
    bad = [(k, rel_l2(a[k], b[k])) for k in a if k not in EXACT and k not in CHAIN and rel_l2(a[k], b[k]) > 1e-6]
    assert not bad, (what, bad[:8])


@pytest.mark.parametrize("B,Tp,SF", CASES)
def test_folded_against_unfolded_and_the_oracle(B, Tp, SF):
    """The forward's outputs and the KL bit-identical with the fold on and off; every parameter gradient, d_enc and d_h0 at most twice
    as far from the float64 oracle folded as unfolded; dY2 and dY1 (every row written) below 1e-5, the bar of an fp32 sum over
    K <= 1920 (sqrt(K) eps = 2.6e-6 typical)."""
    ref = _case(B, Tp, SF)[6]
    on, off = _folded(B, Tp, SF), _unfolded(B, Tp, SF)
    assert on.keys() == off.keys() and ("d_h0" in on) == with_h0(B)
    bad = [k for k in EXACT if not torch.equal(on[k], off[k])]
    assert not bad, f"the fold changed {bad}"
    rows = [(k, rel_l2(on[k], ref[k]), rel_l2(off[k], ref[k])) for k in on if k not in EXACT]
    print(f"B={B} T'={Tp} SF={SF}: error against the oracle, folded | unfolded")
    for k, a, b in rows:
        print(f"  {k:40s} {a:.3e} | {b:.3e}")
    k, a, b = max(rows, key=lambda r: r[1] / r[2])
    print(f"PAIR B={B} T'={Tp} SF={SF}: largest ratio {a / b:.2f} at {k}: {a:.3e} | {b:.3e}")
    worse = [(k, a, b) for k, a, b in rows if k not in ("dy2", "dy1") and a > 2 * b]
    assert not worse, worse
    assert max(rel_l2(on[k], ref[k]) for k in ("dy2", "dy1")) < 1e-5


@pytest.mark.parametrize("B,Tp,SF", CASES)
def test_static_walk_matches_interpreter_on_the_extended_program(B, Tp, SF):
    """The same thirteen descriptors on the static kernel and on the interpreter (which walks the leader's links in step with the
    chain, their pointers two steps ahead): bit-identical wherever nothing is summed with atomics."""
    static = _folded(B, Tp, SF)
    with switches(fold=True, static=False):
        interp, n, joint = _run(B, Tp, SF)
    assert joint and n == (0, 1), n
    _same_but_for_atomics(static, interp, "static walk against interpreter")


@pytest.mark.parametrize("B,Tp,SF", [(64, 11, 1920), (5, 11, 240), (49, 5, 240), (17, 5, 1920)])
def test_results_do_not_depend_on_what_the_buffers_held(B, Tp, SF, monkeypatch):
    """dY2, dY1, the grown workspace, the reserve and every other buffer `blvm.ops` allocates pre-filled with quiet NaNs, with noise,
    with the bytes they held after an identical run and after a run of the same shapes on other inputs (only that one can show a
    missed sentinel: after an identical run it would find the right values)."""
    plain = _folded(B, Tp, SF)
    with switches(fold=True, static=True):
        for mode in ("nan", "noise", "stale_same", "stale_other"):
            stale = None
            if mode.startswith("stale"):
                with poisoned(monkeypatch, "noise", record=True) as rec:
                    _run(B, Tp, SF, variant=0 if mode == "stale_same" else 1)
                stale = rec.buffers
            with poisoned(monkeypatch, "stale" if stale is not None else mode, stale=stale) as h:
                got, n, joint = _run(B, Tp, SF)
            assert h.count > 0 and (stale is None or h.count == len(stale)), "the harness poisoned nothing"
            assert joint and n == (2, 1), (mode, n)
            _same_but_for_atomics(plain, got, mode)


@pytest.mark.parametrize("case", ["Tp3", "decin_too", "bf16", "B65", "width128"])
def test_not_folded_is_the_switch_at_zero(case):
    """A walk too short to arm, a gradient that reaches decin from outside the decoder, 16-bit operands, a batch past the 16-row
    tiles, a decoder whose hidden width is not H: the counter stands still (blvm_vrnn_seq_bwd_dec has done nothing) and the step is
    what the switch at 0 gives."""
    lib = _lib()
    B, Tp, SF, width = {"Tp3": (17, 3, 240, H), "decin_too": (17, 5, 240, H), "bf16": (17, 5, 240, H), "B65": (65, 5, 240, H),
                        "width128": (17, 5, 240, 128)}[case]  # fmt: skip
    old = lib.blvm_get_operand_dtype()
    if case == "bf16":
        lib.blvm_set_operand_dtype(1)
    try:
        with switches(fold=True):
            on, n_on, joint = _run(B, Tp, SF, width=width, decin_too=case == "decin_too")
        with switches(fold=False):
            off, n_off, _ = _run(B, Tp, SF, width=width, decin_too=case == "decin_too")
    finally:
        lib.blvm_set_operand_dtype(old)
    assert n_on[1] == 0 and n_off[1] == 0
    assert joint == (case in ("Tp3", "decin_too"))  # (the others: the forward did not fold, so the cell's node never took the decoder in)
    _same_but_for_atomics(on, off, case)


def test_the_model_takes_the_folded_path_end_to_end():
    """VRNNAudio with the DMoL head (S = 8, T' = 5, B = 5): the backward folds, and every parameter gradient is at most twice as far
    from the float64 oracle as with the switch off."""
    lib = _lib()
    B, S, Tp = 5, 8, 5
    torch.manual_seed(11)
    m = VRNNAudio(likelihood="DMoL", input_size=S, hidden_size=H, latent_size=H, residual_posterior=True)
    T_ = S * Tp - 3
    x_sl = torch.tensor([T_ - (k * T_) // (2 * B) for k in range(B)], dtype=torch.int64)
    x, _ = O.synth_batch(B, T_, seed=3)
    x = x * (torch.arange(T_).unsqueeze(0) < x_sl.unsqueeze(1))
    eps = torch.randn(Tp, B, H, generator=torch.Generator().manual_seed(5))
    sd = {k: v.double().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    O.vrnn_audio_forward(sd, x.double(), x_sl, eps.double(), beta=1.0, free_nats=2.0, stack=S)["loss"].backward()
    m = m.to(DEV)
    got = {}
    for fold in (True, False):
        with switches(fold=fold) as _:
            m.zero_grad(set_to_none=True)
            n0 = lib.blvm_vrnn_dec_bwd_fold(-2)
            loss, _, _ = m(x.to(DEV), x_sl, beta=1.0, free_nats=2.0, eps=eps.to(DEV))
            loss.backward()
            torch.cuda.synchronize()
            assert _hip.take_async_errors() == (0, 0)
            assert lib.blvm_vrnn_dec_bwd_fold(-2) - n0 == int(fold)
            got[fold] = (float(loss), {k: p.grad.detach().clone() for k, p in m.named_parameters()})
    assert abs(got[True][0] - got[False][0]) <= 1e-12 * abs(got[False][0])  # (the forward is the same; float64 sums accumulated with atomics)
    worse = [(k, rel_l2(got[True][1][k], sd[k].grad), rel_l2(got[False][1][k], sd[k].grad)) for k in got[True][1]]
    worse = [w for w in worse if w[1] > 2 * w[2]]
    assert not worse, worse
