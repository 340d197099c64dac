"""GPU: the gradient wrt the encoding as a follower on the static backward walk's posterior half (csrc/vrnn_static.h "d_enc
follower", blvm_vrnn_enc_bwd_fold).

At B <= 64 the backward deal gives the posterior half no tile of the summing link, the phi_z run or dz: between its partial-sum tile
and its run it waits.  With the fold each of its workgroups computes, one walk step behind the chain, its tile of
EP = DGI W_ih[:, :X] (K = 3R) and then d_enc = DQ0 Wq0[:, R:] + EP (K = H), every word written once, instead of two K6 launches behind
the walk of which the second accumulates into the first with float atomics.  Same arithmetic, another summation order: the yardstick
is the float64 oracle, and the folded path's error may be at most twice the unfolded path's on the same inputs (against one fp32
rounding, 6e-8, where the unfolded error is below that).

`ops.vrnn_sequence` at H = Z = X = 256, R = 512 with the decoder handed down (fifteen descriptors: the decoder leader and the
follower) and, where a gradient reaches decin from outside the decoder, without it (twelve).  Cases, inputs and the float64 oracle are
those of test_gpu_vrnn_decoder_bwd_fold.py: T' = 5 (the shortest walk that folds: the lagged links get steps 1 .. 5) and 11;
B = 64, 49, 17, 5; ragged lengths; h0 given at B = 64 and 17.

Measured, rel-L2 error against the oracle, folded | unfolded (one MI355X; the largest ratio folded / max(unfolded, 6e-8) over all
gradients of a case, the gradient it belongs to, and d_enc itself):
  B=64 T'=5    1.01 at grad.prior.4.bias: 1.317e-06 | 1.301e-06; d_enc 8.059e-07 | 8.723e-07
  B=49 T'=5    1.04 at grad.dec3: 2.182e-07 | 2.097e-07; d_enc 7.365e-07 | 8.019e-07
  B=17 T'=5    1.01 at grad.dec5: 9.452e-08 | 9.340e-08; d_enc 7.043e-07 | 7.663e-07
  B=5 T'=5     1.01 at grad.phi_z.4.bias: 3.646e-07 | 3.618e-07; d_enc 7.522e-07 | 8.236e-07
  B=64 T'=11   1.04 at grad.dec3: 2.069e-07 | 1.988e-07; d_enc 7.166e-07 | 7.949e-07
  B=49 T'=11   1.03 at grad.dec3: 2.266e-07 | 2.201e-07; d_enc 7.434e-07 | 8.194e-07
  B=17 T'=11   1.03 at grad.dec3: 2.139e-07 | 2.072e-07; d_enc 7.355e-07 | 8.188e-07
  B=5 T'=11    1.05 at grad.dec5: 7.887e-08 | 7.492e-08; d_enc 6.946e-07 | 7.706e-07
(the ratios above 1 belong to gradients the fold does not compute: they are summed with float atomics and move from run to run;
d_enc itself is closer to the oracle folded than unfolded in every case.)  Without the decoder leader (twelve descriptors), folded
against unfolded: d_enc 4.2e-07 .. 4.4e-07 rel-L2, everything else bit-identical or inside the atomics' 1e-6.
"""
import contextlib
import functools

import pytest
import torch

from blvm import _hip, ops

from test_gpu_buffer_contract import poisoned
from test_gpu_vrnn_decoder_bwd_fold import EXACT, H, R, SLOPE, STRIDE, FREE_NATS, _case, _lib, rel_l2, with_h0

pytestmark = pytest.mark.gpu
SF = 240
CASES = [(B, Tp) for Tp in (5, 11) for B in (64, 49, 17, 5)]
ONCE = ("dy2", "dy1", "d_h0", "d_enc")  # written once each by the launch: no atomics (d_enc: with the fold)
FLOOR = 6e-8  # one fp32 rounding of the quantity


@contextlib.contextmanager
def switches(fold=True, static=True):
    lib = _lib()
    was = lib.blvm_vrnn_enc_bwd_fold(int(fold)), lib.blvm_pchain_static(1 if static else 0)
    try:
        yield lib
    finally:
        lib.blvm_vrnn_enc_bwd_fold(was[0])
        lib.blvm_pchain_static(was[1])


def _run(B, Tp, sf=SF, variant=0, decin_too=False, enc_grad=True):
    """One forward + backward under the switches in effect -> results, (static launches, backward calls that folded d_enc)."""
    lib = _lib()
    cell, dec, inputs, x_sl, w3, w_decin, _ = _case(B, Tp, sf)
    enc, h0, eps = (t.clone() if t is not None else None for t in inputs[variant])
    enc.requires_grad_(enc_grad)
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

    n0 = lib.blvm_pchain_static(-2), lib.blvm_vrnn_enc_bwd_fold(-2)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "wgrad_group", spy)
        decin, kld, kld_fn, mu_q, sd_q, mu_p, sd_p, z = cell.sequence(enc, h0, eps, x_sl, STRIDE, FREE_NATS, decoder=fold)
        out = fold.dec if fold.dec is not None else ops.mlp_given(decin[:Tp].view(Tp * B, H + R), dec, fold.given, ops.ACT_LEAKY, SLOPE, head_gates=True) \
            if fold.given is not None else ops._MLPFunction.apply(decin[:Tp].view(Tp * B, H + R), ops.ACT_LEAKY, SLOPE, True,
                                                                  *[t for lin in dec for t in (lin.weight, lin.bias)])  # fmt: skip
        loss = (out * w3).sum() + 0.5 * kld.sum() + 0.25 * kld_fn.sum()
        if decin_too:
            loss = loss + (decin * w_decin).sum()
        loss.backward()
    torch.cuda.synchronize()
    assert _hip.take_async_errors() == (0, 0)
    res = dict(decin=decin, kld=kld, kld_fn=kld_fn, mu_q=mu_q, sd_q=sd_q, mu_p=mu_p, sd_p=sd_p, z=z, dec=out, **seen)
    if enc_grad:
        res["d_enc"] = enc.grad
    else:
        assert enc.grad is None
    if h0 is not None:
        res["d_h0"] = h0.grad
    res.update({"grad." + k: p.grad for k, p in cell.named_parameters()})
    res.update({f"grad.dec{i}": p.grad for i, p in enumerate(t for lin in dec for t in (lin.weight, lin.bias))})
    res = {k: v.detach().clone() for k, v in res.items()}
    for k, v in res.items():
        assert bool(torch.isfinite(v).all()), k
    return res, (lib.blvm_pchain_static(-2) - n0[0], lib.blvm_vrnn_enc_bwd_fold(-2) - n0[1])


@functools.lru_cache(maxsize=None)
def _folded(B, Tp, sf=SF, decin_too=False):
    with switches(fold=True, static=True):
        res, n = _run(B, Tp, sf, decin_too=decin_too)
    assert n == (2, 1), n  # static forward and backward; the backward folded d_enc
    return res


@functools.lru_cache(maxsize=None)
def _unfolded(B, Tp, sf=SF, decin_too=False):
    with switches(fold=False, static=True):
        res, n = _run(B, Tp, sf, decin_too=decin_too)
    assert n == (2, 0), n
    return res


def _same(a, b, what, once=ONCE):
    """Two paths that must compute the same thing: bit-identical in the forward and in everything written once; what is summed with
    float atomics (the weight gradients; without the fold d_enc) within 1e-6 relative, the bar of test_gpu_vrnn_decoder_bwd_fold.py."""
    assert a.keys() == b.keys(), what
    bad = [k for k in a if (k in EXACT or k in once) and not torch.equal(a[k], b[k])]
    assert not bad, f"{what}: {bad} differ"
    bad = [(k, rel_l2(a[k], b[k])) for k in a if k not in EXACT and k not in once and rel_l2(a[k], b[k]) > 1e-6]
    assert not bad, (what, bad[:8])


@pytest.mark.parametrize("B,Tp", CASES)
def test_folded_against_unfolded_and_the_oracle(B, Tp):
    """The forward's outputs and the KL bit-identical with the fold on and off; d_enc, d_h0 and every parameter gradient at most twice
    as far from the float64 oracle folded as unfolded (as max(unfolded, 6e-8))."""
    ref = _case(B, Tp, SF)[6]
    on, off = _folded(B, Tp), _unfolded(B, Tp)
    assert on.keys() == off.keys() and ("d_h0" in on) == with_h0(B) and "d_enc" in on
    bad = [k for k in EXACT if not torch.equal(on[k], off[k])]
    assert not bad, f"the fold changed {bad}"
    rows = [(k, rel_l2(on[k], ref[k]), rel_l2(off[k], ref[k])) for k in on if k not in EXACT]
    print(f"B={B} T'={Tp}: error against the oracle, folded | unfolded")
    for k, a, b in rows:
        print(f"  {k:40s} {a:.3e} | {b:.3e}")
    k, a, b = max(rows, key=lambda r: r[1] / max(r[2], FLOOR))
    d = next(r for r in rows if r[0] == "d_enc")
    print(f"PAIR B={B} T'={Tp}: largest ratio {a / max(b, FLOOR):.2f} at {k}: {a:.3e} | {b:.3e}; d_enc {d[1]:.3e} | {d[2]:.3e}")
    worse = [(k, a, b) for k, a, b in rows if a > 2 * max(b, FLOOR)]
    assert not worse, worse


@pytest.mark.parametrize("B,Tp", CASES)
def test_static_walk_matches_interpreter_on_the_extended_program(B, Tp):
    """The same fifteen descriptors on the static kernel and on the interpreter (which walks the follower's links last in every step):
    bit-identical wherever nothing is summed with atomics, and that now includes d_enc."""
    static = _folded(B, Tp)
    with switches(fold=True, static=False):
        interp, n = _run(B, Tp)
    assert n == (0, 1), n
    _same(static, interp, "static walk against interpreter")


@pytest.mark.parametrize("B,Tp", [(64, 5), (17, 11), (5, 5)])
def test_the_program_without_the_decoder_leader(B, Tp):
    """A gradient reaches decin from outside the decoder, so the decoder's data gradients stay K6 launches and the program is the ten
    descriptors plus the follower's two: static walk and interpreter bit-identical in d_enc; fold on against off the forward is
    bit-identical and d_enc within 1e-5 rel-L2, the bar of test_gpu_vrnn_decoder_bwd_fold.py for an fp32 sum over K <= 1920 in another
    order (here K = 3R + H = 1792: sqrt(K) eps = 2.5e-6 typical)."""
    on, off = _folded(B, Tp, decin_too=True), _unfolded(B, Tp, decin_too=True)
    with switches(fold=True, static=False):
        interp, n = _run(B, Tp, decin_too=True)
    assert n == (0, 1), n
    _same(on, interp, "static walk against interpreter, twelve descriptors")
    bad = [k for k in EXACT if not torch.equal(on[k], off[k])]
    assert not bad, f"the fold changed {bad}"
    errs = {k: rel_l2(on[k], off[k]) for k in on if k not in EXACT}
    print(f"B={B} T'={Tp}, no leader: folded against unfolded, d_enc {errs['d_enc']:.3e}, largest {max(errs.values()):.3e}")
    assert max(errs.values()) < 1e-5, errs


@pytest.mark.parametrize("B,Tp,sf", [(64, 11, 1920), (5, 11, 240), (49, 5, 240), (17, 5, 1920)])
def test_results_do_not_depend_on_what_the_buffers_held(B, Tp, sf, monkeypatch):
    """d_enc, the grown workspace (EP among it), the reserve and every other buffer `blvm.ops` allocates pre-filled with quiet NaNs,
    with noise, with the bytes they held after an identical run and after a run of the same shapes on other inputs (only that one can
    show a missed sentinel: after an identical run it would find the right values)."""
    plain = _folded(B, Tp, sf)
    with switches(fold=True, static=True):
        for mode in ("nan", "noise", "stale_same", "stale_other"):
            stale = None
            if mode.startswith("stale"):
                with poisoned(monkeypatch, "noise", record=True) as rec:
                    _run(B, Tp, sf, variant=0 if mode == "stale_same" else 1)
                stale = rec.buffers
            with poisoned(monkeypatch, "stale" if stale is not None else mode, stale=stale) as h:
                got, n = _run(B, Tp, sf)
            assert h.count > 0 and (stale is None or h.count == len(stale)), "the harness poisoned nothing"
            assert n == (2, 1), (mode, n)
            _same(plain, got, mode)


@pytest.mark.parametrize("case", ["Tp3", "no_grad", "bf16", "B65"])
def test_not_folded_is_the_switch_at_zero(case):
    """A walk too short to arm, an encoding that asks for no gradient, 16-bit operands, a batch past the 16-row tiles: the counter
    stands still and the step is what the switch at 0 gives (d_enc then comes from K6's float atomics: within 1e-6)."""
    lib = _lib()
    B, Tp = {"Tp3": (17, 3), "no_grad": (17, 5), "bf16": (17, 5), "B65": (65, 5)}[case]
    old = lib.blvm_get_operand_dtype()
    if case == "bf16":
        lib.blvm_set_operand_dtype(1)
    try:
        with switches(fold=True):
            on, n_on = _run(B, Tp, enc_grad=case != "no_grad")
        with switches(fold=False):
            off, n_off = _run(B, Tp, enc_grad=case != "no_grad")
    finally:
        lib.blvm_set_operand_dtype(old)
    assert n_on[1] == 0 and n_off[1] == 0
    assert ("d_enc" in on) == (case != "no_grad")
    _same(on, off, case, once=("dy2", "dy1", "d_h0"))
