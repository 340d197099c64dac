"""The caller-owned-buffer contract (include/blvm_hip.h, Conventions): apart from inputs and from buffers the header marks
ACCUMULATED (and the DMoL ticket words, `test_gpu_dmol_fused.py`), no result of an entry point depends on what its output,
reserve, workspace or scratch buffers held before the call.

The recurrent kernels hand tiles between workgroups through slabs the host driver pre-fills with the word 0xFFFFFFFF; a consumer
re-reads a fragment until no word of it is that sentinel (csrc/pchain.h).  A region that a launch polls or reads but its driver
forgot to fill, zero or write is found "ready" at once and the launch computes from whatever the buffer held — in training, the
previous step's activations in the right layout (the caching allocator returns the same block every step).  `test_gpu_abort.py`
attacks the protocol from the input side (a planted sentinel); this file attacks it from the buffer side.

Harness: every raw buffer originates in `blvm/ops.py` (`torch.empty` / `torch.empty_like`), so a stand-in for the name `torch`
inside `blvm.ops` hands out the same tensors pre-filled:
  nan    every 32-bit word 0x7FC00000 (a quiet NaN that is NOT the sentinel; float64: the float64 quiet NaN);
  noise  finite unit-normal values from a seeded generator ("some other batch");
  stale  buffer i starts as a bit-copy of what buffer i ended as in a first run of the same call on other inputs of the same
         shapes — the training-loop situation made deterministic.
Every case runs under the three modes and asserts
  (a) the bound of the sibling parity test against the same reference (float64 torch, oracle/blvm_oracle.py or a golden):
      loss / ELBO 1e-5 relative, sequence-kernel outputs rel_l2 < 1e-5, gradients rel_l2 < 2e-5 (bare GRU / LSTM kernels) or
      < 1e-3 per parameter (whole models) — `tests/test_gpu_parity.py`;
  (b) every fp32 tensor the sequence kernels write in the forward pass is bit-identical across the modes (float64
      per-utterance sums are accumulated with atomics and gradients go through split-K atomics: (a) only);
  (c) no NaN / Inf in any result, and no persistent launch gave up on a spin;
and that the harness did poison buffers (a refactor that moves allocation elsewhere must not silently empty the test)."""
import contextlib
import copy
import functools
import math
import os

import numpy as np
import pytest
import torch

import blvm_oracle as O
from blvm import _hip, ops

from conftest import GOLDEN

gpu = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("nan", "noise", "stale")
NAN_WORD = 0x7FC00000
SENTINEL_WORD = -1  # 0xFFFFFFFF as int32


# ----------------------------------------------------------------------------------------------------------------------
# the poison harness
# ----------------------------------------------------------------------------------------------------------------------


class PoisonTorch:
    """Stand-in for the module `torch` inside `blvm.ops`: everything is torch's, except that `empty` / `empty_like` return their
    tensor pre-filled according to `mode`.  `count` buffers were poisoned so far; `record=True` keeps them (allocation order) in
    `buffers`, the `stale=` argument of a later stand-in."""

    def __init__(self, mode, seed=20240, stale=None, record=False):
        assert mode in MODES and (mode == "stale") == (stale is not None)
        self.mode, self.count, self.buffers = mode, 0, []
        self._stale, self._record, self._seed, self._gens = stale, record, seed, {}

    def __getattr__(self, name):  # (only names not defined here arrive)
        return getattr(torch, name)

    def empty(self, *args, **kwargs):
        return self._poison(torch.empty(*args, **kwargs))

    def empty_like(self, *args, **kwargs):
        return self._poison(torch.empty_like(*args, **kwargs))

    def _randn(self, like, dtype):
        g = self._gens.get(like.device)
        if g is None:
            g = self._gens[like.device] = torch.Generator(device=like.device).manual_seed(self._seed)
        return torch.randn(like.shape, generator=g, device=like.device, dtype=dtype)

    def _poison(self, t):
        if t.numel() == 0:
            return t
        words32 = t.dtype in (torch.float32, torch.int32)
        if not (words32 or t.dtype == torch.float64):
            raise TypeError(f"poison harness: no fill pattern for a {t.dtype} buffer")
        with torch.no_grad():
            if self.mode == "nan":
                if words32:
                    t.view(torch.int32).fill_(NAN_WORD)
                else:
                    t.fill_(float("nan"))
            elif self.mode == "noise":
                if t.dtype == torch.int32:
                    t.view(torch.float32).copy_(self._randn(t, torch.float32))
                else:
                    t.copy_(self._randn(t, t.dtype))
            else:
                assert self.count < len(self._stale), "the call under test allocates more buffers than its first run did"
                src = self._stale[self.count]
                assert src.shape == t.shape and src.dtype == t.dtype and src.device == t.device, (self.count, src.shape, t.shape)
                t.copy_(src)
        self.count += 1
        if self._record:
            self.buffers.append(t)
        return t


@contextlib.contextmanager
def poisoned(monkeypatch, mode, stale=None, record=False):
    h = PoisonTorch(mode, stale=stale, record=record)
    with monkeypatch.context() as mp:
        mp.setattr(ops, "torch", h)
        yield h


def _words(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.int32)


def test_poison_harness_stand_in(monkeypatch):
    """The harness itself (no GPU): shape / dtype / device of what it returns, no sentinel word under any mode, pass-through of
    everything else, and the stand-in is gone after the context."""
    like = torch.ones(3, 5, dtype=torch.float32)
    first = None
    for mode in MODES:
        stale = None
        if mode == "stale":
            with poisoned(monkeypatch, "noise", record=True) as rec:
                for dt, shape in ((torch.float32, (4, 7)), (torch.float64, ()), (torch.int32, (9,)), (torch.float64, (2, 3))):
                    ops.torch.empty(shape, dtype=dt).add_(1)  # "what the buffer ended as"
                ops.torch.empty_like(like).mul_(2)
            stale, first = rec.buffers, [b.clone() for b in rec.buffers]
            assert len(stale) == 5
        with poisoned(monkeypatch, mode, stale=stale) as h:
            assert ops.torch is h
            got = [ops.torch.empty(4, 7, dtype=torch.float32), ops.torch.empty((), dtype=torch.float64, device="cpu"),
                   ops.torch.empty((9,), dtype=torch.int32), ops.torch.empty(2, 3, dtype=torch.float64), ops.torch.empty_like(like)]
            assert h.count == 5
            assert ops.torch.empty(0, 4).numel() == 0 and h.count == 5  # (nothing to poison in an empty buffer)
            # everything else passes through untouched
            assert ops.torch.zeros is torch.zeros and ops.torch.full is torch.full and ops.torch.float32 is torch.float32
            assert ops.torch.Tensor is torch.Tensor and ops.torch.autograd is torch.autograd and ops.torch.no_grad is torch.no_grad
            assert torch.equal(ops.torch.zeros(3), torch.zeros(3)) and torch.equal(ops.torch.full((2,), 4.0), torch.full((2,), 4.0))
        for t, (dt, shape) in zip(got, ((torch.float32, (4, 7)), (torch.float64, ()), (torch.int32, (9,)), (torch.float64, (2, 3)),
                                        (torch.float32, (3, 5)))):
            assert t.dtype == dt and tuple(t.shape) == shape and t.device.type == "cpu"
            assert not bool((_words(t) == SENTINEL_WORD).any()), mode
        if mode == "nan":
            assert all(bool((_words(t) == NAN_WORD).all()) for t in (got[0], got[2], got[4]))
            assert bool(torch.isnan(got[1])) and bool(torch.isnan(got[3]).all())
            assert _words(got[3].reshape(-1)[:1]).tolist() == [0, 0x7FF80000]  # the float64 quiet NaN
        elif mode == "noise":
            assert all(bool(torch.isfinite(t).all()) for t in (got[0], got[1], got[3], got[4]))
            assert bool(torch.isfinite(got[2].view(torch.float32)).all()) and float(got[0].std()) > 0.3
        else:
            assert all(torch.equal(_words(a), _words(b)) for a, b in zip(got, first))  # bit-copies, in allocation order
    assert ops.torch is torch
    with pytest.raises(AssertionError):  # one buffer more than the first run allocated
        with poisoned(monkeypatch, "stale", stale=[]):
            ops.torch.empty(3)
    assert ops.torch is torch


# ----------------------------------------------------------------------------------------------------------------------
# running a case under the three modes
# ----------------------------------------------------------------------------------------------------------------------


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    lib = _hip.load()
    assert lib.blvm_device_ok() == 1, "libblvm_hip: no gfx950 device visible"
    return lib


def _finish():
    torch.cuda.synchronize()
    _hip.check_async()  # (c): no persistent launch gave up on a bounded spin


def run_modes(monkeypatch, call, modes=MODES):
    """`call(variant)` -> (exact, loose): two dicts of result tensors; variant 0 is the call under test (it asserts bound (a)
    itself), variant 1 the same call on other inputs of the same shapes (the first run of `stale`).  Asserts (b) on `exact`, (c)
    on both, and that buffers were poisoned.  Returns {mode: (exact, loose)}."""
    res = {}
    for mode in modes:
        stale = None
        if mode == "stale":
            with poisoned(monkeypatch, "noise", record=True) as rec:
                call(1)
                _finish()
            stale = rec.buffers
        with poisoned(monkeypatch, mode, stale=stale) as h:
            exact, loose = call(0)
            _finish()
        assert h.count > 0, "no buffer went through blvm.ops' torch.empty / empty_like: the harness poisons nothing"
        assert stale is None or h.count == len(stale), (h.count, len(stale))
        for k, v in {**exact, **loose}.items():
            assert bool(torch.isfinite(v).all()), f"{mode}: non-finite values in {k}"
        res[mode] = ({k: v.detach() for k, v in exact.items()}, {k: v.detach() for k, v in loose.items()})
    first = res[modes[0]][0]
    for mode in modes[1:]:
        assert res[mode][0].keys() == first.keys()
        bad = [k for k in first if not torch.equal(res[mode][0][k], first[k])]
        assert not bad, f"results depend on what the buffers held: {bad} differ between {modes[0]} and {mode}"
    return res


@contextlib.contextmanager
def capturing(monkeypatch, *names):
    """Record what the named `ops` functions return (the models call them as `ops.<name>`): -> list of (name, outputs)."""
    seen = []
    with monkeypatch.context() as mp:
        for name in names:
            real = getattr(ops, name)

            def wrapped(*a, _real=real, _name=name, **k):
                out = _real(*a, **k)
                seen.append((_name, out if isinstance(out, tuple) else (out,)))
                return out

            mp.setattr(ops, name, wrapped)
        yield seen


def _split_captured(seen):
    """fp32 outputs of the sequence kernels -> exact; their float64 per-utterance sums (atomic adds) -> loose."""
    exact, loose = {}, {}
    for i, (name, outs) in enumerate(seen):
        for j, t in enumerate(outs):
            (exact if t.dtype == torch.float32 else loose)[f"{name}#{i}.{j}"] = t
    return exact, loose


@contextlib.contextmanager
def chain_path(one_launch):
    """The execution switch of K1-K5: one persistent launch per sequence | one launch per link; restored afterwards."""
    lib = _lib()
    before = lib.blvm_pchain_max_batch()
    lib.blvm_pchain_configure(128 if one_launch else 0, 0)
    try:
        yield
    finally:
        lib.blvm_pchain_configure(before, 0)


@contextlib.contextmanager
def operand_dtype(code):
    lib = _lib()
    before = lib.blvm_get_operand_dtype()
    lib.blvm_set_operand_dtype(code)
    try:
        yield
    finally:
        lib.blvm_set_operand_dtype(before)


def _ragged(B, T_):
    """Lengths T_ .. ~T_/2, the first row full."""
    return torch.tensor([T_ - (k * T_) // (2 * B) for k in range(B)], dtype=torch.int64)


# ----------------------------------------------------------------------------------------------------------------------
# VRNN / SRNN whole-model steps against the CPU oracle
# ----------------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _oracle_case(model, S, Hd, Z, B, Tp, cut, seed, beta, fn, with_h0, want_ref=True):
    """A model on the device, its inputs (variant 0 | 1) and the oracle's loss, ELBO and gradients for variant 0 (computed once)."""
    from blvm.models import SRNNAudio, VRNNAudio

    torch.manual_seed(seed)
    m = (VRNNAudio if model == "vrnn" else SRNNAudio)(likelihood="DMoL", input_size=S, hidden_size=Hd, latent_size=Z, residual_posterior=True)
    sd = {k: v.clone().requires_grad_(True) for k, v in m.state_dict().items()}
    T_ = S * Tp - cut
    x_sl = _ragged(B, T_)
    mask = torch.arange(T_).unsqueeze(0) < x_sl.unsqueeze(1)
    inputs = []
    for variant in (0, 1):
        x, _ = O.synth_batch(B, T_, seed=seed + 1 + variant)
        g = torch.Generator().manual_seed(seed + 10 + variant)
        eps = torch.randn(Tp, B, Z, generator=g)
        h0 = torch.randn(B, 2 * Hd, generator=g) * 0.3 if with_h0 else None
        inputs.append((x * mask, x_sl, eps, h0))
    ref = None
    if want_ref:
        x, x_sl, eps, h0 = inputs[0]
        fwd = O.vrnn_audio_forward if model == "vrnn" else O.srnn_audio_forward
        r = fwd(sd, x, x_sl, eps, beta=beta, free_nats=fn, stack=S, **(dict(h0=h0) if with_h0 else {}))
        r["loss"].backward()
        ref = (float(r["loss"].detach()), r["elbo"].detach(), {k: sd[k].grad for k in sd})
    m.to(DEV)
    inputs = [(x.to(DEV), x_sl, eps.to(DEV), h0.to(DEV) if h0 is not None else None) for x, x_sl, eps, h0 in inputs]
    return m, inputs, ref


def _model_step(monkeypatch, case, beta, fn, check_ref=True):
    """-> call(variant) for `run_modes`: one forward + backward of the model; bound (a) as `test_vrnn_vs_oracle_ragged_with_initial_state`
    / `test_large_batch_links_on_32x32_tiles_vs_oracle` state it."""
    m, inputs, ref = case

    def call(variant):
        x, x_sl, eps, h0 = inputs[variant]
        m.zero_grad(set_to_none=True)
        with capturing(monkeypatch, "vrnn_sequence", "srnn_latent_chain", "gru_sequence") as seen:
            loss, _, out = m(x, x_sl, beta=beta, free_nats=fn, eps=eps, **(dict(h0=h0) if h0 is not None else {}))
            loss.backward()
        exact, loose = _split_captured(seen)
        assert exact
        exact["z"] = out.z
        loose.update(loss=loss.detach(), elbo=out.elbo, kl=out.kl, log_prob=out.log_prob)
        grads = {k: p.grad for k, p in m.named_parameters()}
        loose.update({"grad." + k: v for k, v in grads.items()})
        if variant == 0 and check_ref and ref is not None:
            ref_loss, ref_elbo, ref_grads = ref
            assert float(loss.detach()) == pytest.approx(ref_loss, rel=1e-5)
            torch.testing.assert_close(out.elbo.cpu(), ref_elbo, rtol=1e-5, atol=1e-3)
            for k, v in grads.items():
                assert rel_l2(v, ref_grads[k]) < 1e-3, k
        return exact, loose

    return call


VRNN_INTERP = ("vrnn", 16, 48, 32, 19, 6, 5, 4, 0.7, 1.5, True)  # two row tiles, the last partial; T = 16*6 - 5; non-zero h0


@gpu
@pytest.mark.parametrize("one_launch", [True, False], ids=["one_launch", "launch_per_link"])
def test_vrnn_program_interpreter(one_launch, monkeypatch):
    """R = 96 is outside the static walk's shape: the program interpreter (or, with the switch at 0, one launch per link)."""
    lib = _lib()
    n0 = lib.blvm_pchain_static(-2)
    with chain_path(one_launch):
        run_modes(monkeypatch, _model_step(monkeypatch, _oracle_case(*VRNN_INTERP), 0.7, 1.5))
    assert lib.blvm_pchain_static(-2) == n0


@gpu
@pytest.mark.parametrize("B", [3, 50])
def test_vrnn_static_walk(B, monkeypatch):
    """H = Z = 256, R = 512, B <= 64: the static walk.  Bound (a) against the oracle at B = 3 (the full-width oracle is affordable
    there); at both B the static walk under `nan` equals the interpreter under `noise` bit for bit in what
    `test_gpu_vrnn_static.py` documents as identical (loss, ELBO, KL, z, h_n) and in every fp32 tensor of the forward kernels."""
    lib = _lib()
    case = _oracle_case("vrnn", 64, 256, 256, B, 4, 7, 5, 1.0, 2.0, False, B == 3)
    call = _model_step(monkeypatch, case, 1.0, 2.0)
    launches = []

    def counted(variant):
        n0 = lib.blvm_pchain_static(-2)
        out = call(variant)
        launches.append(lib.blvm_pchain_static(-2) - n0)
        return out

    was = lib.blvm_pchain_static(1)
    try:
        with chain_path(True):
            static = run_modes(monkeypatch, counted)
            assert launches == [2] * 4, launches  # forward and backward of every run (three modes + the first run of `stale`)
            lib.blvm_pchain_static(0)
            launches.clear()
            interp = run_modes(monkeypatch, counted, modes=("noise",))
            assert launches == [0]
    finally:
        lib.blvm_pchain_static(was)
    (s_exact, s_loose), (i_exact, i_loose) = static["nan"], interp["noise"]
    bad = [k for k in s_exact if not torch.equal(s_exact[k], i_exact[k])]
    bad += [k for k in ("loss", "elbo", "kl") if not torch.equal(s_loose[k], i_loose[k])]
    assert not bad, f"static walk (nan-poisoned) and interpreter (noise-poisoned) differ in {bad}"


@gpu
def test_vrnn_row_groups(monkeypatch):
    """The narrow model of `test_vrnn_row_group_engine_vs_oracle` at B = 72: two groups of 32-row tiles plus half a row tile.  (The
    library has no counter or query for the row-group deal: that it ran follows from the dispatch condition 65 <= B <= 256 with the
    persistent path on, not from an assertion; only the static walk is ruled out by its counter.)"""
    n0 = _lib().blvm_pchain_static(-2)
    _lib()
    with chain_path(True):
        run_modes(monkeypatch, _model_step(monkeypatch, _oracle_case("vrnn", 8, 32, 16, 72, 4, 3, 4, 1.0, 2.0, False), 1.0, 2.0))
    assert _lib().blvm_pchain_static(-2) == n0


@gpu
@pytest.mark.parametrize("model", ["vrnn", "srnn"])
def test_large_batch_32x32_link_kernels(model, monkeypatch):
    """`test_large_batch_links_on_32x32_tiles_vs_oracle` at its own B = 150 with T' cut to 3.  (No counter or query tells which link
    kernel ran: the 32x32 tiles follow from the dispatch condition B >= 128, not from an assertion.)"""
    _lib()
    run_modes(monkeypatch, _model_step(monkeypatch, _oracle_case(model, 16, 64, 32, 150, 3, 3, 6, 0.9, 1.0, False), 0.9, 1.0))


@gpu
@pytest.mark.parametrize("code", [1, 2], ids=["bf16", "f16"])
def test_vrnn_interpreter_16bit_operands(code, monkeypatch):
    """(b) and (c) only: the precision budget of the 16-bit modes is `test_gpu_bf16.py`'s / `test_gpu_f16.py`'s business."""
    _lib()
    with operand_dtype(code), chain_path(True):
        run_modes(monkeypatch, _model_step(monkeypatch, _oracle_case(*VRNN_INTERP), 0.7, 1.5, check_ref=False))


@gpu
def test_vrnn_seq_fwd_c_abi_defines_every_word_of_decin(monkeypatch):
    """`blvm_vrnn_seq_fwd` called as a C caller would, every buffer — decin with its extra row T' included — NaN-poisoned: the
    outputs the header promises (decin rows [phi_t | h_{t-1}], row T' = [0 | h_n], mu / sd / z) equal those of the `ops` path bit
    for bit.  Nothing in the model consumes the phi-part of row T' (`blvm/models/vrnn.py` decodes `decin[:Tp]` and, in the single-step
    path, reads only the h-part of the next row), so as a conservative stand-in for a consumer the decoder MLP runs over ALL rows of
    decin, row T' included, and must stay finite."""
    lib = _lib()
    m, inputs, _ = _oracle_case(*VRNN_INTERP)
    cell = m.vrnn.vrnn_cell
    _, _, dec_lin, _ = m.vrnn._plan()
    Tp, B, X, H, Z, R = 6, 19, 48, 48, 32, 96
    g = torch.Generator().manual_seed(3)
    enc = torch.randn(Tp, B, X, generator=g).to(DEV)
    eps, h0 = inputs[0][2], inputs[0][3]
    sd_eps = float(cell.prior[6].epsilon)
    params = [p.detach().contiguous() for p in cell.kernel_params()]
    x_sl_dev = torch.full((B,), Tp * 16, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        want = ops.vrnn_sequence(enc, h0, eps, x_sl_dev, params, X, H, Z, R, True, 16, 0.0, sd_eps)
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV, dtype=torch.float32)  # noqa: E731
    decin = nan(Tp + 1, B, H + R)
    mu_q, sd_q, mu_p, sd_p, z = (nan(Tp, B, Z) for _ in range(5))
    reserve = nan(lib.blvm_vrnn_reserve_floats(Tp, B, X, H, Z, R))
    p = _hip.ptr
    _hip.check(lib.blvm_vrnn_seq_fwd(ops._pack_weights(params), p(enc), p(h0), p(eps), Tp, B, X, H, Z, R, 1, sd_eps, p(decin), p(mu_q),
                                     p(sd_q), p(mu_p), p(sd_p), p(z), p(reserve), _hip.stream_ptr()), "blvm_vrnn_seq_fwd")  # fmt: skip
    _finish()
    assert bool(torch.isfinite(decin).all()), "decin keeps words of the caller's buffer"
    assert bool((decin[Tp, :, :H] == 0).all())  # the phi-part of the extra row: zeros (include/blvm_hip.h)
    assert torch.equal(decin[0, :, H:], h0) and rel_l2(decin[Tp, :, H:], want[0][Tp, :, H:]) == 0.0
    for name, a, b in zip(("decin", "mu_q", "sd_q", "mu_p", "sd_p", "z"), (decin, mu_q, sd_q, mu_p, sd_p, z), (want[0], *want[3:])):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), name
    with torch.no_grad():
        dec = ops.mlp(decin.view((Tp + 1) * B, H + R), dec_lin)
    _finish()
    assert bool(torch.isfinite(dec).all())


@gpu
@pytest.mark.parametrize("S,layout", [(5, 0), (64, 1), (128, 1)], ids=["frame_kernel", "rows_kernel", "rows_kernel_two_units_per_row"])
def test_dmol_ll_twise_is_a_caller_zeroed_output(S, layout):
    """ll_twise is the one output found that the header had to mark "caller zeroes": the kernels (S = 5: one lane per frame; S = 64
    and 128: the 64-frame row units, one and two per row) write it at the frames t < x_sl[b] only, which `test_gpu_heads.py` pins.  What holds, then: `ops` hands
    the kernel zeros, so the masked frames of what it returns are zeros; the written frames do not depend on what the buffer held
    (a NaN-filled buffer through the C ABI gives the same bits); the per-utterance sums meet the bound of
    `test_dmol_forward_backward_vs_oracle` against the float64 oracle."""
    lib = _lib()
    B, Tp = 3, 7
    T_ = Tp * S - (S // 2)
    x_sl = _ragged(B, T_)
    g = torch.Generator().manual_seed(11 + S)
    W, b = torch.randn(30, 30, generator=g) * 0.3, torch.randn(30, generator=g) * 0.1
    x, dec_bm = O.synth_batch(B, T_, seed=S)[0], torch.randn(B, Tp * S, 30, generator=g) * 1.5

    def oracle(dt):
        lgt, lc, ls = O.dmol_head(dec_bm[:, :T_].to(dt), W.to(dt), b.to(dt))
        ll = O.dmol_ll(x.to(dt).unsqueeze(-1), lgt, lc, ls, 2**16)
        return (ll * O.sequence_mask(x_sl, T_, torch.float64)).sum(1)

    ref32, truth = oracle(torch.float32), oracle(torch.float64)
    dec = dec_bm.view(B * Tp, S * 30) if layout == 0 else dec_bm.view(B, Tp, S * 30).transpose(0, 1).contiguous().view(Tp * B, S * 30)
    dec, Wd, bd, y, lens = dec.to(DEV), W.to(DEV), b.to(DEV), x.to(DEV), x_sl.to(DEV, torch.int32)
    written = torch.arange(T_, device=DEV).unsqueeze(0) < lens.unsqueeze(1)
    want, want_lp = ops.dmol_ll_twise(dec, Wd, bd, y, lens, layout, B, T_, Tp, S, 10, 2**16, -7.0)
    assert bool((~written).any()) and bool((want[~written] == 0).all()) and bool(torch.isfinite(want).all())
    assert rel_l2(want_lp, want.double().sum(1)) < 1e-9
    assert rel_l2(want_lp, truth) <= max(4 * rel_l2(ref32, truth), 1e-5), (rel_l2(want_lp, truth), rel_l2(ref32, truth))
    ll = torch.full((B, T_), float("nan"), device=DEV)
    lp = torch.zeros(B, device=DEV, dtype=torch.float64)
    p = _hip.ptr
    _hip.check(lib.blvm_dmol_fwd(p(dec), layout, p(Wd), p(bd), p(y), p(lens), B, T_, Tp, S, 10, 2**16, -7.0, p(lp), p(ll), _hip.stream_ptr()),
               "blvm_dmol_fwd")  # fmt: skip
    _finish()
    assert torch.equal(ll[written], want[written])
    torch.testing.assert_close(lp, want_lp, rtol=1e-12, atol=0)  # (float64 atomic adds: the order is free)


# ----------------------------------------------------------------------------------------------------------------------
# SRNN latent chain and RSSM cell sequence against the reference's goldens
# ----------------------------------------------------------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("one_launch", [True, False], ids=["one_launch", "launch_per_link"])
@pytest.mark.parametrize("tag,smoothing,beta,fn_", [("sm", True, 1.0, 2.0), ("ns", False, 0.5, 0.0)])
def test_srnn_latent_chain(tag, smoothing, beta, fn_, one_launch, monkeypatch):
    """The configurations and bounds of `test_srnn_small_vs_reference_golden` (smoothing on: the reversed GRU and its backward)."""
    from blvm.models import SRNNAudio

    _lib()
    T = lambda a: torch.from_numpy(np.asarray(a))  # noqa: E731
    g = np.load(os.path.join(GOLDEN, "srnn.npz"))
    m = SRNNAudio(likelihood="DMoL", input_size=8, hidden_size=32, latent_size=16, residual_posterior=True, smoothing=smoothing)
    pre = f"{tag}_sd."
    m.load_state_dict({k[len(pre):]: T(g[k]) for k in g.files if k.startswith(pre)})
    m.to(DEV)
    x, x_sl, eps = T(g["x"]), T(g["x_sl"]), T(g[f"{tag}_eps"])
    assert x.shape[0] % 16 != 0
    inputs = [(x.to(DEV), eps.to(DEV)), ((-x).to(DEV), eps.flip(0).contiguous().to(DEV))]

    def call(variant):
        xd, ed = inputs[variant]
        m.zero_grad(set_to_none=True)
        with capturing(monkeypatch, "srnn_latent_chain", "gru_sequence") as seen:
            loss, _, out = m(xd, x_sl, beta=beta, free_nats=fn_, eps=ed)
            loss.backward()
        exact, loose = _split_captured(seen)
        assert len(seen) == (3 if smoothing else 2)
        exact.update(z=out.z, d_n=out.d_n, z_n=out.z_n, **(dict(a_n=out.a_n) if smoothing else {}))
        loose.update(loss=loss.detach(), elbo=out.elbo, kl=out.kl, log_prob=out.log_prob)
        loose.update({"grad." + k: p.grad for k, p in m.named_parameters()})
        if variant == 0:
            assert float(loss.detach()) == pytest.approx(float(g[f"{tag}_loss"]), rel=1e-5)
            torch.testing.assert_close(out.elbo.cpu(), T(g[f"{tag}_elbo"]), rtol=1e-5, atol=1e-3)
            torch.testing.assert_close(out.log_prob.cpu(), T(g[f"{tag}_log_prob"]), rtol=1e-5, atol=1e-3)
            torch.testing.assert_close(out.kl.cpu(), T(g[f"{tag}_kl"]), rtol=1e-5, atol=1e-4)
            torch.testing.assert_close(out.z.cpu(), T(g[f"{tag}_z"]), rtol=1e-4, atol=1e-5)
            torch.testing.assert_close(out.d_n.cpu(), T(g[f"{tag}_d_n"]), rtol=1e-4, atol=1e-5)
            torch.testing.assert_close(out.z_n.cpu(), T(g[f"{tag}_z_n"]), rtol=1e-4, atol=1e-5)
            if smoothing:
                torch.testing.assert_close(out.a_n.cpu(), T(g[f"{tag}_a_n"]), rtol=1e-4, atol=1e-5)
            for k, p in m.named_parameters():
                assert rel_l2(p.grad, T(g[f"{tag}_grad.{k}"])) < 1e-3, k
        return exact, loose

    with chain_path(one_launch):
        run_modes(monkeypatch, call)


@gpu
@pytest.mark.parametrize("tag,other", [("plain", "res"), ("res", "prec"), ("prec", "plain")])
def test_rssm_cell_sequence(tag, other, monkeypatch):
    """`test_rssm_sequence_vs_reference_golden` itself (its reference, its bounds) under the harness; the first run of `stale` is
    another of its golden cases: the same shapes, other weights and noise."""
    import test_gpu_parity as P

    _lib()
    kws = {"plain": {}, "res": dict(residual_posterior=True), "prec": dict(precision_posterior=True)}

    def call(variant):
        with capturing(monkeypatch, "rssm_sequence") as seen:
            which = tag if variant == 0 else other
            P.test_rssm_sequence_vs_reference_golden(which, kws[which], 48)
        assert len(seen) == 1
        return _split_captured(seen)

    run_modes(monkeypatch, call)


# ----------------------------------------------------------------------------------------------------------------------
# the bare GRU / LSTM sequence kernels against float64 torch
# ----------------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _gru_case(T_, B, I, R, reverse):
    torch.manual_seed(7)
    gru = torch.nn.GRU(I, R)
    lens = torch.tensor([max(1, T_ - (k * T_) // B) for k in range(B)])
    g = torch.Generator().manual_seed(T_ + B + R)
    inputs = [(torch.randn(T_, B, I, generator=g), torch.randn(B, R, generator=g) * 0.5, torch.randn(T_, B, R, generator=g)) for _ in (0, 1)]
    x, h0, w = inputs[0]
    ref_gru = copy.deepcopy(gru).double()
    xr, h0r = x.double().requires_grad_(True), h0.double().requires_grad_(True)
    if reverse:
        out, hn = ref_gru(O.reverse_sequences(xr, lens), h0r.unsqueeze(0))
        out = O.reverse_sequences(out, lens)
    else:
        out, hn = ref_gru(xr, h0r.unsqueeze(0))
    (out * w.double()).sum().backward()
    ref = (out.detach(), hn[0].detach(), [xr.grad, h0r.grad] + [p.grad for p in ref_gru.parameters()])
    return gru.to(DEV), lens.to(DEV, torch.int32), [tuple(t.to(DEV) for t in inp) for inp in inputs], ref


def _gru_call(case, reverse, check_ref=True):
    gru, lens, inputs, (ref_out, ref_hn, ref_grads) = case

    def call(variant):
        x, h0, w = inputs[variant]
        gru.zero_grad(set_to_none=True)
        xd, h0d = x.clone().requires_grad_(True), h0.clone().requires_grad_(True)
        od, hnd = ops.gru_sequence(xd, h0d, gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0, lens, reverse)
        (od * w).sum().backward()
        got = [xd.grad, h0d.grad] + [p.grad for p in gru.parameters()]
        if variant == 0 and check_ref:
            assert rel_l2(od, ref_out) < 1e-5 and rel_l2(hnd, ref_hn) < 1e-5
            for i, (a, b) in enumerate(zip(got, ref_grads)):
                assert rel_l2(a, b) < 2e-5, i
        return dict(out=od, hn=hnd), {f"grad{i}": t for i, t in enumerate(got)}

    return call


@gpu
@pytest.mark.parametrize("one_launch", [True, False], ids=["one_launch", "launch_per_step"])
@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reversed"])
@pytest.mark.parametrize("T_,B,I,R", [(5, 5, 24, 32), (5, 35, 48, 128), (4, 20, 16, 512)])
def test_gru_sequence_kernels(T_, B, I, R, reverse, one_launch, monkeypatch):
    """R = 32: a program of the persistent-chain engine; R = 128, 512: the register-resident kernels of seqchain.hip (R = 512: the
    backward reads its operand once per XCD).  Ragged `lens`, non-zero h0, against nn.GRU in float64."""
    _lib()
    with chain_path(one_launch):
        run_modes(monkeypatch, _gru_call(_gru_case(T_, B, I, R, reverse), reverse))


@gpu
@pytest.mark.parametrize("code", [1, 2], ids=["bf16", "f16"])
def test_gru_sequence_16bit_operands(code, monkeypatch):
    """(b) and (c) only."""
    _lib()
    with operand_dtype(code), chain_path(True):
        run_modes(monkeypatch, _gru_call(_gru_case(5, 35, 48, 128, True), True, check_ref=False))


@functools.lru_cache(maxsize=None)
def _lstm_case(T_, B, I, H):
    torch.manual_seed(8)
    lstm = torch.nn.LSTM(I, H, batch_first=True)
    lens = torch.tensor([5, 5, 4, 3, 2, 1]) if B == 6 else torch.tensor([max(1, T_ - (k * T_) // B) for k in range(B)])
    assert int(lens.max()) == T_ and int(lens.min()) < T_
    g = torch.Generator().manual_seed(T_ + B + H)
    inputs = [(torch.randn(B, T_, I, generator=g), torch.randn(B, T_, H, generator=g)) for _ in (0, 1)]
    x, w = inputs[0]
    ref_lstm = copy.deepcopy(lstm).double()
    xr = x.double().requires_grad_(True)
    out, (hn, cn) = ref_lstm(torch.nn.utils.rnn.pack_padded_sequence(xr, lens, batch_first=True))
    out, _ = torch.nn.utils.rnn.pad_packed_sequence(out, batch_first=True)
    (out * w.double()).sum().backward()
    ref = (out.detach(), hn[0].detach(), cn[0].detach(), [xr.grad] + [p.grad for p in ref_lstm.parameters()])
    past = (torch.arange(T_).unsqueeze(1) >= lens.unsqueeze(0)).to(DEV)  # [T,B]: steps past a row's length
    inputs = [(x.transpose(0, 1).contiguous().to(DEV), w.transpose(0, 1).contiguous().to(DEV)) for x, w in inputs]
    return lstm.to(DEV), lens.to(DEV, torch.int32), past, inputs, ref


def _lstm_call(case):
    lstm, lens, past, inputs, (ref_out, ref_hn, ref_cn, ref_grads) = case

    def call(variant):
        x, w = inputs[variant]
        lstm.zero_grad(set_to_none=True)
        xd = x.clone().requires_grad_(True)
        od, hnd, cnd = ops.lstm_sequence(xd, None, None, lens, lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0)
        (od * w).sum().backward()
        got = [xd.grad.transpose(0, 1)] + [p.grad for p in lstm.parameters()]
        assert bool(past.any()) and bool((od[past] == 0).all()), "out past a row's length must be zeros"
        if variant == 0:
            assert rel_l2(od.transpose(0, 1), ref_out) < 1e-5 and rel_l2(hnd, ref_hn) < 1e-5 and rel_l2(cnd, ref_cn) < 1e-5
            for i, (a, b) in enumerate(zip(got, ref_grads)):
                assert rel_l2(a, b) < 2e-5, i
        return dict(out=od, hn=hnd, cn=cnd), {f"grad{i}": t for i, t in enumerate(got)}

    return call


@gpu
@pytest.mark.parametrize("one_launch", [True, False], ids=["one_launch", "launch_per_step"])
@pytest.mark.parametrize("T_,B,I,H", [(5, 6, 16, 32), (6, 37, 64, 128)])
def test_lstm_sequence_kernels(T_, B, I, H, one_launch, monkeypatch):
    """Packed-sequence semantics against nn.LSTM in float64; `out` past a row's length is exact zeros under every mode (the
    reference writes zeros there: a missing write shows as the poison)."""
    _lib()
    with chain_path(one_launch):
        run_modes(monkeypatch, _lstm_call(_lstm_case(T_, B, I, H)))


# ----------------------------------------------------------------------------------------------------------------------
# one-launch decoders: fixed eps / u / v draws, samples bit-identical across the modes
# ----------------------------------------------------------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("whole_chip", [False, True], ids=["16_per_cu", "whole_chip"])
def test_vrnn_one_launch_decoders(whole_chip, monkeypatch):
    """K1c, both forms, as `test_vrnn_one_launch_decoder_matches_stepwise_generation` sets them, against step-by-step generation."""
    from blvm.models import VRNNAudio

    _lib()
    B, S, Hd, Z, T_ = 5, 16, 64, 32, 4
    torch.manual_seed(B + S)
    m = VRNNAudio(likelihood="DMoL", input_size=S, hidden_size=Hd, latent_size=Z, residual_posterior=True).to(DEV)
    real = ops.vrnn_decode
    decoded = []  # what `ops.vrnn_decode` returned: (x [B,T,S], h_n [B,R])

    def decode(*a, **k):
        decoded.append(real(*a, whole_chip=whole_chip, **k))
        return decoded[-1]

    monkeypatch.setattr(ops, "vrnn_decode", decode)
    g = torch.Generator().manual_seed(3)
    draws = []
    for _ in (0, 1):
        eps = torch.randn(T_, B, Z, generator=g).to(DEV)
        u = torch.empty(T_, B, S, 10).uniform_(1e-5, 1 - 1e-5, generator=g).to(DEV)
        v = torch.empty(T_, B, S).uniform_(1e-8, 1 - 1e-8, generator=g).to(DEV)
        draws.append((eps, (u, v), (torch.rand(B, S, 1, generator=g) * 0.2 - 0.1).to(DEV)))
    eps, uv, x0 = draws[0]
    (a, a_sl), _ = m.generate(n_samples=B, max_timesteps=T_, x=x0, eps=eps, uniforms=uv, fused=False)

    def call(variant):
        eps, uv, x0 = draws[variant]
        decoded.clear()
        (b, b_sl), _ = m.generate(n_samples=B, max_timesteps=T_, x=x0, eps=eps, uniforms=uv, fused=True)
        assert len(decoded) == 1 and tuple(decoded[0][1].shape) == (B, 2 * Hd)
        if variant == 0:
            assert tuple(a.shape) == tuple(b.shape) == (B, T_ + 1, S) and torch.equal(a_sl, b_sl)
            assert float(((a - b).abs() > 2e-4).float().mean()) < 0.02, (a - b).abs().max()
        return dict(x=b, hn=decoded[0][1]), {}

    run_modes(monkeypatch, call)


@gpu
def test_srnn_one_launch_decoder(monkeypatch):
    """K3c at B = 3 and the C3 widths, against the step-by-step path with the bounds of
    `test_srnn_one_launch_decoder_matches_stepwise_at_full_width`."""
    from blvm.models import SRNNAudio

    _lib()
    B, T_ = 3, 4
    torch.manual_seed(B)
    m = SRNNAudio(likelihood="DMoL", input_size=64, hidden_size=256, latent_size=256, residual_posterior=True, smoothing=True).to(DEV)
    g = torch.Generator().manual_seed(3)
    draws = []
    for _ in (0, 1):
        eps = torch.randn(T_, B, 256, generator=g).to(DEV)
        uni = [(torch.empty(B, 64, 10).uniform_(1e-5, 1 - 1e-5, generator=g).to(DEV), torch.empty(B, 64, 1).uniform_(1e-8, 1 - 1e-8, generator=g).to(DEV))
               for _ in range(T_)]
        draws.append((eps, uni, (torch.rand(B, 1, 64, generator=g) * 0.2 - 0.1).to(DEV)))
    eps, uni, x0 = draws[0]
    (a, _), oa = m.srnn.generate(x=x0, n_samples=B, max_timesteps=T_, eps=eps, uniforms=uni, fused=False)

    def call(variant):
        eps, uni, x0 = draws[variant]
        with capturing(monkeypatch, "srnn_generate") as seen:
            (b, _), ob = m.srnn.generate(x=x0, n_samples=B, max_timesteps=T_, eps=eps, uniforms=uni, fused=True)
        assert len(seen) == 1
        if variant == 0:
            assert tuple(a.shape) == tuple(b.shape) == (B, T_, 64, 1)
            assert float(((a - b).abs() > 2e-4).float().mean()) < 0.02, (a - b).abs().max()
            assert float(((oa.h_p - ob.h_p).abs() > 1e-3).float().mean()) < 0.02
        exact, _ = _split_captured(seen)  # x, d_T, zs
        exact.update(x=b, h_p=ob.h_p)
        return exact, {}

    run_modes(monkeypatch, call)


@gpu
def test_wavenet_one_launch_decoder(monkeypatch):
    """`blvm_wavenet_decode` over a partial 16-utterance group against the per-frame window path
    (`test_wavenet_decode_kernel_matches_window_generation`)."""
    from blvm.models import WaveNet
    from blvm.modules.distributions import DiscretizedLogisticMixtureDense

    _lib()
    B, C, layers, stacks, n = 19, 32, 5, 2, 8
    torch.manual_seed(B + C)
    m = WaveNet(likelihood=DiscretizedLogisticMixtureDense(C, 1, num_mix=10, num_bins=2**16), n_layers=layers, n_stacks=stacks, res_channels=C).to(DEV)
    gen = torch.Generator().manual_seed(B)
    draws = [[(torch.empty(B, 1, 10).uniform_(1e-5, 1 - 1e-5, generator=gen).to(DEV), torch.empty(B, 1).uniform_(1e-8, 1 - 1e-8, generator=gen).to(DEV))
              for _ in range(n)] for _ in (0, 1)]
    assert m._decode_kernel_applies()
    a = m.generate(n_samples=B, n_frames=n, uniforms=draws[0])

    def call(variant):
        with capturing(monkeypatch, "wavenet_decode") as seen:
            b = m.generate(n_samples=B, n_frames=n, uniforms=draws[variant], cached=True)
        assert len(seen) == 1
        if variant == 0:
            assert tuple(b.shape) == (B, n, 1)
            assert float(((a - b).abs() > 1e-4).float().mean()) < 0.05, (a - b).abs().max()
        return dict(x=b), {}

    run_modes(monkeypatch, call)


# ----------------------------------------------------------------------------------------------------------------------
# WaveNet training kernels and the conv coders against float64 torch
# ----------------------------------------------------------------------------------------------------------------------


@gpu
def test_wavenet_stack_kernels(monkeypatch):
    """`wavenet_stack` forward + backward against the float64 restatement and bounds of
    `test_wavenet_fused_block_kernels_match_torch`.  (Its skip outputs are ACCUMULATED sums over the blocks: bound (a).)"""
    _lib()
    C, B, L, dil, T_skip = 32, 3, 77, (1, 2, 4), 50

    def ref(x, params):
        h, skip = x.permute(1, 2, 0), 0.0  # [B,C,L]
        for i, d in enumerate(dil):
            cw, cb, rw, rb = params[4 * i : 4 * i + 4]
            pre = torch.nn.functional.conv1d(h, cw, cb, dilation=d)
            act = torch.tanh(pre[:, :C]) * torch.sigmoid(pre[:, C:])
            rs = torch.nn.functional.conv1d(act, rw.unsqueeze(-1), rb)
            skip = skip + rs[:, C:, -T_skip:]
            h = (rs[:, :C] + h[:, :, d:]) * math.sqrt(0.5)
        return skip.permute(2, 0, 1)

    g = torch.Generator().manual_seed(C + L)
    params = []
    for _ in dil:
        params += [torch.randn(2 * C, C, 2, generator=g) * 0.08, torch.randn(2 * C, generator=g) * 0.1,
                   torch.randn(2 * C, C, generator=g) * 0.08, torch.randn(2 * C, generator=g) * 0.1]
    inputs = [(torch.randn(L, B, C, generator=g), torch.randn(T_skip, B, C, generator=g)) for _ in (0, 1)]
    x, gs = inputs[0]
    xr, pr = x.double().requires_grad_(True), [p.double().requires_grad_(True) for p in params]
    want = ref(xr, pr)
    (want * gs.double()).sum().backward()

    def call(variant):
        x, gs = inputs[variant]
        xd = x.to(DEV).requires_grad_(True)
        pd = [p.to(DEV).requires_grad_(True) for p in params]
        out = ops.wavenet_stack(xd, [tuple(pd[4 * i : 4 * i + 4]) for i in range(len(dil))], list(dil), T_skip, math.sqrt(0.5), C)
        (out * gs.to(DEV)).sum().backward()
        if variant == 0:
            assert rel_l2(out, want) < 2e-6
            assert rel_l2(xd.grad, xr.grad) < 5e-6
            last = len(dil) - 1
            for i, (a, b) in enumerate(zip(pd, pr)):
                if i // 4 == last and i % 4 >= 2:  # the last block's residual rows of the 1x1 conv never reach an output
                    assert rel_l2(a.grad[C:], b.grad[C:]) < 2e-5, i
                else:
                    assert rel_l2(a.grad, b.grad) < 2e-5, i
        return dict(out=out), dict(dx=xd.grad, **{f"grad{i}": p.grad for i, p in enumerate(pd)})

    run_modes(monkeypatch, call)


@gpu
@pytest.mark.parametrize("dilation", [1, 2, 4])
def test_conv1d_k2_kernels(dilation, monkeypatch):
    """`conv1d_k2` (the WaveNet's dilated causal convolution, kernel size 2) forward + backward against F.conv1d in float64, with
    the WaveNet kernels' bounds of `test_wavenet_fused_block_kernels_match_torch`; the forward has no atomics: bit-identical."""
    _lib()
    C, B, L = 32, 3, 77
    g = torch.Generator().manual_seed(C + L + dilation)
    W, bias = torch.randn(2 * C, C, 2, generator=g) * 0.08, torch.randn(2 * C, generator=g) * 0.1
    inputs = [(torch.randn(L, B, C, generator=g), torch.randn(L - dilation, B, 2 * C, generator=g)) for _ in (0, 1)]
    x, gy = inputs[0]
    xr, Wr, br = (t.double().requires_grad_(True) for t in (x, W, bias))
    want = torch.nn.functional.conv1d(xr.permute(1, 2, 0), Wr, br, dilation=dilation).permute(2, 0, 1)
    (want * gy.double()).sum().backward()

    def call(variant):
        x, gy = inputs[variant]
        xd, Wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, W, bias))
        out = ops.conv1d_k2(xd, Wd, bd, dilation)
        (out * gy.to(DEV)).sum().backward()
        if variant == 0:
            assert rel_l2(out, want) < 2e-6
            assert rel_l2(xd.grad, xr.grad) < 5e-6
            assert rel_l2(Wd.grad, Wr.grad) < 2e-5 and rel_l2(bd.grad, br.grad) < 2e-5
        return dict(out=out), dict(dx=xd.grad, dW=Wd.grad, db=bd.grad)

    run_modes(monkeypatch, call)


@gpu
def test_chan_norm_kernels(monkeypatch):
    """`chan_norm` at (L, B, C) = (37, 3, 8) against nn.GroupNorm in float64 (`test_chan_norm_matches_groupnorm`, its bounds)."""
    from test_gpu_convcoder import TOL, bct, tm

    _lib()
    L, B, C = 37, 3, 8
    g = torch.Generator().manual_seed(L + B + C)
    gn = torch.nn.GroupNorm(C, C).double()
    with torch.no_grad():
        gn.weight.copy_(torch.randn(C, generator=g))
        gn.bias.copy_(torch.randn(C, generator=g))
    inputs = [((torch.randn(B, C, L, generator=g) * 3 + 1.5).double(), torch.randn(B, C, L, generator=g).double()) for _ in (0, 1)]
    x = inputs[0][0].clone().requires_grad_()
    y = gn(x)
    y.backward(inputs[0][1])

    def call(variant):
        xv, dy = inputs[variant]
        xd = tm(xv.float()).to(DEV).requires_grad_()
        w, b = gn.weight.detach().float().to(DEV).requires_grad_(), gn.bias.detach().float().to(DEV).requires_grad_()
        yd = ops.chan_norm(xd, w, b, gn.eps)
        yd.backward(tm(dy.float()).to(DEV))
        if variant == 0:
            assert rel_l2(bct(yd), y) < TOL
            assert rel_l2(bct(xd.grad), x.grad) < 5 * TOL
            assert rel_l2(w.grad, gn.weight.grad) < TOL and rel_l2(b.grad, gn.bias.grad) < TOL
        return dict(y=yd), dict(dx=xd.grad, dw=w.grad, db=b.grad)

    run_modes(monkeypatch, call)


@gpu
def test_separable_block_kernels(monkeypatch):
    """One `BlockSeparable` at (stride, C, B, L) = (2, 24, 3, 61) against the float64 torch modules
    (`test_separable_block_matches_torch`, its bounds): `ops.py` allocates mr, ss, a1, r and dn2 empty."""
    import torch.nn as nn
    from blvm.models.clockwork_vae.convolutional_coders import BlockSeparable
    from test_gpu_convcoder import TOL, _randomise_norms, _torch_block

    _lib()
    stride, C, B, L = 2, 24, 3, 61
    torch.manual_seed(stride)
    g = torch.Generator().manual_seed(1)
    block = BlockSeparable(C, 5, stride, 1, nn.ReLU, False, bias=True)
    _randomise_norms(block, g)
    ref = BlockSeparable(C, 5, stride, 1, nn.ReLU, False, bias=True).double()
    ref.load_state_dict(block.state_dict())
    xs = [torch.randn(B, C, L, generator=g) for _ in (0, 1)]
    xr = xs[0].double().requires_grad_()
    yr = _torch_block(ref, xr)
    dys = [torch.randn(yr.shape, generator=g) for _ in (0, 1)]
    yr.backward(dys[0].double())
    block = block.to(DEV)
    pr = dict(ref.named_parameters())

    def call(variant):
        block.zero_grad(set_to_none=True)
        xd = xs[variant].to(DEV).requires_grad_()
        yd = block(xd)  # reference layout entry point [B,C,T]
        yd.backward(dys[variant].to(DEV))
        if variant == 0:
            assert yd.shape == yr.shape
            assert rel_l2(yd, yr) < TOL
            assert rel_l2(xd.grad, xr.grad) < 5 * TOL
            for n, p in block.named_parameters():
                assert p.grad is not None, n
                assert rel_l2(p.grad, pr[n].grad) < 3e-4, n  # fp32 GEMM weight gradients over L*B rows vs float64
        return dict(y=yd), dict(dx=xd.grad, **{"grad." + n: p.grad for n, p in block.named_parameters()})

    run_modes(monkeypatch, call)
