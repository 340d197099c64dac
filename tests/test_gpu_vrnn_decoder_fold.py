"""GPU: the VRNN decoder MLP as a follower range of the static forward walk (csrc/vrnn_static.h, blvm_vrnn_seq_fwd_dec).

At B <= 64 the forward deal leaves workgroups free behind the hidden projection's range; they run the decoder of step t from the
slabs PHI16[t] and H16[t] while the chain goes on.  The folded layers sum K in the chain tile's order (per-wave chunks, reduced in
wave order; the first layer as its h-part plus its phi-part), not in K6's, so `dec`, `log_prob`, the loss and the gradients change
in their last bits against the unfolded path; `z`, `h_n` and the KL must not change at all.  The yardstick is the float64 oracle:
the folded path's error may be at most twice the unfolded path's on the same inputs.

T' = 3; S = 8 (15 column tiles of the last layer) and 64 (120: the 7.5-tiles-per-workgroup deal of the benchmark); B = 5 (a partial
row tile), 17 (two row tiles, one partial) and 64 (the benchmark's deal); ragged lengths."""
import contextlib
import functools

import pytest
import torch
import torch.nn as nn

import blvm_oracle as O
from blvm import _hip, ops
from blvm.models import VRNNAudio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TP, H = 3, 256
CASES = [(B, S) for S in (8, 64) for B in (5, 17, 64)]
NAN_WORD, SENTINEL_WORD = 0x7FC00000, -1
EXACT = ("z", "h_n", "kl")  # what the critical roles compute: never touched by the fold
DECODER = ("y1", "y2", "dec", "log_prob", "loss", "elbo")


def _lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    lib = _hip.load()
    assert lib.blvm_device_ok() == 1
    return lib


@contextlib.contextmanager
def switches(fold=True, static=True):
    lib = _lib()
    was = lib.blvm_vrnn_dec_fold(int(fold)), lib.blvm_pchain_static(1 if static else 0)  # (fold = 2: the first two layers only)
    try:
        yield lib
    finally:
        lib.blvm_vrnn_dec_fold(was[0])
        lib.blvm_pchain_static(was[1])


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@functools.lru_cache(maxsize=None)
def _case(B, S, width=H):
    """The model (on the device), its inputs, and the float64 oracle's results for them (computed once, never modified)."""
    torch.manual_seed(100 + B + S)
    m = VRNNAudio(likelihood="DMoL", input_size=S, hidden_size=H, latent_size=H, residual_posterior=True)
    if width != H:  # a decoder whose hidden width is not the cell's
        d = m.vrnn.decoder
        d[0], d[2], d[4] = nn.Linear(3 * H, width), nn.Linear(width, width), nn.Linear(width, d[4].out_features)
    T_ = S * TP - 3
    x_sl = torch.tensor([T_ - (k * T_) // (2 * B) for k in range(B)], dtype=torch.int64)  # ragged, the first row full
    x, _ = O.synth_batch(B, T_, seed=B + S)
    x = x * (torch.arange(T_).unsqueeze(0) < x_sl.unsqueeze(1))
    eps = torch.randn(TP, B, H, generator=torch.Generator().manual_seed(7 + B))
    ref = None
    if width == H:
        sd = {k: v.double().clone().requires_grad_(True) for k, v in m.state_dict().items()}
        xd, ed = x.double(), eps.double()
        r = O.vrnn_audio_forward(sd, xd, x_sl, ed, beta=1.0, free_nats=2.0, stack=S)
        r["loss"].backward()
        with torch.no_grad():  # the decoder's activations, from the oracle's own cell and MLP
            h, hs, phis = torch.zeros(B, 2 * H, dtype=torch.float64), [], []
            for t in range(TP):
                hs.append(h)
                h, o = O.vrnn_cell_step(sd, r["enc"][:, t], h, ed[t], True)
                phis.append(o["phi"])
            acts, a = [], torch.cat([torch.stack(phis, 0), torch.stack(hs, 0)], -1).reshape(TP * B, 3 * H)  # time-major rows
            for i in (0, 2, 4):
                a = torch.nn.functional.leaky_relu(torch.nn.functional.linear(a, sd[f"vrnn.decoder.{i}.weight"], sd[f"vrnn.decoder.{i}.bias"]))
                acts.append(a)
        ref = {"y1": acts[0], "y2": acts[1], "dec": acts[2], "log_prob": r["log_prob"].detach(), "loss": r["loss"].detach(),
               "elbo": r["elbo"].detach(), **{"grad." + k: v.grad for k, v in sd.items()}}
    return m.to(DEV), (x.to(DEV), x_sl, eps.to(DEV)), ref


def _step(B, S, width=H, fill=None):
    """One forward + backward under the switches in effect.  fill: an int32 word every buffer `blvm.ops` allocates with torch.empty /
    empty_like holds before the call (the outputs, the decoder's activations and the reserve among them).  -> results, folded calls."""
    lib = _lib()
    m, (x, x_sl, eps), _ = _case(B, S, width)
    m.zero_grad(set_to_none=True)
    seen = {}
    real = ops.mlp_dmol_log_prob

    def spy(*a, **k):
        given = k.get("given", a[16] if len(a) > 16 else None)
        dec, lp = real(*a, **k)
        seen.update(dec=dec, given=given)
        return dec, lp

    class Filled:
        def __getattr__(self, name):
            return getattr(torch, name)

        @staticmethod
        def _fill(t):
            if t.numel() and t.dtype in (torch.float32, torch.int32):
                t.view(torch.int32).fill_(fill)
            return t

        def empty(self, *a, **k):
            return self._fill(torch.empty(*a, **k))

        def empty_like(self, *a, **k):
            return self._fill(torch.empty_like(*a, **k))

    n0 = lib.blvm_vrnn_dec_fold(-2)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "mlp_dmol_log_prob", spy)
        if fill is not None:
            mp.setattr(ops, "torch", Filled())
        loss, _, out = m(x, x_sl, beta=1.0, free_nats=2.0, eps=eps)
        loss.backward()
    torch.cuda.synchronize()
    assert _hip.take_async_errors() == (0, 0)
    res = {"loss": loss.detach().clone(), "elbo": out.elbo.detach().clone(), "kl": out.kl.detach().clone(), "z": out.z.detach().clone(),
           "h_n": out.h_n.detach().clone(), "log_prob": out.log_prob.detach().clone(), "dec": seen["dec"].clone()}
    if seen["given"] is not None:
        if len(seen["given"]) == 3:
            assert seen["given"][2].data_ptr() == seen["dec"].data_ptr()  # the head read the launch's own buffer
        res.update(y1=seen["given"][0].clone(), y2=seen["given"][1].clone())
    for k, p in m.named_parameters():
        res["grad." + k] = p.grad.detach().clone()
    for k, v in res.items():
        assert bool(torch.isfinite(v).all()), k
    return res, lib.blvm_vrnn_dec_fold(-2) - n0


@functools.lru_cache(maxsize=None)
def _folded(B, S):
    with switches(fold=True, static=True) as lib:
        n0 = lib.blvm_pchain_static(-2)
        res, n = _step(B, S)
        assert n == 1 and lib.blvm_pchain_static(-2) - n0 == 2  # folded, on the static kernels (forward and backward)
    return res


@functools.lru_cache(maxsize=None)
def _unfolded(B, S):
    with switches(fold=False, static=True):
        res, n = _step(B, S)
        assert n == 0 and "y1" not in res
    return res


@pytest.mark.parametrize("B,S", CASES)
def test_static_walk_matches_interpreter_on_the_extended_program(B, S):
    """The same ten descriptors on the static kernel and on the interpreter: every output of the step bit-identical, the decoder's
    three buffers included; gradients as `test_gpu_vrnn_static.py` states it (split-K atomics: <= 1e-6 relative)."""
    static = _folded(B, S)
    with switches(fold=True, static=False) as lib:
        n0 = lib.blvm_pchain_static(-2)
        interp, n = _step(B, S)
        assert n == 1 and lib.blvm_pchain_static(-2) == n0
    assert static.keys() == interp.keys() and {"y1", "y2"} <= static.keys()
    bad = [k for k in (*EXACT, *DECODER) if not torch.equal(static[k], interp[k])]
    assert not bad, f"static walk and interpreter differ in {bad}"
    bad = [(k, rel_l2(static[k], interp[k])) for k in static if k.startswith("grad.") and rel_l2(static[k], interp[k]) > 1e-6]
    assert not bad, bad[:8]


@pytest.mark.parametrize("B,S", CASES)
def test_folded_against_unfolded_and_the_oracle(B, S):
    """z, h_n and the KL bit-identical with the fold on and off; dec, log_prob, the loss and every gradient at most twice as far
    from the float64 oracle folded as unfolded."""
    ref = _case(B, S)[2]
    on, off = _folded(B, S), _unfolded(B, S)
    bad = [k for k in EXACT if not torch.equal(on[k], off[k])]
    assert not bad, f"the fold changed {bad}"
    rows, worse = [], []
    for k in ["dec", "log_prob", "loss", "y1", "y2", *[k for k in on if k.startswith("grad.")]]:
        e_on = rel_l2(on[k], ref[k])
        e_off = rel_l2(off[k], ref[k]) if k in off else None  # (y1, y2: the unfolded path keeps them inside its autograd node)
        rows.append((k, e_on, e_off))
        if e_off is not None and e_on > 2 * e_off:
            worse.append((k, e_on, e_off))
    print(f"B={B} S={S}: error against the oracle, folded | unfolded")
    for k, a, b in rows:
        print(f"  {k:55s} {a:.3e} | " + (f"{b:.3e}" if b is not None else "-"))
    assert not worse, worse
    assert max(rel_l2(on[k], ref[k]) for k in ("y1", "y2")) < 1e-5  # fp32 K = 768 / 256 sums


@pytest.mark.parametrize("B,S", [(17, 8), (64, 64)])
def test_first_two_layers_only(B, S):
    """blvm_vrnn_dec_fold(2): the launch runs the first two layers (nine descriptors) and the last stays a K6 GEMM on the launch's y2.
    y1, y2 and everything the chain computes are what the full fold gives, bit for bit; dec is within the bound against the oracle."""
    ref, full, off = _case(B, S)[2], _folded(B, S), _unfolded(B, S)
    with switches(fold=2, static=True) as lib:
        n0 = lib.blvm_pchain_static(-2)
        two, n = _step(B, S)
        assert n == 1 and lib.blvm_pchain_static(-2) - n0 == 2
    bad = [k for k in (*EXACT, "y1", "y2") if not torch.equal(two[k], full[k])]
    assert not bad, bad
    for k in ("dec", "log_prob", "loss"):
        assert rel_l2(two[k], ref[k]) <= 2 * rel_l2(off[k], ref[k]), k


@pytest.mark.parametrize("word", [NAN_WORD, SENTINEL_WORD], ids=["nan", "sentinel"])
@pytest.mark.parametrize("B,S", [(17, 8), (64, 64)])
def test_results_do_not_depend_on_what_the_buffers_held(B, S, word):
    """Every buffer the step allocates (the decoder's activations and the grown reserve among them) pre-filled with quiet NaNs or with
    the hand-off sentinel: the forward's results are bit-identical to the plain run's."""
    plain = _folded(B, S)
    with switches(fold=True, static=True):
        got, n = _step(B, S, fill=word)
    assert n == 1
    bad = [k for k in (*EXACT, "y1", "y2", "dec") if not torch.equal(plain[k], got[k])]
    assert not bad, f"results depend on what the buffers held: {bad}"
    for k in ("loss", "elbo", "log_prob"):
        assert rel_l2(got[k], plain[k]) < 1e-12, k  # (float64 sums accumulated with atomics)
    bad = [(k, rel_l2(got[k], plain[k])) for k in plain if k.startswith("grad.") and rel_l2(got[k], plain[k]) > 1e-6]
    assert not bad, bad[:8]


@pytest.mark.parametrize("case", ["bf16", "B65", "width128"])
def test_fallbacks_run_the_unfolded_path(case):
    """16-bit operands, a batch past the 16-row tiles and a decoder whose hidden width is not H: nothing folds (the counter stands
    still) and the step is what the switch at 0 gives, bit for bit in the forward's results."""
    lib = _lib()
    B, S, width = (65, 8, H) if case == "B65" else (17, 8, 128) if case == "width128" else (17, 8, H)
    old = lib.blvm_get_operand_dtype()
    if case == "bf16":
        lib.blvm_set_operand_dtype(1)
    try:
        with switches(fold=True):
            on, n_on = _step(B, S, width)
        with switches(fold=False):
            off, n_off = _step(B, S, width)
    finally:
        lib.blvm_set_operand_dtype(old)
    assert (n_on, n_off) == (0, 0) and "y1" not in on
    bad = [k for k in (*EXACT, "dec", "loss", "elbo", "log_prob") if not torch.equal(on[k], off[k])]
    assert not bad, bad
    bad = [(k, rel_l2(on[k], off[k])) for k in on if k.startswith("grad.") and rel_l2(on[k], off[k]) > 1e-6]
    assert not bad, bad[:8]
