"""GPU (MI355X): WaveNet with the Gaussian and Gaussian-mixture heads — training against the reference's values
(tests/golden/wavenet_gauss.npz) and generation on the three paths (one launch K10c, window, block by block) against the float64
restatement of tests/wavenet_gauss_cases.py.

Generation bound: test_wavenet_prompt.py's TOL = 1e-4 was set for samples clamped to [-1, 1].  The Gaussian draws are not clamped
(samples up to |x| = 2.3 in these cases), so a sample is compared relative to its size once that exceeds 1:
|hip - x64| <= TOL * max(1, |x64|).  Ties are excluded by construction (test_wavenet_gauss_cpu.py::test_cases_have_no_near_ties), so
EVERY sample is compared."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from blvm import _hip, ops

from conftest import GOLDEN
from test_gpu_buffer_contract import poisoned
from test_wavenet_prompt import MIN_GAP, TOL, window_of
import wavenet_gauss_cases as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 12345.0


def T(a):
    return torch.from_numpy(np.asarray(a))


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope="module", autouse=True)
def _require_hip():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert _hip.load().blvm_device_ok() == 1, "libblvm_hip: no gfx950 device visible"


# ---- training ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("p,pad_rf", [("s", True), ("n", False)])
@pytest.mark.parametrize("tag,head,nsf", [("gauss", "Gaussian", 1), ("gmm3", "GMM-3", 1), ("gmm10", "GMM-10", 1), ("stk", "GMM-3", 4)])
def test_training_vs_reference_golden(tag, head, nsf, p, pad_rf):
    """Loss, log_prob, log_prob_twise, metrics, dx and every parameter gradient at the tolerances of
    test_gpu_parity.py::test_wavenet_small_vs_reference_golden; the lazy outputs in the reference's shapes."""
    from blvm.models import WaveNet

    g = np.load(os.path.join(GOLDEN, "wavenet_gauss.npz"))
    hd = W.HEADS[head]
    m = WaveNet(likelihood=hd.module(16), n_layers=3, n_stacks=2, res_channels=16, kernel_size=2, base_dilation=2, n_stack_frames=nsf)
    pre = f"{tag}.sd."
    m.load_state_dict({k[len(pre) :]: T(g[k]) for k in g.files if k.startswith(pre)})
    m = m.to(DEV)
    assert m.receptive_field == int(g[f"{tag}.rf"])
    x = T(g[f"{tag}.x"]).to(DEV).requires_grad_(True)
    loss, metrics, out = m(x, T(g[f"{tag}.x_sl"]), pad_receptive_field=pad_rf)
    loss.backward()
    assert float(loss) == pytest.approx(float(g[f"{tag}.{p}_loss"]), rel=1e-5)
    torch.testing.assert_close(out.log_prob.cpu(), T(g[f"{tag}.{p}_log_prob"]), rtol=1e-5, atol=1e-3)
    ref_tw = T(g[f"{tag}.{p}_ll_twise"])
    torch.testing.assert_close(out.log_prob_twise.cpu(), ref_tw, rtol=1e-4, atol=1e-4)
    vals = {mm.name: mm.value for mm in metrics}
    for name, val in zip(g[f"{tag}.{p}_metric_names"].tolist(), g[f"{tag}.{p}_metric_values"].tolist()):
        assert vals[name] == pytest.approx(val, rel=1e-5), name
    assert rel_l2(x.grad, T(g[f"{tag}.{p}_dx"])) < 1e-3
    for k, prm in m.named_parameters():
        assert rel_l2(prm.grad, T(g[f"{tag}.{p}_grad.{k}"])) < 1e-3, k
    B, Ty = ref_tw.shape
    par = out.parameters
    if hd.num_mix:
        assert [tuple(t.shape) for t in par] == [(B, Ty, hd.num_mix), (B, Ty, 1, hd.num_mix), (B, Ty, 1, hd.num_mix)]
    else:
        assert [tuple(t.shape) for t in par] == [(B, Ty, 1), (B, Ty, 1)]
    assert bool((par[-1] > 0).all())
    assert out.predictions.shape == out.predictions_mode.shape == (B, Ty, 1)
    assert bool(torch.isfinite(out.predictions).all())


def test_forward_split_runs_with_a_mixture_head():
    """`forward_split` (the experiment's --split_eval): split 0 pads the receptive field, the later ones do not; finite losses."""
    m = W.build_model("g16", "GMM-3").to(DEV)
    g = torch.Generator().manual_seed(3)
    x, x_sl = torch.rand(3, 150, generator=g) * 1.6 - 0.8, torch.tensor([150, 111, 64])
    xs, sls = m.split_sequence(x, x_sl, length=64)
    assert len(xs) > 1
    for i, (x_i, sl_i) in enumerate(zip(xs, sls)):
        loss, _, out = m.forward_split(x_i.to(DEV), sl_i, i_split=i)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(out.log_prob).all()), i


# ---- generation -------------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def gpu_model(shape, head):
    return W.build_model(shape, head).to(DEV)


def _dev(uni):
    return [(None if u is None else u.to(DEV), n.to(DEV)) for u, n in uni]


def _within(tag, got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err, bar = (got - want).abs(), TOL * want.abs().clamp(min=1.0)
    print(f"{tag}: max |diff| {float(err.max()):.3e}, max |diff| / bar {float((err / bar).max()):.3g}, beyond the bar: {int((err > bar).sum())} of {err.numel()}")
    assert bool((err <= bar).all()), tag


def _no_block_step(*a, **k):
    raise AssertionError("ops.wavenet_block_step was called on the one-launch path")


@pytest.mark.parametrize("shape,head,P", W.ONE_LAUNCH)
def test_one_launch_generation_matches_float64_and_the_other_paths(monkeypatch, shape, head, P):
    """generate(cached=True) in one launch (block steps forbidden) from the zero start (P = 0) or a prompt, against the float64
    restatement; the window path and the block-by-block path on the same draws agree with it."""
    case = W.case_of(shape, head)
    _, prompt, uni, x64, gap = W.reference(shape, head, P)
    assert gap >= MIN_GAP
    m = gpu_model(shape, head)
    assert m._gauss_decode_kernel_applies() and not m._decode_kernel_applies() and not m._cat_decode_kernel_applies()
    kw = dict(x=prompt.to(DEV)) if P else {}
    with monkeypatch.context() as mp:
        mp.setattr(ops, "wavenet_block_step", _no_block_step)
        got = m.generate(n_samples=case.B, n_frames=case.n_frames, uniforms=_dev(uni), cached=True, **kw)
    assert tuple(got.shape) == (case.B, case.n_frames, 1) and bool(torch.isfinite(got).all())
    _within(f"{shape} {head} P={P} one launch vs float64", got, x64)
    win = m.generate(n_samples=case.B, n_frames=case.n_frames, x=window_of(prompt, case.rf).to(DEV), uniforms=_dev(uni), cached=False)
    _within(f"{shape} {head} P={P} one launch vs window path", got, win)
    _within(f"{shape} {head} P={P} window path vs float64", win, x64)
    blk = m._generate_cached(case.B, case.n_frames, _dev(uni), state=m._prime(prompt.to(DEV)) if P else None)
    _within(f"{shape} {head} P={P} one launch vs block by block", got, blk)
    _within(f"{shape} {head} P={P} block by block vs float64", blk, x64)


@pytest.mark.parametrize("shape,head,P", W.BLOCK_BY_BLOCK)
def test_eleven_components_generate_block_by_block(monkeypatch, shape, head, P):
    """3 * 11 > 32 head rows: generate(cached=True) must not reach the decode kernel, and matches float64 and the window path."""
    case = W.case_of(shape, head)
    _, prompt, uni, x64, gap = W.reference(shape, head, P)
    assert gap >= MIN_GAP
    m = gpu_model(shape, head)
    assert not m._gauss_decode_kernel_applies()
    kw = dict(x=prompt.to(DEV)) if P else {}
    with monkeypatch.context() as mp:
        mp.setattr(ops, "wavenet_decode", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the decode kernel was called")))
        got = m.generate(n_samples=case.B, n_frames=case.n_frames, uniforms=_dev(uni), cached=True, **kw)
    _within(f"{shape} {head} P={P} block by block vs float64", got, x64)
    win = m.generate(n_samples=case.B, n_frames=case.n_frames, x=window_of(prompt, case.rf).to(DEV), uniforms=_dev(uni), cached=False)
    _within(f"{shape} {head} P={P} block by block vs window path", got, win)


@pytest.mark.parametrize("shape,head,P,n", [("g16", "GMM-10", 11, 5), ("g16", "GMM-3", 0, 7), ("g16", "Gaussian", 40, 5), ("r32", "GMM-10", 70, 9),
                                            ("r32", "Gaussian", 0, 7), ("r64", "GMM-3", 601, 5), ("r64", "GMM-10", 0, 3), ("g16", "GMM-11", 11, 5)])  # fmt: skip
def test_generation_in_two_chunks_is_bit_identical(shape, head, P, n):
    """2n frames in one call == n frames with return_state=True, then n frames from the state; n odd and below the largest dilation."""
    case = W.case_of(shape, head)
    assert n % 2 == 1 and n < max(case.dilations) and 2 * n <= case.n_frames
    prompt, uni = W.draws(shape, head, P)
    m = gpu_model(shape, head)
    uni = _dev(uni)[: 2 * n]
    kw = dict(x=prompt.to(DEV)) if P else {}
    whole = m.generate(n_samples=case.B, n_frames=2 * n, uniforms=uni, cached=True, **kw)
    first, state = m.generate(n_samples=case.B, n_frames=n, uniforms=uni[:n], cached=True, return_state=True, **kw)
    assert state.n_frames == P + n and tuple(state.samples.shape) == (case.B, 2)
    assert torch.equal(state.samples[:, 1], first[:, -1, 0]) and torch.equal(state.samples[:, 0], first[:, -2, 0])
    second, state2 = m.generate(n_samples=case.B, n_frames=n, uniforms=uni[n:], cached=True, state=state, return_state=True)
    assert state2.n_frames == P + 2 * n and torch.equal(state2.samples[:, 1], second[:, -1, 0])
    chunks = torch.cat([first, second], 1)
    assert tuple(chunks.shape) == tuple(whole.shape) == (case.B, 2 * n, 1)
    assert torch.equal(whole, chunks)


@pytest.mark.parametrize("shape,head", [("g16", "GMM-10"), ("g16", "Gaussian"), ("r64", "GMM-3")])
def test_zero_prompt_equals_the_zero_start(shape, head):
    case = W.case_of(shape, head)
    _, _, uni, x64, _ = W.reference(shape, head, 0)
    m = gpu_model(shape, head)
    a = m.generate(n_samples=case.B, n_frames=case.n_frames, uniforms=_dev(uni), cached=True)
    b = m.generate(n_samples=case.B, n_frames=case.n_frames, x=torch.zeros(case.B, case.rf, 1, device=DEV), uniforms=_dev(uni), cached=True)
    _within(f"{shape} {head} zero prompt vs zero start", b, a)
    _within(f"{shape} {head} zero prompt vs float64", b, x64)


@pytest.mark.parametrize("shape,head", [("g16", "GMM-10"), ("g16", "GMM-3"), ("g16", "GMM-1"), ("g16", "Gaussian"), ("r32", "GMM-3"), ("g128", "GMM-10")])
def test_no_draws_gives_the_arg_max_components_mean(shape, head):
    """`ops.wavenet_decode(draws=None)`: every frame is the mean of the component with the largest logit (the Gaussian head: the
    mean), fed back as the next input — the float64 restatement of exactly that."""
    case = W.case_of(shape, head)
    x64, gap = W.mode_reference(shape, head)
    assert gap >= MIN_GAP
    m = gpu_model(shape, head)
    blk = m.res_stack.res_blocks[0]
    hd = ops.GmmHead(case.num_mix, m.likelihood.softplus_beta, W.EPS) if case.num_mix else ops.GaussHead(m.likelihood.softplus_beta, W.EPS)
    out = ops.wavenet_decode(m._one_launch_parts(), hd, case.B, case.n_frames, blk.inv_std, 1.0 / m.variance_scale, draws=None)
    _within(f"{shape} {head} mode vs float64", out.x.unsqueeze(-1), x64)


# ---- the caller-owned buffers -----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("shape,head,P", [("r32", "GMM-10", 70), ("r32", "Gaussian", 70), ("g16", "GMM-3", 0)])
def test_results_do_not_depend_on_what_the_buffers_held(monkeypatch, shape, head, P):
    """The zero-start call and the resumed call (a prompt's state, or the zero start's own) under `poisoned` `nan` and `noise`:
    identical bits, no NaN."""
    case = W.case_of(shape, head)
    prompt, uni = W.draws(shape, head, P)
    m = gpu_model(shape, head)
    uni, n = _dev(uni), 5
    res = {}
    for mode in ("nan", "noise"):
        with poisoned(monkeypatch, mode) as h:
            kw = dict(x=prompt.to(DEV)) if P else {}
            first, state = m.generate(n_samples=case.B, n_frames=n, uniforms=uni[:n], cached=True, return_state=True, **kw)
            second, state = m.generate(n_samples=case.B, n_frames=n, uniforms=uni[n : 2 * n], cached=True, state=state, return_state=True)
            torch.cuda.synchronize()
        assert h.count > 0
        res[mode] = (first.cpu(), second.cpu(), state.samples.cpu(), torch.cat([r.reshape(-1) for r in state.rings]).cpu())
        for t in res[mode]:
            assert bool(torch.isfinite(t).all()), mode
    for a, b in zip(res["nan"], res["noise"]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------


def test_entry_points_refuse_before_any_launch():
    """head_kind outside {1, 2}, eleven components (33 head rows), a width that is no multiple of 16 and more than 64 blocks: an
    error code, a message that names the value, and every output left as it was."""
    lib = _hip.load()
    shape, head = "g16", "GMM-3"
    case, m = W.case_of(shape, head), gpu_model(shape, head)
    B, C, n, nb = case.B, case.C, 4, len(case.dilations)
    dil = (ctypes.c_int * 65)(*case.dilations, *([1] * (65 - nb)))
    packed = torch.zeros(lib.blvm_wavenet_decode_pack_floats(C, C, C, 65), device=DEV)
    scratch = torch.full((lib.blvm_wavenet_decode_scratch_floats(dil, 65, 16, C, C),), SENTINEL, device=DEV)
    x_out, x_state = torch.full((16, n), SENTINEL, device=DEV), torch.full((16, 2), SENTINEL, device=DEV)
    x_in = torch.zeros(16, 2, device=DEV)
    u, nrm = torch.full((n, B, 11), 0.5, device=DEV), torch.zeros(n, B, device=DEV)
    beta = float(m.likelihood.softplus_beta)

    def call(resume, kind=1, num_mix=3, C_=C, nb_=nb):
        a = (packed.data_ptr(), dil, nb_, B, C_, C_, C_, kind, num_mix, n)
        if resume:
            return lib.blvm_wavenet_gauss_decode_resume(*a, 7, 0.7, 1.0, beta, W.EPS, u.data_ptr(), nrm.data_ptr(), x_in.data_ptr(),
                                                        scratch.data_ptr(), x_out.data_ptr(), x_state.data_ptr(), None)  # fmt: skip
        return lib.blvm_wavenet_gauss_decode(*a, 0.7, 1.0, beta, W.EPS, u.data_ptr(), nrm.data_ptr(), scratch.data_ptr(), x_out.data_ptr(), None)

    for resume in (False, True):
        for kw, word in ((dict(kind=0), "head_kind"), (dict(kind=3), "head_kind"), (dict(num_mix=11), "num_mix"), (dict(C_=24), "multiples of 16"),
                         (dict(nb_=65), "n_blocks")):  # fmt: skip
            assert call(resume, **kw) != 0, (resume, kw)
            assert word in lib.blvm_last_error().decode(), (kw, lib.blvm_last_error().decode())
    torch.cuda.synchronize()
    for name, t in (("x_out", x_out), ("x_state", x_state), ("scratch", scratch)):
        assert bool((t == SENTINEL).all()), f"{name} written by a refused call"
    # the host side refuses the same head before it packs anything for the device
    with pytest.raises(NotImplementedError):
        ops.wavenet_decode(gpu_model("g16", "GMM-11")._one_launch_parts(), ops.GmmHead(11, beta, W.EPS), B, n, 0.7, 1.0)
