"""GPU: one-launch cached WaveNet generation with the categorical head (`blvm_wavenet_cat_decode` / `_resume`, K10c;
`WaveNet.generate(cached=True)` on a `CategoricalDense` model with 16 <= V <= 1024).

Reference: the float64 restatement of window generation in tests/wavenet_cat_cases.py.  Its cases keep every draw at least MIN_GAP
from a CDF boundary (asserted on the CPU, tests/test_wavenet_cat_decode.py), so EVERY class is compared, none left out, and every
returned float must be `likelihood.dequantize(class)` to the bit."""
import ctypes
import functools

import pytest
import torch

import wavenet_cat_cases as W
from test_gpu_buffer_contract import poisoned

gpu = pytest.mark.gpu
DEV = "cuda:0"


def _lib():
    from blvm import _hip

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    lib = _hip.load()
    assert lib.blvm_device_ok() == 1, "libblvm_hip: no gfx950 device visible"
    return lib


@functools.lru_cache(maxsize=None)
def gpu_model(name):
    return W.build_model(W.SHAPES[name]).to(DEV)


def _dev(uni):
    return [u.to(DEV) for u in uni]


def _check_classes(tag, got, k64, lik):
    """got [B,n,1] floats == dequantize(k64) to the bit: the classes and the table at once; the message counts the classes that differ."""
    want = lik.dequantize(k64.to(DEV))
    k_got = torch.bucketize(got.squeeze(-1), lik.levels)
    wrong = int((k_got.cpu() != k64).sum())
    print(f"{tag}: classes that differ {wrong} of {k64.numel()}")
    assert got.dtype == torch.float32 and tuple(got.shape) == (*k64.shape, 1)
    assert wrong == 0, f"{tag}: {wrong} of {k64.numel()} classes differ from the float64 restatement"
    assert torch.equal(got.squeeze(-1).view(torch.int32), want.view(torch.int32)), f"{tag}: a value is not dequantize(k) to the bit"


def _forbid_block_steps(monkeypatch):
    from blvm import ops

    def refuse(*a, **k):
        raise AssertionError("the block-by-block path ran")

    monkeypatch.setattr(ops, "wavenet_block_step", refuse)


def _op_args(m, B, n, draws):
    """The arguments of `ops.wavenet_decode` for a model of either head."""
    from blvm import ops

    lik = m.likelihood
    head = ops.CategoricalHead(lik.levels) if hasattr(lik, "levels") else ops.DmolHead(lik.num_mix, lik.log_epsilon)
    return m._one_launch_parts(), head, B, n, m.res_stack.res_blocks[0].inv_std, 1.0 / m.variance_scale, draws


# ---- 1: one-launch generation ------------------------------------------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("name,P", W.STARTS)
def test_one_launch_generation_matches_float64(name, P, monkeypatch):
    """generate(cached=True) of a categorical model inside the predicate, from a zero start and from a prompt, with the block-by-block
    path's kernel wrapper made to raise: shape [B,n,1] float32, every class the float64 restatement's, every value dequantize(k)."""
    _lib()
    case = W.SHAPES[name]
    _, prompt, uni, r = W.reference(name, P)
    assert r["gap"] >= W.MIN_GAP
    m = gpu_model(name)
    assert m._cat_decode_kernel_applies() is True and m._decode_kernel_applies() is False
    _forbid_block_steps(monkeypatch)
    kw = dict(x=prompt.to(DEV)) if P else {}
    got = m.generate(n_samples=case.B, n_frames=case.n_frames, uniforms=_dev(uni), cached=True, **kw)
    _check_classes(f"{name} P={P} one launch vs float64", got, r["k"], m.likelihood)


# ---- 2: agreement with the other paths --------------------------------------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("name", ["c16v32", "c32v256"])
def test_one_launch_window_and_block_by_block_paths_draw_the_same_classes(name):
    _lib()
    case = W.SHAPES[name]
    _, _, uni, r = W.reference(name, 0)
    assert r["gap"] >= W.MIN_GAP
    m = gpu_model(name)
    uni = _dev(uni)
    one = m.generate(n_samples=case.B, n_frames=case.n_frames, uniforms=uni, cached=True)
    win = m.generate(n_samples=case.B, n_frames=case.n_frames, uniforms=uni, cached=False)
    blk = m._generate_cached(case.B, case.n_frames, uni)
    _check_classes(f"{name} one launch", one, r["k"], m.likelihood)
    assert torch.equal(one, win), "one launch vs the window path"
    assert torch.equal(one, blk), "one launch vs block by block"


@gpu
def test_a_softmax_of_2048_classes_still_generates_block_by_block(monkeypatch):
    from blvm import ops

    _lib()
    case = W.SHAPES["v2048"]
    _, _, uni, r = W.reference("v2048", 0)
    assert r["gap"] >= W.MIN_GAP
    m = gpu_model("v2048")
    assert m._cat_decode_kernel_applies() is False and m._decode_kernel_applies() is False
    calls, step = [], ops.wavenet_block_step
    monkeypatch.setattr(ops, "wavenet_block_step", lambda *a, **k: (calls.append(1), step(*a, **k))[1])
    uni = _dev(uni)
    got = m.generate(n_samples=case.B, n_frames=case.n_frames, uniforms=uni, cached=True)
    assert len(calls) >= case.n_frames * len(case.dilations)
    win = m.generate(n_samples=case.B, n_frames=case.n_frames, uniforms=uni, cached=False)
    assert torch.equal(got, win)
    _check_classes("v2048 block by block vs float64", got, r["k"], m.likelihood)


# ---- 3: chunks -----------------------------------------------------------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("name,P,n", [("c16v32", 11, 5), ("c16v32", 0, 7), ("c32v256", 70, 9), ("c32v256", 0, 7), ("c64v1024", 77, 5),
                                      ("c64v1024", 0, 7), ("c128v16", 9, 3), ("c128v16", 0, 3)])  # fmt: skip
def test_generation_in_two_chunks_is_bit_identical(name, P, n, monkeypatch):
    """2n frames in one call == n frames with return_state=True, then n frames from the state; n is odd and smaller than the largest
    dilation, so the split lands inside the rings; P = 0 is the zero start, whose first call is the steady-state entry."""
    _lib()
    case = W.SHAPES[name]
    assert n % 2 == 1 and n < max(case.dilations) and 2 * n <= case.n_frames
    prompt, uni = W.draws(case, P)
    m = gpu_model(name)
    _forbid_block_steps(monkeypatch)
    uni = _dev(uni)[: 2 * n]
    kw = dict(x=prompt.to(DEV)) if P else {}
    whole = m.generate(n_samples=case.B, n_frames=2 * n, uniforms=uni, cached=True, **kw)
    first, state = m.generate(n_samples=case.B, n_frames=n, uniforms=uni[:n], cached=True, return_state=True, **kw)
    assert state.n_frames == P + n and tuple(state.samples.shape) == (case.B, 2) and state.scratch is not None
    assert torch.equal(state.samples[:, 1], first[:, -1, 0]) and torch.equal(state.samples[:, 0], first[:, -2, 0])
    second, state2 = m.generate(n_samples=case.B, n_frames=n, uniforms=uni[n:], cached=True, state=state, return_state=True)
    assert state2.n_frames == P + 2 * n and torch.equal(state2.samples[:, 1], second[:, -1, 0])
    chunks = torch.cat([first, second], 1)
    assert tuple(chunks.shape) == tuple(whole.shape) == (case.B, 2 * n, 1)
    assert torch.equal(whole.view(torch.int32), chunks.view(torch.int32))
    assert len(whole.unique()) >= 4  # (no constant output)


@gpu
@pytest.mark.parametrize("name", ["c16v32", "c64v1024"])
def test_zero_prompt_equals_the_zero_start(name):
    """A prompt of rf zeros is the all-zero past: the primed rings and the steady-state fill give the same classes."""
    _lib()
    case = W.SHAPES[name]
    _, _, uni, r = W.reference(name, 0)
    assert r["gap"] >= W.MIN_GAP
    m = gpu_model(name)
    a = m.generate(n_samples=case.B, n_frames=case.n_frames, uniforms=_dev(uni), cached=True)
    b = m.generate(n_samples=case.B, n_frames=case.n_frames, x=torch.zeros(case.B, case.rf, 1, device=DEV), uniforms=_dev(uni), cached=True)
    assert torch.equal(a, b)
    _check_classes(f"{name} zero prompt vs float64", b, r["k"], m.likelihood)


@gpu
def test_a_block_by_block_state_is_refused():
    """A state of `_generate_cached` from a zero start has no scratch buffer: the ValueError of the DMoL path."""
    _lib()
    case = W.SHAPES["c16v32"]
    m = gpu_model("c16v32")
    _, state = m._generate_cached(case.B, 2, None, want_state=True)
    assert state.scratch is None
    with pytest.raises(ValueError, match="does not come from the decode kernel's path"):
        m.generate(n_samples=case.B, n_frames=2, cached=True, state=state)


# ---- 4: mode ---------------------------------------------------------------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("name", W.KERNEL_CASES)
def test_without_uniforms_every_frame_is_the_first_arg_max_class(name):
    from blvm import ops

    _lib()
    case = W.SHAPES[name]
    r = W.mode_reference(name)
    assert r["logit_gap"] >= W.MIN_LOGIT_GAP
    m = gpu_model(name)
    x, k = ops.wavenet_decode(*_op_args(m, case.B, case.n_frames, None))[:2]
    assert k.dtype == torch.int32 and tuple(k.shape) == (case.B, case.n_frames)
    wrong = int((k.cpu().long() != r["k"]).sum())
    print(f"{name} mode: classes that differ {wrong} of {k.numel()}")
    assert wrong == 0
    assert torch.equal(x, m.likelihood.dequantize(k))


@gpu
def test_the_class_output_and_sampling_without_given_uniforms():
    """`k_out` holds the classes of `x_out`; `uniforms=None` draws on the device: values are levels, and not one constant."""
    from blvm import ops

    _lib()
    case = W.SHAPES["c32v256"]
    _, _, uni, r = W.reference("c32v256", 0)
    m = gpu_model("c32v256")
    x, k = ops.wavenet_decode(*_op_args(m, case.B, case.n_frames, torch.stack(_dev(uni))))[:2]
    assert torch.equal(k.cpu().long(), r["k"]) and torch.equal(x, m.likelihood.dequantize(k))
    torch.manual_seed(3)
    free = m.generate(n_samples=case.B, n_frames=case.n_frames, cached=True)
    kf = torch.bucketize(free.squeeze(-1), m.likelihood.levels)
    assert torch.equal(m.likelihood.dequantize(kf), free.squeeze(-1)) and len(kf.unique()) >= 8


# ---- 5: buffer contract ----------------------------------------------------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("mode", ["nan", "noise"])
def test_results_do_not_depend_on_what_the_buffers_held(mode, monkeypatch):
    """The zero-start call and the resume call of either head with every `torch.empty` of blvm.ops pre-filled (NaN words, noise):
    identical bits to the unpoisoned run, no NaN, and the harness did poison buffers.  The categorical head at c32v256, the DMoL head
    at the r32 shape of tests/test_wavenet_prompt.py; 7 frames per call."""
    import test_wavenet_prompt as WP
    from blvm import ops

    _lib()
    n = 7
    cat, dmol = W.SHAPES["c32v256"], WP.SHAPES["r32"]
    u_cat = torch.stack(_dev(W.draws(cat, 0)[1]))
    uni = WP.draws(dmol, 0)[1]
    u = torch.stack([a.reshape(dmol.B, dmol.num_mix) for a, _ in uni]).to(DEV)
    v = torch.stack([b.reshape(dmol.B) for _, b in uni]).to(DEV)
    sides = [(gpu_model("c32v256"), cat.B, lambda lo, hi: u_cat[lo:hi]), (WP.gpu_model("r32"), dmol.B, lambda lo, hi: (u[lo:hi], v[lo:hi]))]

    def run(m, B, draws):
        a = ops.wavenet_decode(*_op_args(m, B, n, draws(0, n)))
        b = ops.wavenet_decode(*_op_args(m, B, n, draws(n, 2 * n)), resume=(n, a.x[:, -2:].contiguous(), a.scratch))
        torch.cuda.synchronize()
        return [t.clone() for t in (a.x, a.k, b.x, b.k, b.samples) if t is not None]

    clean = [run(*side) for side in sides]
    with poisoned(monkeypatch, mode) as h:
        dirty, counts = [], []
        for side in sides:
            before = h.count
            dirty.append(run(*side))
            counts.append(h.count - before)
    assert h.count >= 6, "the harness poisoned fewer buffers than the two calls allocate"
    # per head: scratch, x, k | x, k, samples; the DMoL head has no k
    assert counts[0] >= 6 and counts[1] >= 4, counts
    for a, b in zip(clean[0] + clean[1], dirty[0] + dirty[1]):
        assert not bool(torch.isnan(b.float()).any())
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert len(clean[0][1].unique()) >= 8 and len(clean[1][0].unique()) >= 8


# ---- 6: refusals -----------------------------------------------------------------------------------------------------------------------


@gpu
def test_unsupported_widths_are_refused_before_any_launch():
    from blvm import _hip

    lib = _lib()
    ENOSUP = _hip.CONSTANTS["BLVM_ENOSUP"]
    B, n = 2, 3
    dil = (ctypes.c_int * 2)(1, 2)
    buf = torch.zeros(4096, device=DEV)  # stands for every read-only operand: no call below gets as far as reading it
    out = torch.full((B, n), -7.0, device=DEV)
    k_out = torch.full((B, n), -7, device=DEV, dtype=torch.int32)
    state = torch.full((B, 2), -7.0, device=DEV)

    def both(C, V):
        p = buf.data_ptr()
        yield lib.blvm_wavenet_cat_decode(p, dil, 2, B, C, C, C, V, n, 0.7, 1.0, p, p, p, out.data_ptr(), k_out.data_ptr(), None)
        yield lib.blvm_wavenet_cat_decode_resume(p, dil, 2, B, C, C, C, V, n, 4, 0.7, 1.0, p, p, p, p, out.data_ptr(), k_out.data_ptr(),
                                                 state.data_ptr(), None)  # fmt: skip

    for V in (2048, 24, 8, 0):
        for rc in both(16, V):
            assert rc == ENOSUP, V
            msg = lib.blvm_last_error().decode()
            assert f"V = {V}" in msg and "16 <= V <= 1024" in msg, msg
    for rc in both(512, 1024):
        assert rc != 0
        msg = lib.blvm_last_error().decode()
        assert "bytes of LDS (> 160 KB)" in msg and "V=1024" in msg, msg
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((k_out == -7).all()) and bool((state == -7.0).all()) and bool((buf == 0).all())
