"""K4b: both directions of a bidirectional LSTM layer in one launch (`blvm_lstm_bidir_fwd/_bwd`, csrc/seqchain.hip
lstm_bidir_*_kernel, `ops.lstm_bidir_sequence`, `LSTMBlock`).

Reference: the float64 reference of tests/test_gpu_rnn_sequences.py for K4 — `blvm_oracle.lstm_sequence_ref`, the reverse direction
between two `blvm_oracle.reverse_sequences` — with that file's bars and per-row checks (`Checks`): relative L2 <= 1e-5 for out,
<= 2e-5 for d_in and each of the eight weight / bias gradients; exact zeros in both halves of out past a row's length.  Lengths:
`rnn_arms.unsorted_lens` (unsorted, one full row, one row of length 1, one row of length 0 inside the last row tile).

Shapes (T, B, I, H), one per way the kernel can go wrong: (5,3,5,128) one partial row tile; (4,16,24,128) an exact tile at the
shortest T the persistent path takes; (7,17,24,128) two row tiles, the second with one row; (5,3,5,256) two k-chunks per wave forward
and eight backward; (5,17,5,384) three and twelve k-chunks, the shared-slab product.  With the unsorted pattern the one row of
(7,17,.)'s second tile has length 0, so that shape also runs with descending lengths >= 1 (every tile live).

In f32 and in both 16-bit operand modes `out` has the BITS of the two-call composition LSTMBlock builds otherwise: the per-element
arithmetic is that of the unidirectional kernels and the gathers only move values.  Gradients are compared with float64 only (the
reverse direction's weight-gradient GEMMs sum their rows in another order)."""
import ctypes
import functools

import pytest
import torch

import blvm_oracle as O
from asr_reference import TorchASR
from blvm import _hip, ops
from blvm.modules.lstm_block import LSTMBlock, _reverse
from rnn_arms import sorted_lens, unsorted_lens
from test_gpu_lstm_asr import within
from test_gpu_rnn_sequences import BAR_GRAD, BAR_VALUE, Checks, path_counts

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NOT_APPLICABLE = _hip.CONSTANTS["BLVM_NOT_APPLICABLE"]
QNAN = 0x7FC00000
SHAPES = [(5, 3, 5, 128), (4, 16, 24, 128), (7, 17, 24, 128), (5, 3, 5, 256), (5, 17, 5, 384)]
CASES = [s + ("unsorted",) for s in SHAPES] + [(7, 17, 24, 128, "sorted")]
PARAMS = ("Wih_f", "Whh_f", "bih_f", "bhh_f", "Wih_r", "Whh_r", "bih_r", "bhh_r")


@pytest.fixture(scope="module", autouse=True)
def _require_hip():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert _hip.load().blvm_device_ok() == 1, "libblvm_hip: no gfx950 device visible"


def _id(c):
    return f"T{c[0]}-B{c[1]}-I{c[2]}-H{c[3]}" + (f"-{c[4]}" if len(c) > 4 else "")


def bidir_ref(x, lens, p):
    """The float64 composition: forward K4 reference | reverse K4 reference between two reverse_sequences."""
    fwd = O.lstm_sequence_ref(x, None, None, lens, *(p[n] for n in PARAMS[:4]))[0]
    rev = O.lstm_sequence_ref(O.reverse_sequences(x, lens), None, None, lens, *(p[n] for n in PARAMS[4:]))[0]
    return torch.cat([fwd, O.reverse_sequences(rev, lens)], dim=2)


@functools.lru_cache(maxsize=None)
def bidir_case(T_, B, I, H, lens_kind="unsorted"):
    """fp32 inputs and the float64 reference (computed once, shared by the tests; treat as read-only).  `w`, the gradient of the
    loss wrt out, is non-zero in the padding too."""
    g = torch.Generator().manual_seed(7000 * H + 10 * B + T_)
    k = H ** -0.5
    shapes = ((4 * H, I), (4 * H, H), (4 * H,), (4 * H,)) * 2
    inp = {n: (torch.rand(s, generator=g) * 2 - 1) * k for n, s in zip(PARAMS, shapes)}
    inp["x"] = torch.randn(T_, B, I, generator=g)
    inp["w"] = torch.randn(T_, B, 2 * H, generator=g)
    inp["lens"] = lens = (unsorted_lens if lens_kind == "unsorted" else sorted_lens)(T_, B)
    leaves = {n: inp[n].double().requires_grad_(True) for n in ("x",) + PARAMS}
    out = bidir_ref(leaves["x"], lens, leaves)
    (out * inp["w"].double()).sum().backward()
    return inp, dict(out=out.detach(), **{"d_" + n: t.grad for n, t in leaves.items()})


def bidir_counts():
    return ops.lstm_bidir_path_counts()


def two_call(x, lens_host, lens_dev, p):
    """What LSTMBlock builds without the one-launch call: two K4 calls, the reverse one between two gathers, and a cat."""
    fwd = ops.lstm_sequence(x, None, None, lens_dev, *(p[n] for n in PARAMS[:4]))[0]
    rev = ops.lstm_sequence(_reverse(x, lens_host), None, None, lens_dev, *(p[n] for n in PARAMS[4:]))[0]
    return torch.cat([fwd, _reverse(rev, lens_host)], dim=2)


def check_padding(ck, out, lens, H):
    out_c = out.detach().cpu()
    for b in range(out_c.shape[1]):
        n = int(lens[b])
        ck.exact(f"out[{n}:, {b}, :H] == 0 (forward half past its length)", (out_c[n:, b, :H] == 0).all())
        ck.exact(f"out[{n}:, {b}, H:] == 0 (reverse half past its length)", (out_c[n:, b, H:] == 0).all())


# ----------------------------------------------------------------------------------------------------------------------
# 1. against float64
# ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_against_float64(case):
    T_, B, I, H, lens_kind = case
    inp, ref = bidir_case(*case)
    tag = f"lstm bidir {_id(case)}"
    dev = {n: inp[n].to(DEV).requires_grad_(True) for n in ("x",) + PARAMS}
    lens_dev = inp["lens"].to(DEV, torch.int32)
    _hip.take_async_errors()
    rnn_before, before = path_counts(), bidir_counts()
    out = ops.lstm_bidir_sequence(dev["x"], lens_dev, [dev[n] for n in PARAMS[:4]], [dev[n] for n in PARAMS[4:]])
    assert out is not None, f"{tag}: the one-launch call refused a shape it must take"
    assert bidir_counts() == (before[0] + 1, before[1])
    (out * inp["w"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert bidir_counts() == (before[0] + 1, before[1] + 1)
    assert path_counts() == rnn_before, "the K4 / K2 counters moved"
    ck = Checks(tag)
    assert out.shape == (T_, B, 2 * H)
    ck.close("out", out, ref["out"], BAR_VALUE, row_dim=1)
    ck.close("out[forward half]", out[..., :H], ref["out"][..., :H], BAR_VALUE, row_dim=1)
    ck.close("out[reverse half]", out[..., H:], ref["out"][..., H:], BAR_VALUE, row_dim=1)
    ck.close("d_x", dev["x"].grad, ref["d_x"], BAR_GRAD, row_dim=1)
    for n in PARAMS:
        ck.close("d_" + n, dev[n].grad, ref["d_" + n], BAR_GRAD)
    check_padding(ck, out, inp["lens"], H)
    ck.done()


# ----------------------------------------------------------------------------------------------------------------------
# 2. the bits of the two-call composition
# ----------------------------------------------------------------------------------------------------------------------


def _same_bits(case, tag):
    inp, _ = bidir_case(*case)
    dev = {n: inp[n].to(DEV) for n in ("x",) + PARAMS}
    lens_dev = inp["lens"].to(DEV, torch.int32)
    _hip.take_async_errors()
    with torch.no_grad():
        before = bidir_counts()
        got = ops.lstm_bidir_sequence(dev["x"], lens_dev, [dev[n] for n in PARAMS[:4]], [dev[n] for n in PARAMS[4:]])
        assert got is not None and bidir_counts()[0] == before[0] + 1
        want = two_call(dev["x"], inp["lens"], lens_dev, dev)
        assert bidir_counts()[0] == before[0] + 1
    torch.cuda.synchronize()
    assert _hip.take_async_errors() == (0, 0)
    differ = int((got.view(torch.int32) != want.view(torch.int32)).sum())
    print(f"{tag}: {differ} of {got.numel()} words differ, max |diff| {float((got - want).abs().max()):.3e}")
    assert got.shape == want.shape and torch.equal(got, want), f"{tag}: {differ} words differ from the two-call composition"
    return got


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_same_bits_as_the_two_call_composition(case):
    _same_bits(case, f"lstm bidir {_id(case)} f32")


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_same_bits_in_the_16bit_operand_modes(mode):
    case = (7, 17, 24, 128, "unsorted")
    f32 = _same_bits(case, f"lstm bidir {_id(case)} f32")
    before = _hip.get_operand_dtype()
    _hip.set_operand_dtype(mode)
    try:
        got = _same_bits(case, f"lstm bidir {_id(case)} {mode}")
    finally:
        _hip.set_operand_dtype(before)
    assert not torch.equal(got, f32), f"the {mode} mode produced the f32 bits: the operand mode was not honoured"


# ----------------------------------------------------------------------------------------------------------------------
# 3. buffer contract through the raw ABI
# ----------------------------------------------------------------------------------------------------------------------


def _prefilled(n, kind, seed):
    if kind == "zeros":
        return torch.zeros(n, device=DEV, dtype=torch.float32)
    if kind == "nan":
        return torch.full((n,), QNAN, device=DEV, dtype=torch.int32).view(torch.float32)
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _raw_run(case, kind):
    T_, B, I, H, _ = case
    inp, _ = bidir_case(*case)
    lib = _hip.load()
    dev = {n: inp[n].to(DEV).contiguous() for n in ("x", "w") + PARAMS}
    lens_dev = inp["lens"].to(DEV, torch.int32)
    out = _prefilled(T_ * B * 2 * H, kind, 1).view(T_, B, 2 * H)
    reserve = _prefilled(lib.blvm_lstm_bidir_reserve_floats(T_, B, H), kind, 2)
    ws = _prefilled(lib.blvm_lstm_bidir_bwd_workspace_floats(T_, B, H), kind, 3)
    d_in = _prefilled(T_ * B * I, kind, 4).view(T_, B, I)
    grads = {n: torch.zeros_like(dev[n]) for n in PARAMS}  # accumulated: the caller zeroes them
    p, sp = _hip.ptr, _hip.stream_ptr()
    _hip.check(lib.blvm_lstm_bidir_fwd(*(p(dev[n]) for n in PARAMS), p(dev["x"]), p(lens_dev), T_, B, I, H, p(out), p(reserve), sp),
               "blvm_lstm_bidir_fwd")  # fmt: skip
    _hip.check(lib.blvm_lstm_bidir_bwd(p(dev["Wih_f"]), p(dev["Whh_f"]), p(dev["Wih_r"]), p(dev["Whh_r"]), p(dev["x"]), p(lens_dev),
                                       p(reserve), p(dev["w"]), T_, B, I, H, p(d_in), *(p(grads[n]) for n in PARAMS), p(ws), sp),
               "blvm_lstm_bidir_bwd")  # fmt: skip
    torch.cuda.synchronize()
    _hip.check_async("blvm_lstm_bidir_fwd/_bwd")
    return out, d_in, grads


def test_results_do_not_depend_on_what_the_buffers_held():
    case = (7, 17, 24, 128, "unsorted")
    inp, ref = bidir_case(*case)
    _hip.take_async_errors()
    runs = {kind: _raw_run(case, kind) for kind in ("zeros", "nan", "noise")}
    ck = Checks(f"lstm bidir raw ABI {_id(case)}")
    for kind, (out, d_in, grads) in runs.items():
        for name, t in [("out", out), ("d_in", d_in)] + [("d_" + n, grads[n]) for n in PARAMS]:
            ck.exact(f"[{kind}] {name} is finite", torch.isfinite(t).all())
        ck.exact(f"[{kind}] out has the bits of the zero-prefilled run", torch.equal(out.view(torch.int32), runs["zeros"][0].view(torch.int32)))
        ck.close(f"[{kind}] out", out, ref["out"], BAR_VALUE, row_dim=1)
        ck.close(f"[{kind}] d_in", d_in, ref["d_x"], BAR_GRAD, row_dim=1)
        for n in PARAMS:
            ck.close(f"[{kind}] d_{n}", grads[n], ref["d_" + n], BAR_GRAD)
        check_padding(ck, out, inp["lens"], case[3])
    ck.done()


# ----------------------------------------------------------------------------------------------------------------------
# 4. refusal and fallback
# ----------------------------------------------------------------------------------------------------------------------


def _refused_shapes():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    shapes = [(4, 113, 5, 384, "2 * 24 * 8 = 384 workgroups"), (5, 3, 5, 64, "H = 64"), (3, 3, 5, 128, "T = 3")]
    assert 2 * 24 * 8 > cus, f"a device of {cus} CUs holds the 384 workgroups this case needs refused"
    rt = cus // 48 + 1  # the first row-tile count whose 2 * 24 * rt workgroups exceed the CUs
    if rt <= 8:
        shapes.append((4, 16 * (rt - 1) + 1, 5, 384, f"2 * 24 * {rt} workgroups on {cus} CUs"))
    return shapes


def test_shapes_outside_the_one_launch_form_are_refused_untouched():
    lib = _hip.load()
    p, sp = _hip.ptr, _hip.stream_ptr()
    for T_, B, I, H, why in _refused_shapes():
        f32 = dict(device=DEV, dtype=torch.float32)
        par = {n: torch.zeros(s, **f32) for n, s in zip(PARAMS, ((4 * H, I), (4 * H, H), (4 * H,), (4 * H,)) * 2)}
        x, d_out = torch.zeros(T_, B, I, **f32), torch.zeros(T_, B, 2 * H, **f32)
        lens_dev = unsorted_lens(T_, B).to(DEV, torch.int32)
        out, d_in = _prefilled(T_ * B * 2 * H, "nan", 0), _prefilled(T_ * B * I, "nan", 0)
        reserve = _prefilled(lib.blvm_lstm_bidir_reserve_floats(T_, B, H), "nan", 0)
        ws = _prefilled(lib.blvm_lstm_bidir_bwd_workspace_floats(T_, B, H), "nan", 0)
        grads = {n: torch.zeros_like(par[n]) for n in PARAMS}
        rnn_before, before = path_counts(), bidir_counts()
        rc_f = lib.blvm_lstm_bidir_fwd(*(p(par[n]) for n in PARAMS), p(x), p(lens_dev), T_, B, I, H, p(out), p(reserve), sp)
        rc_b = lib.blvm_lstm_bidir_bwd(p(par["Wih_f"]), p(par["Whh_f"]), p(par["Wih_r"]), p(par["Whh_r"]), p(x), p(lens_dev), p(reserve),
                                       p(d_out), T_, B, I, H, p(d_in), *(p(grads[n]) for n in PARAMS), p(ws), sp)  # fmt: skip
        torch.cuda.synchronize()
        assert (rc_f, rc_b) == (NOT_APPLICABLE, NOT_APPLICABLE), f"{why}: return codes {(rc_f, rc_b)}"
        assert bidir_counts() == before and path_counts() == rnn_before, why
        for name, t in (("out", out), ("d_in", d_in), ("reserve", reserve), ("workspace", ws)):
            assert bool((t.view(torch.int32) == QNAN).all()), f"{why}: {name} was written"
        assert all(not bool(g.any()) for g in grads.values()), f"{why}: a weight gradient was written"
        # and through ops: None, nothing launched
        assert ops.lstm_bidir_sequence(x, lens_dev, [par[n] for n in PARAMS[:4]], [par[n] for n in PARAMS[4:]]) is None, why
        assert bidir_counts() == before and path_counts() == rnn_before, why


def test_block_outside_the_form_takes_the_two_call_path():
    T_, B, I, H = 6, 3, 5, 64
    torch.manual_seed(11)
    block = LSTMBlock(I, H, num_layers=1, bidirectional=True, dropout_prob=0.0).eval()
    lstm = block.lstm_layers[0]
    names = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
    p64 = {n: getattr(lstm, m + sfx).detach().double() for n, (m, sfx) in zip(PARAMS, [(m, s) for s in ("", "_reverse") for m in names])}
    x = torch.randn(T_, B, I, generator=torch.Generator().manual_seed(12))
    lens = unsorted_lens(T_, B)
    want = bidir_ref(x.double(), lens, p64)
    block.to(DEV)
    rnn_before, before = path_counts(), bidir_counts()
    _hip.take_async_errors()
    with torch.no_grad():
        got, sl = block(x.to(DEV), lens)
    delta = [a - b for a, b in zip(path_counts(), rnn_before)]
    assert bidir_counts() == before and sum(delta[:3]) == 2 and sum(delta[3:]) == 0, (bidir_counts(), delta)
    assert torch.equal(sl, lens)
    ck = Checks(f"LSTMBlock T{T_}-B{B}-I{I}-H{H} two-call path")
    ck.close("out", got, want, BAR_VALUE, row_dim=1)
    check_padding(ck, got, lens, H)
    ck.done()


# ----------------------------------------------------------------------------------------------------------------------
# 5. through the block
# ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train_temporal_masks"])
@pytest.mark.parametrize("sumd", [False, True], ids=["cat", "sum"])
def test_block_runs_each_layer_as_one_launch(sumd, train):
    """By the rule of tests/test_gpu_lstm_asr.py: the error against the float64 torch composition (tests/asr_reference.py) is at most
    4 times that of the same composition in torch fp32, floors 1e-5 (values) / 2e-5 (gradients)."""
    T_, B, I, H, L, p = 7, 5, 24, 128, 2, 0.3
    gen = torch.Generator().manual_seed(21 + 2 * sumd + train)
    torch.manual_seed(31)
    block = LSTMBlock(I, H, num_layers=L, bidirectional=True, sum_directions=sumd, dropout_prob=p, return_all=True)
    block.train(train)
    width = H if sumd else 2 * H
    assert block.output_size == width
    x = torch.randn(B, I, T_, generator=gen)
    x_sl = torch.tensor([4, 7, 1, 6, 2])  # unsorted, >= 1: packing takes no empty row
    w = torch.randn(T_, B, width, generator=gen)
    scales = [(torch.rand((1, width), generator=gen) > p).float() / (1 - p) for _ in range(L)] if train else None

    refs = {}
    for dtype in (torch.float64, torch.float32):
        ref = TorchASR(3, I, H, L, True, sumd).to(dtype)
        ref.lstm.load_state_dict({k: v.to(dtype) for k, v in block.state_dict().items()}, strict=True)
        _, _, layers = ref(x.to(dtype), x_sl, torch.ones(B, 1, dtype=torch.long), torch.ones(B, dtype=torch.long), scales=scales)
        (layers[-1] * w.to(dtype)).sum().backward()
        refs[dtype] = ([t.detach() for t in layers], {k: q.grad for k, q in ref.lstm.named_parameters()})
    (layers64, grads64), (layers32, grads32) = refs[torch.float64], refs[torch.float32]

    block.to(DEV)
    _hip.take_async_errors()
    rnn_before, before = path_counts(), bidir_counts()
    outs, sl = block(x.permute(2, 0, 1).contiguous().to(DEV), x_sl, dropout_masks=None if scales is None else [s.to(DEV) for s in scales])
    assert bidir_counts() == (before[0] + L, before[1])
    (outs[-1] * w.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert bidir_counts() == (before[0] + L, before[1] + L) and path_counts() == rnn_before
    assert _hip.take_async_errors() == (0, 0)
    assert isinstance(outs, list) and len(outs) == L and torch.equal(sl, x_sl)
    for k, (got, want32, want64) in enumerate(zip(outs, layers32, layers64)):
        assert got.shape == (T_, B, width)
        within(f"layer {k} output", got.detach(), want32, want64, 1e-5)
        for b in range(B):
            assert float(got.detach()[int(x_sl[b]):, b].abs().max() if int(x_sl[b]) < T_ else 0.0) == 0.0
    for k, q in block.named_parameters():
        within(f"d {k}", q.grad, grads32[k], grads64[k], 2e-5)


def test_counts_reader_matches_the_abi():
    buf = (ctypes.c_ulonglong * 2)()
    assert _hip.load().blvm_lstm_bidir_path_counts(buf) == 0 and tuple(buf) == ops.lstm_bidir_path_counts()
