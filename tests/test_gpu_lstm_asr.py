"""SimpleLSTMASR (LSTMBlock on K4, Linear on K6, CTC loss and greedy decode on K9) against the float64 torch composition with copied
weights (tests/asr_reference.py).  The bound is that of tests/test_gpu_ctc.py: the kernel path's error against float64 is at most
4 times the error of the SAME composition evaluated by torch in fp32 on the CPU, never below the K4 bars (1e-5 values, 2e-5
gradients); relative L2 per tensor, and per batch row for the logits.  Figures are printed before they are asserted."""
import pytest
import torch

from asr_reference import TorchASR
from blvm import _hip
from blvm.data.token_map import TokenMap, char_tokenizer, word_tokenizer
from blvm.evaluation import ErrorRateMetric
from blvm.models import SimpleLSTMASR
from blvm.modules.lstm_block import LSTMBlock
from blvm.utils.decoding import greedy_ctc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLOOR_VALUE, FLOOR_GRAD, TIMES = 1e-5, 2e-5, 4.0
TOKENS = ["aa", "b", "ch", "d", "eh", "f"]  # 7 classes with the blank


@pytest.fixture(scope="module", autouse=True)
def _require_hip():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert _hip.load().blvm_device_ok() == 1, "libblvm_hip: no gfx950 device visible"


def rel(a, r):
    return float((a.double().cpu() - r.double()).norm() / r.double().norm())


def within(name, got, got32, ref, floor):
    e, e32 = rel(got, ref), rel(got32, ref)
    bar = max(TIMES * e32, floor)
    print(f"{name}: kernel {e:.3e}  torch fp32 {e32:.3e}  bar {bar:.3e}")
    assert e <= bar, f"{name}: relative error {e:.3e} above {bar:.3e} (torch fp32: {e32:.3e})"


def mask_scales(kind, widths, T, B, p, gen):
    if kind is None:
        return None
    return [(torch.rand((1, w) if kind == "temporal" else (T, B, w), generator=gen) > p).float() / (1 - p) for w in widths]


CONFIGS = {
    "uni_1layer": dict(hidden=16, inp=5, layers=1, bi=False, sumd=False, T=20, sl=[20, 13, 7]),
    "bi_2layer_cat": dict(hidden=16, inp=24, layers=2, bi=True, sumd=False, T=17, sl=[17, 12, 5]),
    "bi_2layer_sum": dict(hidden=32, inp=5, layers=2, bi=True, sumd=True, T=19, sl=[19, 11, 8]),
    "train_temporal_dropout": dict(hidden=16, inp=5, layers=2, bi=True, sumd=False, T=15, sl=[15, 9, 6], masks="temporal", train=True),
    "train_elementwise_dropout": dict(hidden=16, inp=5, layers=2, bi=True, sumd=False, T=15, sl=[15, 9, 6], masks="element", train=True, temporal=False),
    "eval_ignores_dropout": dict(hidden=16, inp=5, layers=1, bi=True, sumd=False, T=15, sl=[15, 9, 6], p=0.5),
    "unsorted_lengths": dict(hidden=32, inp=24, layers=2, bi=True, sumd=False, T=18, sl=[6, 18, 11]),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_against_the_float64_composition(name):
    c = CONFIGS[name]
    H, I, T, sl, B = c["hidden"], c["inp"], c["T"], c["sl"], 3
    p = c.get("p", 0.3 if c.get("masks") else 0.0)
    gen = torch.Generator().manual_seed(len(name))
    tm = TokenMap(TOKENS, add_blank=True)
    model = SimpleLSTMASR(tm, I, H, num_layers=c["layers"], bidirectional=c["bi"], sum_directions=c["sumd"], dropout_prob=p,
                          temporal_dropout=c.get("temporal", True))  # fmt: skip
    model.train(bool(c.get("train")))
    x = torch.randn(B, I, T, generator=gen)
    x_sl = torch.tensor(sl)
    y_sl = torch.tensor([min(4, n // 2) for n in sl])  # feasible whatever the repeats
    y = torch.randint(1, len(tm), (B, 4), generator=gen)
    width = H * (2 if c["bi"] and not c["sumd"] else 1)
    scales = mask_scales(c.get("masks"), [width] * c["layers"], T, B, p, gen)

    refs = {}
    for dtype in (torch.float64, torch.float32):
        ref = TorchASR(len(tm), I, H, c["layers"], c["bi"], c["sumd"]).to(dtype)
        ref.load_state_dict({k: v.to(dtype) for k, v in model.state_dict().items()}, strict=True)
        loss, logits, _ = ref(x.to(dtype), x_sl, y, y_sl, blank=model.blank_index, scales=scales)
        loss.backward()
        refs[dtype] = (loss.detach(), logits.detach(), {k: q.grad for k, q in ref.named_parameters()})
    (loss64, logits64, grads64), (loss32, logits32, grads32) = refs[torch.float64], refs[torch.float32]

    model.to(DEV)
    loss, metrics, out = model(x.to(DEV), x_sl, y, y_sl, dropout_masks=None if scales is None else [s.to(DEV) for s in scales])
    loss.backward()
    within("loss", loss.detach(), loss32, loss64, FLOOR_VALUE)
    assert out.logits.shape == logits64.shape
    within("logits", out.logits.detach(), logits32, logits64, FLOOR_VALUE)
    for b in range(B):
        within(f"logits[row {b}]", out.logits.detach()[b], logits32[b], logits64[b], FLOOR_VALUE)
    for k, q in model.named_parameters():
        within(f"d {k}", q.grad, grads32[k], grads64[k], FLOOR_GRAD)

    raw = greedy_ctc(logits64.transpose(0, 1), x_sl, blank=model.blank_index)
    want_hyps = tm.decode_batch(raw, [len(h) for h in raw], " ")
    want_refs = tm.decode_batch(y, y_sl, " ")
    assert out.hyps == want_hyps and out.refs == want_refs
    assert torch.equal(torch.as_tensor(out.sl), x_sl)
    values = {m.name: m.value for m in metrics}
    assert values["wer"] == ErrorRateMetric(want_refs, want_hyps, word_tokenizer).value
    assert values["cer"] == ErrorRateMetric(want_refs, want_hyps, char_tokenizer).value
    assert abs(values["loss"] - float(loss64)) <= 1e-4 * abs(float(loss64))


def test_return_all_gives_every_layer():
    gen = torch.Generator().manual_seed(9)
    block = LSTMBlock(5, 16, num_layers=2, bidirectional=True, sum_directions=False, dropout_prob=0.0, return_all=True).eval()
    ref = TorchASR(3, 5, 16, 2, True, False).double()
    ref.lstm.load_state_dict({k: v.double() for k, v in block.state_dict().items()}, strict=True)
    x, x_sl = torch.randn(2, 5, 11, generator=gen), torch.tensor([7, 11])
    _, _, layers = ref(x.double(), x_sl, torch.ones(2, 1, dtype=torch.long), torch.tensor([1, 1]))
    block.to(DEV)
    outs, sl = block(x.permute(2, 0, 1).contiguous().to(DEV), x_sl)
    assert isinstance(outs, list) and len(outs) == 2 and torch.equal(sl, x_sl)
    for got, want in zip(outs, layers):
        assert got.shape == want.shape and rel(got.detach(), want.detach()) <= FLOOR_VALUE


def test_rows_of_length_zero_are_accepted():
    block = LSTMBlock(5, 16, num_layers=1, bidirectional=True, dropout_prob=0.0).eval().to(DEV)
    x = torch.randn(6, 3, 5, generator=torch.Generator().manual_seed(1)).to(DEV)
    out = block(x, torch.tensor([6, 0, 3]))[0].detach()
    assert out.shape == (6, 3, 32) and float(out[:, 1].abs().max()) == 0.0 and float(out[3:, 2].abs().max()) == 0.0
    assert bool(torch.isfinite(out).all()) and float(out[:, 0].abs().max()) > 0.0
