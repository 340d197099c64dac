"""`ops.ctc_error_counts` and `ops.ctc_greedy_device` against the host composition `greedy_ctc` -> `TokenMap.decode_batch` ->
`ErrorRateMetric`, and `SimpleLSTMASR`'s device error rates: exact equality throughout (the counts are integers)."""
from types import SimpleNamespace

import pytest
import torch

import blvm.evaluation.metrics as metrics_module
from blvm import _hip, ops
from blvm.data.token_map import TokenMap, char_tokenizer, word_tokenizer
from blvm.evaluation import ErrorRateMetric
from blvm.models import SimpleLSTMASR
from blvm.utils.decoding import greedy_ctc
from edit_cases import string_counts

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BLANK_FIRST = TokenMap(["aa", "b", "ch", "d", "eh", "f"], add_blank=True)  # C = 7
# C = 40, every token sorts before "%": the blank is the LAST index; every fifth token holds two words
BLANK_LAST = TokenMap([f"!{i} x" if i % 5 == 0 else f"!{i}" for i in range(39)] + ["%"])
CASES = {
    # rows: a plain one | a shorter one | no frames at all | all frames blank | an empty target
    "blank_first": dict(tm=BLANK_FIRST, T=20, input_lens=[20, 13, 0, 17, 9], target_lens=[4, 3, 2, 3, 0], all_blank=3),
    # rows: a plain one | no frames and an empty target | all frames blank
    "blank_last": dict(tm=BLANK_LAST, T=70, input_lens=[70, 0, 41], target_lens=[6, 0, 5], all_blank=2),
}


@pytest.fixture(scope="module", autouse=True)
def _require_hip():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert _hip.load().blvm_device_ok() == 1, "libblvm_hip: no gfx950 device visible"


def make(name):
    c = CASES[name]
    tm, T, B = c["tm"], c["T"], len(c["input_lens"])
    blank = tm("%")
    gen = torch.Generator().manual_seed(len(name))
    logits = torch.randn(T, B, len(tm), generator=gen)
    logits[:, c["all_blank"], blank] += 100.0
    labels = [i for i in range(len(tm)) if i != blank]
    y = torch.tensor(labels)[torch.randint(0, len(labels), (B, max(c["target_lens"])), generator=gen)]
    return SimpleNamespace(tm=tm, blank=blank, logits=logits, input_lens=torch.tensor(c["input_lens"]), y=y,
                           y_sl=torch.tensor(c["target_lens"]))  # fmt: skip


def host_counts(tm, hyps_raw, y, y_sl):
    """[(sum of edits, sum of reference lengths)] for (words, characters) by the string path, and the per-row counts."""
    refs = [row[:n] for row, n in zip(y.tolist(), y_sl.tolist())]
    rows = [string_counts(tm, refs, hyps_raw, tok) for tok in (word_tokenizer, char_tokenizer)]
    return [[sum(e for e, _ in r), sum(n for _, n in r)] for r in rows], rows


@pytest.mark.parametrize("name", list(CASES))
def test_error_counts_equal_the_host_composition(name):
    c = make(name)
    assert c.blank == (0 if name == "blank_first" else len(c.tm) - 1)
    hyps_raw = greedy_ctc(c.logits, c.input_lens, blank=c.blank)
    assert hyps_raw[CASES[name]["all_blank"]] == [] and any(len(h) > 3 for h in hyps_raw)
    want, _ = host_counts(c.tm, hyps_raw, c.y, c.y_sl)
    # the same sums from the metric class itself
    hyps, refs = c.tm.decode_batch(hyps_raw, [len(h) for h in hyps_raw], " "), c.tm.decode_batch(c.y, c.y_sl, " ")
    for k, tok in enumerate((word_tokenizer, char_tokenizer)):
        m = ErrorRateMetric(refs, hyps, tok)
        assert [m._edits, m._len] == want[k]

    counts, invalid = ops.ctc_error_counts(c.logits.to(DEV), c.input_lens, c.y, c.y_sl, c.tm.unit_tables(), blank=c.blank)
    assert counts.dtype == torch.int32 and counts.is_cuda and tuple(counts.shape) == (2, 2) and tuple(invalid.shape) == (2,)
    print(name, counts.cpu().tolist(), want)
    assert counts.cpu().tolist() == want and invalid.cpu().tolist() == [0, 0]
    # device lengths and device targets give the same
    again, _ = ops.ctc_error_counts(c.logits.to(DEV), c.input_lens.to(DEV, torch.int32), c.y.to(DEV), c.y_sl.to(DEV, torch.int32),
                                    c.tm.unit_tables(), blank=c.blank)  # fmt: skip
    assert torch.equal(again, counts)


@pytest.mark.parametrize("name", list(CASES))
def test_greedy_device_equals_greedy(name):
    c = make(name)
    T, B = c.logits.shape[:2]
    hyp, hyp_lens = ops.ctc_greedy_device(c.logits.to(DEV), c.input_lens, blank=c.blank)
    assert hyp.dtype == hyp_lens.dtype == torch.int32 and tuple(hyp.shape) == (B, T) and tuple(hyp_lens.shape) == (B,)
    lists = ops.ctc_greedy(c.logits.to(DEV), c.input_lens, blank=c.blank)
    assert lists == greedy_ctc(c.logits, c.input_lens, blank=c.blank)
    hyp, hyp_lens = hyp.cpu().tolist(), hyp_lens.cpu().tolist()
    assert hyp_lens == [len(r) for r in lists]
    assert all(row[:n] == want and set(row[n:]) <= {-1} for row, n, want in zip(hyp, hyp_lens, lists))


def test_a_label_outside_the_map_is_counted_as_refused():
    c = make("blank_first")
    y = c.y.clone()
    y[1, 1] = len(c.tm)
    hyps_raw = greedy_ctc(c.logits, c.input_lens, blank=c.blank)
    _, rows = host_counts(c.tm, hyps_raw, c.y, c.y_sl)
    want = [[sum(e for b, (e, _) in enumerate(r) if b != 1), sum(n for b, (_, n) in enumerate(r) if b != 1)] for r in rows]
    counts, invalid = ops.ctc_error_counts(c.logits.to(DEV), c.input_lens, y, c.y_sl, c.tm.unit_tables(), blank=c.blank)
    assert counts.cpu().tolist() == want and invalid.cpu().tolist() == [1, 1]


def refuse(*a, **k):
    raise AssertionError("the host path was taken")


def model_inputs(tm, seed):
    gen = torch.Generator().manual_seed(seed)
    x, x_sl = torch.randn(4, 5, 24, generator=gen), torch.tensor([24, 17, 9, 6])  # enough frames for each row's labels
    y, y_sl = torch.randint(1, len(tm), (4, 5), generator=gen), torch.tensor([5, 3, 0, 2])
    return x, x_sl, y, y_sl


def host_values(model, tm, out, x_sl, y, y_sl):
    raw = greedy_ctc(out.logits.detach().transpose(0, 1).cpu(), x_sl, blank=model.blank_index)
    sums, _ = host_counts(tm, raw, y, y_sl)
    return raw, [s[0] / s[1] for s in sums]


def test_the_model_computes_its_error_rates_without_the_host_path(monkeypatch):
    tm = BLANK_FIRST
    torch.manual_seed(5)
    model = SimpleLSTMASR(tm, input_size=5, hidden_size=16, num_layers=1, bidirectional=True).to(DEV)
    x, x_sl, y, y_sl = model_inputs(tm, 1)
    monkeypatch.setattr(metrics_module, "edit_distance", refuse)
    monkeypatch.setattr(ops, "ctc_greedy", refuse)
    loss, metrics, out = model(x.to(DEV), x_sl, y, y_sl)
    loss.backward()
    values = {m.name: m.value for m in metrics}
    raw, (wer, cer) = host_values(model, tm, out, x_sl, y, y_sl)  # string_counts holds the real edit_distance
    assert values["wer"] == wer and values["cer"] == cer and values["loss"] == float(loss.detach())
    assert torch.equal(torch.as_tensor(out.sl), x_sl)
    monkeypatch.undo()
    assert out.hyps == tm.decode_batch(raw, [len(h) for h in raw], " ") and out.refs == tm.decode_batch(y, y_sl, " ")
    assert values["wer"] == ErrorRateMetric(out.refs, out.hyps, word_tokenizer).value
    assert values["cer"] == ErrorRateMetric(out.refs, out.hyps, char_tokenizer).value


def test_a_map_with_an_empty_token_takes_the_host_path(monkeypatch):
    tm = TokenMap(["", "a", "b", "c c"], add_blank=True)  # sorted: "%", "", "a", "b", "c c"
    assert tm.unit_tables() is None
    torch.manual_seed(6)
    model = SimpleLSTMASR(tm, input_size=5, hidden_size=16, num_layers=1, bidirectional=False).to(DEV)
    x, x_sl, y, y_sl = model_inputs(tm, 2)
    calls, greedy = [], ops.ctc_greedy
    monkeypatch.setattr(ops, "ctc_greedy", lambda *a, **k: calls.append(1) or greedy(*a, **k))
    loss, metrics, out = model(x.to(DEV), x_sl, y, y_sl)
    assert calls == [1]
    raw = greedy_ctc(out.logits.detach().transpose(0, 1).cpu(), x_sl, blank=model.blank_index)
    hyps, refs = tm.decode_batch(raw, [len(h) for h in raw], " "), tm.decode_batch(y, y_sl, " ")
    values = {m.name: m.value for m in metrics}
    assert out.hyps == hyps and out.refs == refs
    assert values["wer"] == ErrorRateMetric(refs, hyps, word_tokenizer).value
    assert values["cer"] == ErrorRateMetric(refs, hyps, char_tokenizer).value
