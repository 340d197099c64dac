"""Host side of the device error rates: `TokenMap.unit_tables()` + `expand_units` reproduce the string metrics exactly (the edit
distance between expanded index sequences equals the one between tokenised joined strings, and so does the reference length),
`ErrorRateMetric.from_counts`, and the refusal of CPU tensors.  No GPU."""
import copy

import pytest
import torch

from blvm import _hip, ops
from blvm.data.token_map import TokenMap, UnitTable, expand_units
from blvm.evaluation import ErrorRateMetric
from blvm.evaluation.metrics import DeferredScalars, edit_distance
from edit_cases import TOKEN_MAPS, TOKENIZERS, random_rows, string_counts

REF_LENS = [0, 1, 0, 1, 2, 3, 5, 8, 13, 21, 9, 7]  # empty and single-token rows on either side
HYP_LENS = [0, 0, 1, 1, 3, 2, 5, 9, 11, 17, 0, 30]


@pytest.mark.parametrize("kind", list(TOKEN_MAPS))
def test_expanded_sequences_reproduce_the_string_metrics(kind):
    tm = TOKEN_MAPS[kind]
    tables = tm.unit_tables()
    assert tables is not None and tm.unit_tables() is tables  # built once
    for seed in range(4):
        refs, hyps = random_rows(tm, REF_LENS, 10 * seed), random_rows(tm, HYP_LENS, 10 * seed + 1)
        for table, tokenizer in zip(tables, TOKENIZERS):
            want = string_counts(tm, refs, hyps, tokenizer)
            got = [(edit_distance(expand_units(r, table), expand_units(h, table)), len(expand_units(r, table))) for r, h in zip(refs, hyps)]
            assert got == want, (kind, tokenizer.__name__)


def test_unit_table_layout():
    tm = TOKEN_MAPS["inner_spaces"]  # sorted: "%", "  ", " lead", "a b c", "new york", "trail ", "x", "x y"
    words, chars = tm.unit_tables()
    assert len(words) == len(chars) == len(tm) and words.separator < 0 and chars.separator == ord(" ")
    assert expand_units([tm("  ")], words) == [] and expand_units([tm("  ")], chars) == [32, 32]
    x, xy = expand_units([tm("x")], words), expand_units([tm("x y")], words)
    assert len(x) == 1 and xy[0] == x[0] and len(xy) == 2  # word ids are interned over the whole map
    assert expand_units([tm("x"), tm("%")], chars) == [ord("x"), 32, ord("%")]
    assert chars.max_units == len("new york") and words.max_units == 3
    assert expand_units(torch.tensor([tm("x")]), chars) == [ord("x")]
    with pytest.raises(ValueError):
        expand_units([len(tm)], chars)
    with pytest.raises(ValueError):
        expand_units([-1], words)
    table = UnitTable([[5, 6], [], [7]], separator=9)
    assert table.offsets == [0, 2, 2, 3] and table.units == [5, 6, 7] and expand_units([0, 1, 2], table) == [5, 6, 9, 9, 7]


def test_a_map_with_an_empty_token_has_no_tables():
    assert TokenMap(["", "a", "b"], add_blank=True).unit_tables() is None


def test_from_counts_pools_over_updates_and_mixes_with_strings():
    a = ErrorRateMetric.from_counts((3, 10), name="wer")
    assert a.name == "wer" and a.value == 3 / 10
    a.update(ErrorRateMetric.from_counts((1, 5), name="wer"))
    a.update(ErrorRateMetric.from_counts((0.0, 5.0), name="wer"))
    assert a.value == 4 / 20
    strings = ErrorRateMetric(["the cat sat", "a b"], ["the bat sat down", ""], str.split, name="wer")  # 4 edits over 5 words
    a.update(strings)
    assert a.value == 8 / 25
    strings.update(ErrorRateMetric.from_counts((1, 5), name="wer"))
    assert strings.value == 5 / 10
    assert ErrorRateMetric.from_counts((0, 0)).value != ErrorRateMetric.from_counts((0, 0)).value  # no reference units: NaN
    assert a.get_best([a, strings]) is a


class CountingScalars(DeferredScalars):
    """A DeferredScalars over a host tensor that counts its reads."""

    reads = 0

    def values(self):
        if self._values is None:
            CountingScalars.reads += 1
        return super().values()


def test_from_counts_stays_deferred_until_a_value_is_read():
    CountingScalars.reads = 0
    total = ErrorRateMetric.from_counts((2, 8), name="cer")
    for step in range(3):
        d = CountingScalars(torch.tensor([step + 1, 10, 0], dtype=torch.int32))
        total.update(ErrorRateMetric.from_counts((d[0], d[1]), name="cer", invalid=d[2]))
    assert CountingScalars.reads == 0
    assert total.value == (2 + 1 + 2 + 3) / 38 and CountingScalars.reads == 3
    assert total.value == 8 / 38 and CountingScalars.reads == 3


def test_from_counts_deepcopy():
    d = DeferredScalars(torch.tensor([4, 16], dtype=torch.int32))
    m = ErrorRateMetric.from_counts((d[0], d[1]), name="cer", tags={"x"})
    c, c2 = m.copy(), copy.deepcopy(m)
    m.update(ErrorRateMetric.from_counts((4, 0)))
    assert c.value == c2.value == 4 / 16 and m.value == 8 / 16 and c.name == "cer" and c.tags == {"x"}


def test_an_invalid_row_raises_when_the_metric_is_resolved():
    for counts, invalid in (((-1, 12), None), ((3, -1), None), ((3, 12), 2)):
        d = DeferredScalars(torch.tensor(list(counts) + [invalid or 0], dtype=torch.int32))
        m = ErrorRateMetric.from_counts((d[0], d[1]), name="my_wer", invalid=d[2] if invalid else None)  # building it is fine
        good = ErrorRateMetric.from_counts((1, 2), name="my_wer")
        good.update(m)
        for metric in (m, good):
            with pytest.raises(ValueError, match="my_wer"):
                metric.value


def test_cpu_tensors_are_refused():
    words, chars = TOKEN_MAPS["multi_character"].unit_tables()
    ref, hyp = torch.ones(2, 3, dtype=torch.int32), torch.ones(2, 4, dtype=torch.int32)
    with pytest.raises(_hip.BlvmHipError):
        ops.edit_distance(ref, [3, 3], hyp, [4, 4])
    with pytest.raises(_hip.BlvmHipError):
        ops.edit_distance(ref, [3, 3], hyp, [4, 4], table=chars)
    with pytest.raises(_hip.BlvmHipError):
        ops.ctc_error_counts(torch.zeros(4, 2, 8), [4, 4], ref, [3, 3], (words, chars))
    with pytest.raises(_hip.BlvmHipError):
        ops.ctc_greedy_device(torch.zeros(4, 2, 8), [4, 4])


def test_the_reference_limit_is_judged_on_the_host():
    words, chars = TOKEN_MAPS["inner_spaces"].unit_tables()  # the longest token has 8 characters
    assert ops.edit_distance_fits(8192) and not ops.edit_distance_fits(8193)
    assert ops.edit_distance_fits(910, (words, chars)) and not ops.edit_distance_fits(911, (words, chars))  # 9 * 910 - 1 = 8189
