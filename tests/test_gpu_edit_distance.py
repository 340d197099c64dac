"""`ops.edit_distance` (csrc/editdist.hip) against the host `edit_distance`: exact equality, at the lane, wave and strip edges, with
and without unit tables, the caller-owned-buffer contract, refused rows and the reference limit."""
import pytest
import torch

from blvm import _hip, ops
from blvm.data.token_map import UnitTable, expand_units
from blvm.evaluation.metrics import edit_distance
from edit_cases import TOKEN_MAPS, TOKENIZERS, random_rows, string_counts

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STRIP = ops.EDIT_STRIP_UNITS
# (reference, hypothesis) lengths: empty sides, around 64 and 128 (the wave's width in rows of the skewed walk, and multiples of a
# lane's 8 columns), the strip width in both directions, and hypotheses of several strips
LENGTHS = [(0, 0), (0, 5), (5, 0), (1, 1), (63, 64), (64, 63), (64, 64), (65, 65), (128, 129), (STRIP, STRIP + 1), (STRIP + 1, STRIP),
           (STRIP - 1, STRIP), (3, 2 * STRIP + 88), (130, 2 * STRIP + 18)]  # fmt: skip
FILL = 0x7F7F7F7F


@pytest.fixture(scope="module", autouse=True)
def _require_hip():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert _hip.load().blvm_device_ok() == 1, "libblvm_hip: no gfx950 device visible"


def padded(rows, pad, width=None):
    width = max([len(r) for r in rows] + [1]) if width is None else width
    return torch.tensor([r + [pad] * (width - len(r)) for r in rows], dtype=torch.int32).reshape(len(rows), width)


def run(refs, hyps, table=None, pad=-1):
    """(edits, ref_units) as lists; the hypotheses on the device, the references and lengths from the host."""
    e, n = ops.edit_distance(padded(refs, pad), [len(r) for r in refs], padded(hyps, pad).to(DEV), [len(h) for h in hyps], table=table)
    return e.cpu().tolist(), n.cpu().tolist()


@pytest.mark.parametrize("alphabet", [2, 1000])
def test_lengths_at_the_lane_wave_and_strip_edges(alphabet):
    gen = torch.Generator().manual_seed(alphabet)
    refs = [torch.randint(0, alphabet, (r,), generator=gen).tolist() for r, _ in LENGTHS]
    hyps = [torch.randint(0, alphabet, (h,), generator=gen).tolist() for _, h in LENGTHS]
    edits, ref_units = run(refs, hyps)
    want = [edit_distance(r, h) for r, h in zip(refs, hyps)]
    print(list(zip(LENGTHS, edits, want)))
    assert edits == want and ref_units == [r for r, _ in LENGTHS]


def test_identical_and_disjoint_sequences():
    gen = torch.Generator().manual_seed(3)
    rows = [torch.randint(0, 50, (n,), generator=gen).tolist() for n in (1, 64, 65, STRIP, STRIP + 1, 2 * STRIP + 7)]
    assert run(rows, rows)[0] == [0] * len(rows)
    pairs = [(1, 1), (5, 70), (70, 5), (STRIP + 1, 64), (64, STRIP + 1), (STRIP + 44, STRIP + 44)]
    refs = [torch.randint(0, 50, (r,), generator=gen).tolist() for r, _ in pairs]
    hyps = [torch.randint(50, 100, (h,), generator=gen).tolist() for _, h in pairs]
    assert run(refs, hyps)[0] == [max(p) for p in pairs]


def library_call(ref, ref_len, hyp, hyp_len, edits, ref_units):
    B = hyp.shape[0]
    _hip.check(_hip.load().blvm_edit_distance(ref.data_ptr(), ref_len.data_ptr(), ref.shape[1], hyp.data_ptr(), hyp_len.data_ptr(),
                                              hyp.shape[1], B, 0, 0, None, None, None, 0, edits.data_ptr(), ref_units.data_ptr(), None,
                                              _hip.stream_ptr()), "blvm_edit_distance")  # fmt: skip


def test_a_ragged_batch_ignores_padding_and_prior_buffer_contents():
    gen = torch.Generator().manual_seed(11)
    pairs = [(40, 38), (0, 9), (70, STRIP + 44), (1, 0), (129, 64), (33, 33), (STRIP + 1, 5)]  # B = 7
    refs = [torch.randint(0, 6, (r,), generator=gen).tolist() for r, _ in pairs]
    hyps = [torch.randint(0, 6, (h,), generator=gen).tolist() for _, h in pairs]
    want = [edit_distance(r, h) for r, h in zip(refs, hyps)]
    rl, hl = torch.tensor([r for r, _ in pairs], dtype=torch.int32).to(DEV), torch.tensor([h for _, h in pairs], dtype=torch.int32).to(DEV)
    results = []
    for pad, fill in ((-1, 0), (3, 0), (-1, FILL), (-1, FILL)):  # -1 padding | valid symbols as padding | pre-filled outputs, twice
        ref, hyp = padded(refs, pad, STRIP + 40).to(DEV), padded(hyps, pad, STRIP + 50).to(DEV)
        edits, ref_units = torch.full((7,), fill, dtype=torch.int32, device=DEV), torch.full((7,), fill, dtype=torch.int32, device=DEV)
        library_call(ref, rl, hyp, hl, edits, ref_units)
        results.append((edits.cpu(), ref_units.cpu()))
    assert results[0][0].tolist() == want and results[0][1].tolist() == [r for r, _ in pairs]
    for edits, ref_units in results[1:]:
        assert torch.equal(edits, results[0][0]) and torch.equal(ref_units, results[0][1])


@pytest.mark.parametrize("kind", list(TOKEN_MAPS))
def test_unit_tables_give_the_string_metrics(kind):
    tm = TOKEN_MAPS[kind]
    tables = tm.unit_tables()
    ref_lens, hyp_lens = [0, 1, 0, 5, 40, 33, 2, 64, 17], [0, 0, 1, 7, 38, 260, 190, 64, 3]  # long rows cross a strip as characters
    refs, hyps = random_rows(tm, ref_lens, 5), random_rows(tm, hyp_lens, 6)
    want = [string_counts(tm, refs, hyps, tok) for tok in TOKENIZERS]
    edits, ref_units = run(refs, hyps, table=list(tables))  # both tables in one launch: [2,B]
    for k in range(2):
        assert list(zip(edits[k], ref_units[k])) == want[k], (kind, TOKENIZERS[k].__name__)
    for k in range(2):  # and each table alone: [B]
        e, n = run(refs, hyps, table=tables[k])
        assert list(zip(e, n)) == want[k]
    # padding made of valid tokens changes nothing
    e, n = run(refs, hyps, table=list(tables), pad=1)
    assert (e, n) == (edits, ref_units)

    # a token outside the map inside a row's length, on either side: that row is -1, its neighbours keep their values
    bad_refs, bad_hyps = [list(r) for r in refs], [list(h) for h in hyps]
    bad_refs[4][7], bad_hyps[6][189], bad_hyps[8][0] = len(tm), -1, 2**31 - 1
    e, n = run(bad_refs, bad_hyps, table=list(tables))
    for k in range(2):
        for b in range(len(refs)):
            assert (e[k][b], n[k][b]) == ((-1, -1) if b in (4, 6, 8) else want[k][b])


def test_a_length_outside_its_row_is_refused_for_that_row():
    refs, hyps = [[1, 2, 3], [4, 5], [6]], [[1, 2], [4, 5, 5], [7]]
    ref, hyp = padded(refs, 0), padded(hyps, 0).to(DEV)
    e, n = ops.edit_distance(ref, [3, 4, 1], hyp, [2, 3, -1])
    assert e.cpu().tolist() == [1, -1, -1] and n.cpu().tolist() == [3, -1, -1]


def test_the_expanded_reference_limit():
    gen = torch.Generator().manual_seed(8)
    limit = ops.EDIT_MAX_REF_UNITS
    ref = torch.randint(0, 3, (1, limit + 1), generator=gen, dtype=torch.int32)
    hyp = torch.randint(0, 3, (1, 5), generator=gen, dtype=torch.int32)
    e, n = ops.edit_distance(ref[:, :limit], [limit], hyp.to(DEV), [5])
    assert e.cpu().tolist() == [edit_distance(ref[0, :limit].tolist(), hyp[0].tolist())] and n.cpu().tolist() == [limit]
    with pytest.raises(_hip.BlvmHipError, match="8193"):
        ops.edit_distance(ref, [limit + 1], hyp.to(DEV), [5])
    # under a table the bound counts every token at the table's longest, and a separator
    table = UnitTable([[1, 2, 3], [4]], separator=0)  # 4 units per token at most: 2048 tokens are 8191, 2049 are 8195
    tokens = torch.randint(0, 2, (1, 2049), generator=gen, dtype=torch.int32)
    e, n = ops.edit_distance(tokens[:, :2048], [2048], hyp.to(DEV) % 2, [5], table=table)
    units = expand_units(tokens[0, :2048], table)
    assert n.cpu().tolist() == [len(units)] and e.cpu().tolist() == [edit_distance(units, expand_units(hyp[0] % 2, table))]
    with pytest.raises(_hip.BlvmHipError):
        ops.edit_distance(tokens, [2049], hyp.to(DEV) % 2, [5], table=table)
