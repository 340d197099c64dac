"""The device greedy CTC decode (`ops.ctc_greedy`, csrc/ctc.hip) must equal the host `blvm.utils.decoding.greedy_ctc` on the same
logits: arg-max per frame with the lowest index winning a tie, repeats collapsed, blanks dropped, only the first input_lens[b] frames."""
import pytest
import torch

from blvm import _hip, ops
from blvm.utils.decoding import greedy_ctc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _require_hip():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert _hip.load().blvm_device_ok() == 1, "libblvm_hip: no gfx950 device visible"


@pytest.mark.parametrize("T,B,C,lens,blank", [(1, 1, 5, [1], 0), (70, 2, 7, [70, 70], 0), (70, 4, 130, [70, 33, 1, 0], 129), (150, 4, 3, [150, 64, 65, 128], 1)],
                         ids=["T1", "T70", "ragged_B4", "chunk_edges"])  # fmt: skip
def test_matches_the_host_decode(T, B, C, lens, blank):
    logits = torch.randn(T, B, C, generator=torch.Generator().manual_seed(T + C))
    want = greedy_ctc(logits, torch.tensor(lens), blank=blank)
    got = ops.ctc_greedy(logits.to(DEV), torch.tensor(lens), blank=blank)
    assert got == want


def frames(labels, C, tie_with=None):
    """[T,1,C] logits whose arg-max per frame is `labels`; tie_with[t]: a HIGHER index given exactly the same value at frame t."""
    x = torch.zeros(len(labels), 1, C)
    for t, l in enumerate(labels):
        x[t, 0, l] = 2.0
        if tie_with and tie_with.get(t) is not None:
            x[t, 0, tie_with[t]] = 2.0
    return x


def test_crafted_cases():
    C = 70  # ties across the two halves of a row that is wider than a wavefront
    rows = [
        (frames([1, 1, 0, 1, 1, 2, 2, 0, 0, 2], C), [1, 1, 2, 2]),  # runs of repeats split by a blank survive as two labels
        (frames([0] * 10, C), []),  # all blank
        (frames([3, 3, 0, 5, 5, 5, 0, 0, 3, 1], C, tie_with={0: 69, 1: 4, 3: 66, 9: 65}), [3, 5, 3, 1]),  # exact ties: the lowest index wins
        (torch.zeros(10, 1, C), []),  # every class ties: index 0, the blank
    ]
    logits = torch.cat([r[0] for r in rows], dim=1)
    lens = torch.tensor([10, 10, 10, 10])
    want = greedy_ctc(logits, lens, blank=0)
    assert want == [r[1] for r in rows]
    assert ops.ctc_greedy(logits.to(DEV), lens, blank=0) == want
    # the same frames cut short: only the first input_lens[b] frames count
    lens = torch.tensor([5, 0, 4, 1])
    assert ops.ctc_greedy(logits.to(DEV), lens, blank=0) == greedy_ctc(logits, lens, blank=0) == [[1, 1], [], [3, 5], []]


def test_c_abi_pads_with_minus_one_whatever_the_buffers_held():
    logits = frames([1, 1, 0, 2], 5).to(DEV)
    lib = _hip.load()
    il = torch.tensor([3], device=DEV, dtype=torch.int32)
    outs = []
    for fill in (0, 12345):
        hyp = torch.full((1, 4), fill, device=DEV, dtype=torch.int32)
        n = torch.full((1,), fill, device=DEV, dtype=torch.int32)
        _hip.check(lib.blvm_ctc_greedy(_hip.ptr(logits), _hip.ptr(il), 4, 1, 5, 0, _hip.ptr(hyp), _hip.ptr(n), _hip.stream_ptr()), "blvm_ctc_greedy")
        outs.append((hyp.cpu().tolist(), n.cpu().tolist()))
    assert outs[0] == outs[1] == ([[1, -1, -1, -1]], [1])
