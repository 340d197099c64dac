"""Host side of the ASR probe: state_dict compatibility of SimpleLSTMASR with the stock torch composition, the host greedy CTC
decode, the error-rate metric, the token map, the refusal of CPU tensors and the experiment's argument parser.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from asr_reference import TorchASR
from blvm import _hip, ops
from blvm.data.token_map import BLANK_TOKEN, TokenMap, char_tokenizer, word_tokenizer
from blvm.evaluation import ErrorRateMetric
from blvm.evaluation.metrics import edit_distance
from blvm.models import SimpleLSTMASR
from blvm.modules.lstm_block import LSTMBlock
from blvm.utils.decoding import greedy_ctc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("layers,bi,sumd", [(1, False, False), (2, True, False), (2, True, True)])
def test_state_dict_round_trip_with_the_torch_composition(layers, bi, sumd):
    tm = TokenMap(["a", "b", "c"], add_blank=True)
    model = SimpleLSTMASR(tm, input_size=5, hidden_size=16, num_layers=layers, bidirectional=bi, sum_directions=sumd)
    ref = TorchASR(len(tm), 5, 16, layers, bi, sumd)
    sd = model.state_dict()
    assert list(sd) == list(ref.state_dict())
    assert "lstm.lstm_layers.0.weight_ih_l0" in sd and ("lstm.lstm_layers.0.weight_hh_l0_reverse" in sd) == bi
    width = 16 * (2 if bi and not sumd else 1)
    assert tuple(sd["output.weight"].shape) == (4, width)
    if layers > 1:
        assert tuple(sd["lstm.lstm_layers.1.weight_ih_l0"].shape) == (64, width)
    ref.load_state_dict(sd, strict=True)
    model.load_state_dict({k: v + 1 for k, v in ref.state_dict().items()}, strict=True)
    assert all(torch.equal(model.state_dict()[k], ref.state_dict()[k] + 1) for k in sd)


def test_checkpoint_round_trip(tmp_path):
    from blvm.models import load_model

    tm = TokenMap(["sh", "aa", "b"], add_blank=True)
    model = SimpleLSTMASR(tm, input_size=5, hidden_size=16, num_layers=2, bidirectional=True, dropout_prob=0.25)
    model.save(str(tmp_path))
    again = load_model(str(tmp_path))
    assert isinstance(again, SimpleLSTMASR) and again.token_map.tokens == tm.tokens and again.blank_index == 0
    assert (again.num_layers, again.bidirectional, again.dropout_prob) == (2, True, 0.25)
    assert all(torch.equal(v, again.state_dict()[k]) for k, v in model.state_dict().items())


def test_lstm_block_arguments():
    with pytest.raises(ValueError):
        LSTMBlock(4, 16, bidirectional=False, sum_directions=True)
    block = LSTMBlock(4, 16)
    assert (block.num_layers, block.bidirectional, block.sum_directions, block.p, block.temporal_dropout, block.return_all) == (
        1, True, False, 0.40, True, False)  # fmt: skip


def test_greedy_ctc_on_hand_made_cases():
    def onehot(labels, C=4):
        return np.eye(C, dtype=np.float32)[np.asarray(labels)]

    logits = np.stack([onehot([1, 1, 0, 1, 2, 2, 0, 0]), onehot([0, 0, 0, 0, 0, 0, 0, 0]), onehot([3, 3, 3, 0, 3, 1, 1, 2])], axis=1)  # [T,B,C]
    assert greedy_ctc(logits, torch.tensor([8, 8, 8])) == [[1, 1, 2], [], [3, 3, 1, 2]]
    assert greedy_ctc(torch.from_numpy(logits), torch.tensor([3, 0, 5])) == [[1], [], [3, 3]]
    assert greedy_ctc(logits, torch.tensor([8, 8, 8]), blank=3) == [[1, 0, 1, 2, 0], [0], [0, 1, 2]]
    ties = np.zeros((2, 1, 4), dtype=np.float32)  # the lowest index wins a tie: index 0, the blank
    assert greedy_ctc(ties, torch.tensor([2])) == [[]]
    ties[:, 0, 2:] = 1.0
    assert greedy_ctc(ties, torch.tensor([2])) == [[2]]


def test_edit_distance_and_error_rate():
    assert edit_distance("kitten", "sitting") == 3
    assert edit_distance([], ["a", "b"]) == 2 and edit_distance(["a", "b"], []) == 2 and edit_distance([], []) == 0
    assert edit_distance(["a", "b", "c"], ["a", "c"]) == 1 and edit_distance(["a", "b"], ["b", "a"]) == 2
    refs, hyps = ["the cat sat", "a b"], ["the bat sat down", ""]
    wer = ErrorRateMetric(refs, hyps, word_tokenizer, name="wer")  # (1 substitution + 1 insertion) + 2 deletions over 3 + 2 words
    assert wer.name == "wer" and wer.value == 4 / 5
    cer = ErrorRateMetric(refs, hyps, char_tokenizer, name="cer")  # "the cat sat" -> "the bat sat down": 1 + 5; "a b" -> "": 3
    assert cer.value == 9 / 14
    other = ErrorRateMetric(["x y z w v"], ["x y z w v"], word_tokenizer, name="wer")
    wer.update(other)
    assert wer.value == 4 / 10
    assert wer.get_best([wer, other]) is other


def test_token_map_order_and_blank():
    tm = TokenMap(["sh", "aa", "b"], add_blank=True)
    assert tm.tokens == [BLANK_TOKEN, "aa", "b", "sh"] and len(tm) == 4 and tm.token2index[BLANK_TOKEN] == 0
    assert tm.encode(["b", "sh", "aa"]) == [2, 3, 1]
    assert tm.decode([3, 1]) == ["sh", "aa"] and tm.decode(torch.tensor([3, 1]), " ") == "sh aa"
    assert tm.decode_batch(torch.tensor([[2, 3, 0], [1, 0, 0]]), torch.tensor([2, 1]), " ") == ["b sh", "aa"]
    assert tm.decode_batch([[2], []], [1, 0], " ") == ["b", ""]
    assert len(TokenMap(["x"])) == 1
    with pytest.raises(KeyError):
        tm.encode(["zz"])


def test_labelled_dataset_plumbing(tmp_path):
    """A source CSV with per-example [T,D] arrays and label files -> ((x [B,D,T], x_sl), (y [B,L], y_sl)), longest first."""
    from blvm.data.base_dataset import BaseDataset
    from blvm.data.batchers import DynamicTensorBatcher, TextBatcher
    from blvm.data.loaders import NumpyLoader, TextLoader
    from blvm.data.transforms import EncodeInteger
    from blvm.modules.convenience import Permute

    tm = TokenMap(["aa", "b", "sh"], add_blank=True)
    feats = {"u1": np.arange(12, dtype=np.float64).reshape(4, 3), "u2": np.ones((6, 3))}
    texts = {"u1": "b aa\n", "u2": "sh\nsh b\n"}
    for k in feats:
        np.save(tmp_path / f"{k}.run-z0-n1.npy", feats[k])
        (tmp_path / f"{k}.PHN").write_text(texts[k])
    (tmp_path / "train.csv").write_text("filename,length.wav.samples\nu1,400\nu2,600\n")
    ds = BaseDataset(str(tmp_path / "train.csv"), [(NumpyLoader("run-z0-n1.npy", dtype=torch.float32), Permute(1, 0), DynamicTensorBatcher()),
                                                   (TextLoader("PHN"), EncodeInteger(word_tokenizer, tm), TextBatcher())])  # fmt: skip
    ((x, x_sl), (y, y_sl)), _ = ds.collate([ds[0], ds[1]])
    assert x.dtype == torch.float32 and tuple(x.shape) == (2, 3, 6) and x_sl.tolist() == [6, 4]
    assert torch.equal(x[1, :, :4], torch.from_numpy(feats["u1"]).float().T) and float(x[1, :, 4:].abs().max()) == 0.0
    assert y.tolist() == [[3, 3, 2], [2, 1, 0]] and y_sl.tolist() == [3, 2]


def test_synthetic_batches_are_feasible():
    sys.path.insert(0, os.path.join(ROOT, "experiments"))
    try:
        from experiment_asr_ctc import SyntheticLabelled
    finally:
        sys.path.pop(0)
    batches = list(SyntheticLabelled(3, 5, 8, 6, 60, seed=1))
    assert len(batches) == 3
    for (x, x_sl), (y, y_sl) in batches:
        assert tuple(x.shape) == (5, 8, int(x_sl.max())) and tuple(y.shape) == (5, int(y_sl.max()))
        assert bool((x_sl >= 2 * y_sl).all()) and bool((y_sl >= 1).all()) and x_sl.tolist() == sorted(x_sl.tolist(), reverse=True)
        assert int(y.max()) <= 6 and all(int(y[b, : y_sl[b]].min()) >= 1 for b in range(5))
    again = list(SyntheticLabelled(3, 5, 8, 6, 60, seed=1))
    assert all(torch.equal(a[0][0], b[0][0]) and torch.equal(a[1][0], b[1][0]) for a, b in zip(batches, again))


def test_cpu_tensors_are_refused():
    with pytest.raises(_hip.BlvmHipError):
        ops.ctc_loss(torch.zeros(4, 2, 3), torch.ones(2, 1, dtype=torch.long), [4, 4], [1, 1])
    with pytest.raises(_hip.BlvmHipError):
        ops.ctc_greedy(torch.zeros(4, 2, 3), [4, 4])
    model = SimpleLSTMASR(TokenMap(["a"], add_blank=True), input_size=3, hidden_size=16)
    with pytest.raises(_hip.BlvmHipError):
        model(torch.zeros(2, 3, 4), torch.tensor([4, 4]), torch.ones(2, 1, dtype=torch.long), torch.tensor([1, 1]))


def test_experiment_help_parses():
    for script in ("experiment_asr_ctc.py", "dump_representations.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "experiments", script), "--help"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert "--hidden_size" in r.stdout or "--run_dir" in r.stdout
