"""CPU: what `represent()` and the resampling CTC probe decide on the host — the level dependency rules, the refusals, K8r's host
checks and export, the front end's hand-off view on a stub model, the script's flags and the synthetic waveform source."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import blvm_oracle as O
from blvm import _hip, ops
from blvm.data.transforms import LatentRepresentation
from blvm.models import CWVAEAudio, SRNNAudio, STCN, VRNNAudio, importance
from blvm.models.clockwork_vae.clockwork_vae import CWVAE

from conftest import ROOT

SCRIPT = os.path.join(ROOT, "experiments", "experiment_asr_ctc_resampling.py")
CW_SMALL = dict(z_size=[32, 16, 16], h_size=16, strides=[4, 2, 2], num_level_layers=2, stride_per_layer=2, likelihood="DMoL",
                num_mix=10, num_bins=2**16, precision_posterior=True)  # fmt: skip
ST_SMALL = dict(likelihood="DMoL", n_layers=3, latent_size=[16, 16, 32], res_channels=16, n_stack_frames=8)


def test_cwvae_dependency_rule():
    assert CWVAE.represent_levels(3, 2) == [2]
    assert CWVAE.represent_levels(3, 1) == [2, 1]
    assert CWVAE.represent_levels(3, 0) == [2, 1, 0]
    assert CWVAE.represent_levels(3, None) == [2, 1, 0]
    assert CWVAE.represent_levels(1, 0) == [0]
    for bad in (3, -1, 7, 1.0, True):
        with pytest.raises(IndexError):
            CWVAE.represent_levels(3, bad)


def test_stcn_dependency_rule_both_directions():
    assert [STCN.represent_levels(3, True, l) for l in (2, 1, 0, None)] == [[2], [2, 1], [2, 1, 0], [2, 1, 0]]
    assert [STCN.represent_levels(3, False, l) for l in (0, 1, 2, None)] == [[0], [0, 1], [0, 1, 2], [0, 1, 2]]
    for top_down in (True, False):
        for bad in (3, -1):
            with pytest.raises(IndexError):
                STCN.represent_levels(3, top_down, bad)


def test_one_level_models_take_level_none_or_zero():
    assert importance.levels_upto([0], None) == [0] and importance.levels_upto([0], 0) == [0]
    with pytest.raises(IndexError):
        importance.levels_upto([0], 1)


def build(name):
    torch.manual_seed(3)
    if name == "vrnn":
        return VRNNAudio(likelihood="DMoL", input_size=16, hidden_size=32, latent_size=16), 80
    if name == "srnn":
        return SRNNAudio(likelihood="DMoL", input_size=16, hidden_size=32, latent_size=16), 80
    if name == "stcn":
        return STCN(**ST_SMALL), 48
    return CWVAEAudio(**CW_SMALL), 64


@pytest.mark.parametrize("name", ["vrnn", "srnn", "stcn", "cwvae"])
def test_cpu_tensors_bad_counts_and_bad_levels_are_refused(name):
    m, T = build(name)
    x, x_sl = O.synth_batch(3, T, seed=1, ragged=True)
    with pytest.raises(_hip.BlvmHipError):
        m.represent(x, x_sl)
    for k in (0, -2):
        with pytest.raises(ValueError):
            m.represent(x, x_sl, num_samples=k)
    with pytest.raises(IndexError):
        m.represent(x, x_sl, level=3)
    for training in (True, False):  # evaluation-only in either state: the refusal is the same one
        m.train(training)
        with pytest.raises(_hip.BlvmHipError):
            m.represent(x, x_sl, level=0)
    assert not any(p.grad is not None for p in m.parameters())


def test_library_exports_particle_mean_and_the_header_declares_it():
    lib = ctypes.CDLL(_hip.lib_path())
    assert hasattr(lib, "blvm_particle_mean")
    res, args = _hip.SIGNATURES["blvm_particle_mean"]
    c_int, c_float, p = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    assert (res, args) == (c_int, [p, p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, p, p])
    assert callable(ops.particle_mean)


def test_particle_mean_host_checks_run_before_any_launch():
    """No device is touched: the pointers are never dereferenced, every case returns BLVM_EINVAL with its text."""
    lib, einval, p = _hip.load(), _hip.CONSTANTS["BLVM_EINVAL"], 4096
    cases = [
        ((p, p, 3, 1, 3, 6, 1, 1, 1.0, p, None), b"multiple of 4"),
        ((p, p, 3, 1, 3, 18, 1, 1, 1.0, p, None), b"multiple of 4"),
        ((p, p, 3, 0, 3, 16, 1, 1, 1.0, p, None), b"c=0"),
        ((p, p, 3, -1, 3, 16, 1, 1, 1.0, p, None), b"c=-1"),
        ((None, p, 3, 1, 3, 16, 1, 1, 1.0, p, None), b"null"),
        ((p, None, 3, 1, 3, 16, 1, 1, 1.0, p, None), b"null"),
        ((p, p, 3, 1, 3, 16, 1, 1, 1.0, None, None), b"null"),
        ((p + 4, p, 3, 1, 3, 16, 1, 1, 1.0, p, None), b"aligned"),
        ((p, p, 3, 1, 3, 16, 1, 1, 1.0, p + 8, None), b"aligned"),
        ((p, p, 0, 1, 3, 16, 1, 1, 1.0, p, None), b"bad shape"),
        ((p, p, 3, 1, 0, 16, 1, 1, 1.0, p, None), b"bad shape"),
    ]
    for a, text in cases:
        assert lib.blvm_particle_mean(*a) == einval, a
        assert text in lib.blvm_last_error(), (a, lib.blvm_last_error())


def test_ops_particle_mean_refuses_cpu_tensors_and_bad_shapes():
    z, lens = torch.zeros(3, 6, 16), torch.tensor([3, 1, 0], dtype=torch.int32)
    with pytest.raises(_hip.BlvmHipError):
        ops.particle_mean(z, lens, 3)
    with pytest.raises(_hip.BlvmHipError, match="c\\*B"):
        ops.particle_mean(torch.zeros(3, 7, 16), lens, 3)
    with pytest.raises(_hip.BlvmHipError, match="int32"):
        ops.particle_mean(z, lens.long(), 3)


class StubModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(2))
        self.calls = []

    def represent(self, x, x_sl, level=None, num_samples=1, eps=None, max_rows=None):
        self.calls.append((level, num_samples, self.training))
        B = x.shape[0]
        self.z = torch.arange(5 * B * 8, dtype=torch.float32).view(5, B, 8)
        return self.z, torch.tensor([5, 3, 2][:B])


def test_front_end_hands_out_a_view_and_freezes_the_model():
    stub = StubModel().train()
    fe = LatentRepresentation(stub, level=1, num_samples=3)
    assert not stub.training and not stub.w.requires_grad
    fe.train()
    assert not stub.training and not fe.training  # the extractor stays in eval() whatever the modules around it do
    feats, lens = fe(torch.zeros(3, 40), torch.tensor([40, 30, 20]))
    assert stub.calls == [(1, 3, False)] and lens.tolist() == [5, 3, 2]
    assert tuple(feats.shape) == (3, 8, 5) and feats.data_ptr() == stub.z.data_ptr() and not feats.is_contiguous()
    back = feats.permute(2, 0, 1).contiguous()  # what SimpleLSTMASR.forward does with its input
    assert back.data_ptr() == stub.z.data_ptr() and torch.equal(back, stub.z)
    with pytest.raises(TypeError):
        LatentRepresentation(torch.nn.Linear(2, 2))


def test_script_help_lists_its_flags():
    r = subprocess.run([sys.executable, SCRIPT, "--help"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for flag in ("--run_dir", "--z_index", "--num_samples", "--input_coding", "--num_bits", "--synthetic_model", "--hidden_size",
                 "--num_batches_per_epoch", "--optimizer", "--batch_len"):  # fmt: skip
        assert flag in r.stdout, flag


def _script_module():
    """experiments/_asr.py, the module both probe scripts share (it declares no flags, so importing it leaves the parser alone)."""
    sys.path.insert(0, os.path.join(ROOT, "experiments"))
    try:
        import _asr as mod
    finally:
        sys.path.pop(0)
    return mod


def test_synthetic_waveforms_are_deterministic_and_feasible():
    mod = _script_module()
    S = 16
    batches = list(mod.SyntheticWaveforms(3, 5, 6, 60, S, seed=1))
    assert len(batches) == 3
    for (x, x_sl), (y, y_sl) in batches:
        assert tuple(x.shape) == (5, int(x_sl.max())) and tuple(y.shape) == (5, int(y_sl.max())) and x.dtype == torch.float32
        frames = -(-x_sl // S)
        assert bool((x_sl % S == 0).all()) and bool((frames >= 2 * y_sl).all()) and bool((y_sl >= 1).all())
        assert x_sl.tolist() == sorted(x_sl.tolist(), reverse=True)
        assert float(x.abs().max()) <= 1.0 and all(float(x[b, x_sl[b] :].abs().sum()) == 0 for b in range(5))
        assert int(y.max()) <= 6 and all(int(y[b, : y_sl[b]].min()) >= 1 for b in range(5))
    again = list(mod.SyntheticWaveforms(3, 5, 6, 60, S, seed=1))
    assert all(torch.equal(a[0][0], b[0][0]) and torch.equal(a[1][0], b[1][0]) for a, b in zip(batches, again))
    padded = list(mod.SyntheticWaveforms(3, 5, 6, 60, 8, seed=1, pad_to=16))  # strideable batches for a hierarchy
    for ((x, x_sl), _), ((x8, _), _) in zip(padded, list(mod.SyntheticWaveforms(3, 5, 6, 60, 8, seed=1))):
        assert x.shape[1] % 16 == 0 and 0 <= x.shape[1] - int(x_sl.max()) < 16 and torch.equal(x[:, : x8.shape[1]], x8)
        assert float(x[:, x8.shape[1] :].abs().sum()) == 0
    other = list(mod.SyntheticWaveforms(3, 5, 6, 60, S, seed=2))
    assert not all(a[0][0].shape == b[0][0].shape and torch.equal(a[0][0], b[0][0]) for a, b in zip(batches, other))


def test_synthetic_models_have_widths_in_multiples_of_16_and_the_stated_strides():
    mod = _script_module()
    for kind, sizes in (("vrnn", [16]), ("srnn", [16]), ("stcn", [16, 16, 32]), ("cwvae", [32, 16, 16])):
        m, frame_samples = mod.synthetic_model(kind, seed=5)
        assert callable(m.represent) and len(frame_samples) == len(sizes) and all(z % 16 == 0 for z in sizes)
        m2, _ = mod.synthetic_model(kind, seed=5)
        assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
