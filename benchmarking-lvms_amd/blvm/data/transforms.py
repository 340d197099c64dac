"""The transforms on the hot path (reference: blvm/data/transforms.py:90-98 StackTensor, :192-215 µ-law) and the probe's log-mel
front end (:113-166), which runs on the device."""
import math
from typing import Optional

import torch
import torch.nn as nn

from blvm import ops
from blvm._hip import BlvmHipError, ptr
from blvm.utils.operations import stack_tensor


class Transform(nn.Module):
    def forward(self, x):
        raise NotImplementedError()


class StackTensor(Transform):
    def __init__(self, n_frames: int, dim=-1):
        super().__init__()
        self.n_frames = n_frames
        self.dim = dim

    def forward(self, x):
        x, _ = stack_tensor(x, self.n_frames, dim=self.dim)
        return x


class EncodeInteger(Transform):
    """A string -> the indices of its tokens (transforms.py:66-75)."""

    def __init__(self, tokenizer, token_map):
        super().__init__()
        self.tokenizer = tokenizer
        self.token_map = token_map

    def forward(self, x: str):
        return self.token_map.encode(self.tokenizer(x))


class MuLawEncode(Transform):
    def __init__(self, bits: int = 8):
        super().__init__()
        self.bits = bits
        self.mu = 2**bits - 1
        self._divisor = math.log(self.mu + 1)

    def forward(self, x: torch.Tensor):
        return x.sign() * torch.log(1 + self.mu * x.abs()) / self._divisor


class MuLawDecode(Transform):
    def __init__(self, bits: int = 8):
        super().__init__()
        self.bits = bits
        self.mu = 2**bits - 1
        self._divisor = math.log(self.mu + 1)

    def forward(self, x: torch.Tensor):
        return x.sign() * (torch.exp(x.abs() * self._divisor) - 1) / self.mu


class Quantize(Transform):
    """Values in [-1, 1] -> integer classes (transforms.py:216-260): `bucketize` against `linspace(-1, 1, bins)` with right=False, so
    class k is the interval (boundaries[k-1], boundaries[k]] and a value above 1 gets class `bins` (callers that need a class below
    `bins` clamp, as `WaveNet.forward` does).  Give one of `bits` (bins = 2**bits) and `bins` (pass bits=None).
    `rescale=True` returns floats instead: `linspace(low, high, bins)[min(k, bins - 1)]`, the value that quantises back to class k —
    `CategoricalDense.dequantize` for the default range (the reference names a class `Scale` there that does not exist)."""

    def __init__(self, low: float = -1.0, high: float = 1.0, bits: Optional[int] = 8, bins: Optional[int] = None,
                 force_out_int64: bool = True, rescale: bool = False):  # fmt: skip
        super().__init__()
        assert (bits is None) != (bins is None), "Must set one and only one of `bits` and `bins`"
        self.low, self.high = low, high
        self.bits = bins // 8 if bits is None else bits
        self.bins = 2**bits if bins is None else bins
        self.boundaries = torch.linspace(start=-1, end=1, steps=self.bins)
        self.out_int32 = (self.bits <= 32) and (not force_out_int64)
        self.rescale = torch.linspace(start=low, end=high, steps=self.bins) if rescale else None

    def forward(self, x: torch.Tensor):
        k = torch.bucketize(x, self.boundaries.to(x.device), out_int32=self.out_int32, right=False)
        return self.rescale.to(x.device)[k.long().clamp(max=self.bins - 1)] if self.rescale is not None else k


class Compose(Transform):
    """Apply transforms left to right (transforms.py:30-52)."""

    def __init__(self, *transforms):
        super().__init__()
        self.transforms = nn.ModuleList([t for t in transforms if t is not None])

    def forward(self, x):
        for t in self.transforms:
            x = t(x)
        return x


class RandomSegment(Transform):
    """A random window of `length` samples out of an example [T, *] (transforms.py:101-110); one `torch.randint` draw per
    call, shorter examples are returned whole."""

    def __init__(self, length: int):
        super().__init__()
        self.length = length

    def forward(self, x):
        start = int(torch.randint(low=0, high=max(x.size(0) - self.length, 1), size=(1,)))
        return x[start : start + self.length]


class LogMelSpectrogram(Transform):
    """Log-mel spectrogram in dB, normalised per utterance and mel bin (transforms.py:113-166), computed on the device by the fused
    front end (`ops.log_mel_spectrogram`): one call per BATCH of waveforms, where the reference runs torchaudio per example in the
    loader's workers.  `forward(waveform)` takes [time] or [B, time] of full-length rows and returns [..., n_mels, T];
    `forward(waveform, lengths)` takes a right-padded batch with its lengths and returns (features [B, n_mels, T_max], feature
    lengths [B] int32 on the device), T = 1 + time // hop_length.  A CPU tensor raises BlvmHipError."""

    def __init__(self, sample_rate: int = 16000, n_fft: int = 400, win_length: Optional[int] = None, hop_length: Optional[int] = None,
                 n_mels: int = 80, normalize_frq_bins: bool = True):  # fmt: skip
        super().__init__()
        self.sample_rate = sample_rate
        self.n_fft = n_fft
        self.win_length = win_length if win_length is not None else n_fft
        self.hop_length = hop_length if hop_length is not None else self.win_length // 2
        self.n_mels = n_mels
        self.normalize_frq_bins = normalize_frq_bins
        ops.logmel_check_geometry(self.n_fft, self.win_length, self.hop_length, self.n_mels)

    def forward(self, waveform: torch.Tensor, lengths=None):
        ptr(waveform)
        if waveform.dim() not in (1, 2):
            raise BlvmHipError(f"LogMelSpectrogram: waveform must be [time] or [B, time], got {tuple(waveform.shape)}")
        batch = waveform.reshape(-1, waveform.size(-1))
        features, feature_lens = ops.log_mel_spectrogram(
            batch, lengths if lengths is not None else [batch.size(1)] * batch.size(0), self.sample_rate, self.n_fft, self.win_length,
            self.hop_length, self.n_mels, self.normalize_frq_bins)  # fmt: skip
        if lengths is not None:
            return features, feature_lens
        return features[0] if waveform.dim() == 1 else features


class LatentRepresentation(Transform):
    """Fresh latents z ~ q(z | x) of a frozen latent-variable model as the probe's features, drawn anew on every call (the
    reference's `get_representation`, experiments/experiment_asr_ctc_resampling.py:184-199): `forward(x [B,L] on the device, x_sl)`
    -> (features [B, D, T], lengths [B]) from `model.represent(x, x_sl, level, num_samples)`, which runs only what the latents need.
    `features` is the VIEW `z.permute(1, 2, 0)` of the time-major result z [T,B,D]: `SimpleLSTMASR.forward` turns its input back with
    `x.permute(2, 0, 1).contiguous()`, which on this view is z itself, so the hand-off to the LSTM kernels copies nothing.
    The model is put in `eval()` and its parameters are frozen (`requires_grad_(False)`); frames past an utterance's length are zero."""

    def __init__(self, model: nn.Module, level: int = 0, num_samples: int = 1):
        super().__init__()
        if not callable(getattr(model, "represent", None)):
            raise TypeError(f"LatentRepresentation: {type(model).__name__} has no represent() (the latent-variable models have)")
        self.model = model.eval()
        for p in self.model.parameters():
            p.requires_grad_(False)
        self.level, self.num_samples = level, num_samples

    def train(self, mode: bool = True):
        """The extractor stays in `eval()` whatever mode the modules around it are put in."""
        return super().train(False)

    @torch.no_grad()
    def forward(self, x: torch.Tensor, lengths):
        z, z_sl = self.model.represent(x, lengths, level=self.level, num_samples=self.num_samples)
        return z.permute(1, 2, 0), z_sl


class Normalize(Transform):
    """(x - mean) / std with fixed statistics, or the example's own over `dim` (transforms.py:169-179)."""

    def __init__(self, mean=None, std=None, dim: int = -1):
        super().__init__()
        self.mean, self.std, self.dim = mean, std, dim

    def forward(self, x):
        mean = self.mean if self.mean is not None else x.mean(self.dim)
        std = self.std if self.std is not None else x.std(self.dim)
        return (x - mean) / std


class Denormalize(Transform):
    def __init__(self, mean=None, std=None):
        super().__init__()
        self.mean, self.std = mean, std

    def forward(self, x):
        return x * self.std + self.mean
