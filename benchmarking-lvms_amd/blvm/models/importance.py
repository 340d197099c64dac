"""What the models' `iw_bound` methods share: the K-sample importance-weighted bound (IWAE, Burda et al. 2016)

    L_K = log (1/K) sum_k p(x, z_k) / q(z_k | x),   z_k ~ q,

an evaluation quantity beyond the reference, which reports the single-sample ELBO.  Each model runs its deterministic part once on
the B utterances, tiles it along the batch axis for a pass of c particles (rows particle-major: row k * B + b) and runs its
stochastic part and its head on the c * B rows through the kernels `forward` uses; the Monte-Carlo log-ratio and the reduction over
particles are K8m (`ops.gauss_log_ratio_sums`, `ops.iw_reduce`)."""
import contextlib
from types import SimpleNamespace

import torch

from blvm import _hip, ops
from blvm.evaluation import BitsPerDimMetric, DeferredScalars, LLMetric, RunningMeanMetric


@contextlib.contextmanager
def fp32_operands():
    """The bound is compared across runs: always fp32 operands, whatever the training mode (as the experiments' test loop)."""
    prev = _hip.get_operand_dtype()
    _hip.set_operand_dtype("f32")
    try:
        yield
    finally:
        _hip.set_operand_dtype(prev)


def check_samples(num_samples) -> int:
    K = int(num_samples)
    if K < 1:
        raise ValueError(f"iw_bound: num_samples must be at least 1, got {num_samples}")
    return K


def passes(K: int, B: int, max_rows=None):
    """(first particle, particle count) of every pass."""
    k0 = 0
    for c in ops.iw_chunks(K, B, ops.iw_max_rows(B, max_rows)):
        yield k0, c
        k0 += c


def tile_rows(t, c: int, dim: int = 1):
    """[.., B, ..] -> [.., c * B, ..] along `dim`, particle-major (row k * B + b); None stays None."""
    if t is None or c == 1:
        return t
    reps = [1] * t.ndim
    reps[dim] = c
    return t.repeat(*reps)


def pass_eps(eps, k0: int, c: int, T: int, B: int, Z: int, dev):
    """Noise of particles k0 .. k0 + c - 1 as [T, c * B, Z]: from `eps` [K, T, B, Z], or drawn on the device."""
    if eps is None:
        return torch.randn(T, c * B, Z, device=dev, dtype=torch.float32)
    e = torch.as_tensor(eps[k0 : k0 + c]).to(device=dev, dtype=torch.float32)
    if e.shape != (c, T, B, Z):
        raise ValueError(f"iw_bound: eps must be [K, {T}, {B}, {Z}] per level, got {tuple(eps.shape)}")
    return e.permute(1, 0, 2, 3).reshape(T, c * B, Z).contiguous()


def finish(parts, K: int, B: int, n_frames: float):
    """log_w of every pass ([c * B] float64 each, in particle order) -> (bound [B], metrics, outputs)."""
    log_w = torch.cat(parts).view(K, B)
    bound, ess = ops.iw_reduce(log_w)
    sums = DeferredScalars(torch.stack([bound.sum(), ess.sum()]))
    metrics = [
        LLMetric(sums[0], name=f"iw-{K} (nats)", reduce_by=B),
        BitsPerDimMetric(sums[0], name=f"iw-{K} (bpt)", reduce_by=n_frames),
        RunningMeanMetric(sums[1], name=f"iw-{K} ess", reduce_by=B),
    ]
    return bound, metrics, SimpleNamespace(log_w=log_w, ess=ess, elbo_mc=log_w.mean(0))
