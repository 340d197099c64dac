"""What the models' `iw_bound` methods share: the K-sample importance-weighted bound (IWAE, Burda et al. 2016)

    L_K = log (1/K) sum_k p(x, z_k) / q(z_k | x),   z_k ~ q,

an evaluation quantity beyond the reference, which reports the single-sample ELBO.  Each model runs its deterministic part once on
the B utterances, tiles it along the batch axis for a pass of c particles (rows particle-major: row k * B + b) and runs its
stochastic part and its head on the c * B rows through the kernels `forward` uses; the Monte-Carlo log-ratio and the reduction over
particles are K8m (`ops.gauss_log_ratio_sums`, `ops.iw_reduce`).

The models' `represent` methods lay their particles out the same way (`passes`, `tile_rows`, `pass_eps`) but stop at the latents:
the level dependency rule (`levels_upto`) and the mean over particles with the padding zeroed, K8r (`mean_pass`), are below."""
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


# ---- `represent()`: the latents alone, K particles averaged (K8r) -------------------------------------------------------------------
def levels_upto(order, level):
    """The dependency rule of a latent hierarchy visited in `order` (each level conditions on the one visited before it): the
    levels `z[level]` needs, in visiting order; all of them for None.  A level outside the hierarchy raises IndexError."""
    order = list(order)
    if level is None:
        return order
    if isinstance(level, bool) or not isinstance(level, int) or level not in order:
        raise IndexError(f"represent: level {level!r} is outside the hierarchy of {len(order)} level(s)")
    return order[: order.index(level) + 1]


def particle_axis(eps, K: int):
    """`represent`'s noise with the particle axis in front: a single particle's noise may come in `forward`'s shape [T, B, Z]."""
    if eps is None:
        return None
    eps = torch.as_tensor(eps)
    return eps.unsqueeze(0) if (K == 1 and eps.ndim == 3) else eps


def mean_pass(out, z, lens_dev, B: int, k0: int, c: int, K: int):
    """Particles k0 .. k0 + c - 1 (z [T, c * B, Z], row k * B + b) join the running sum `out` [T, B, Z] (None on the first pass); the
    last pass scales by 1 / K and zeroes the frames past `lens_dev`.  One K8r launch; K = 1 is z with its padding zeroed."""
    return ops.particle_mean(z, lens_dev, B, out=out, first=k0 == 0, last=k0 + c == K, scale=1.0 / K)


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
