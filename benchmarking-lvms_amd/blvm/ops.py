"""autograd glue over the C ABI: each Function enqueues hand-written gfx950 kernels (csrc/*.hip) on the current
torch HIP stream.  PyTorch is used for device memory, streams and autograd bookkeeping only — no ATen math on the
hot path, and no CPU fallback (``_hip.ptr`` refuses CPU tensors).

Layout convention: sequence tensors are time-major ``[T', B, F]``.
"""
import ctypes
from typing import List, NamedTuple, Optional, Sequence

import torch

from . import _hip
from ._hip import VrnnWeights, check, load, ptr, stream_ptr

ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
LEAKY_SLOPE = 0.01  # nn.LeakyReLU default (blvm/models/vrnn.py:491)

LAYOUT_BATCH_MAJOR, LAYOUT_TIME_MAJOR = 0, 1

# optional profiling hook: called with "fwd_begin"/"fwd_end"/"bwd_begin"/"bwd_end" around the recurrent-cell calls so
# a caller (bench.py) can record HIP events on the launching stream.  None = disabled.
seq_timer_hook = None


def _tick(tag):
    if seq_timer_hook is not None:
        seq_timer_hook(tag)


def _c_ints(v):
    """A host array of C ints from any sequence of integers."""
    return (ctypes.c_int * len(v))(*[int(i) for i in v])


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise _hip.BlvmHipError(f"blvm HIP kernels compute in fp32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


# ----------------------------------------------------------------------------------------------------------------------
# raw launch helpers (no autograd)
# ----------------------------------------------------------------------------------------------------------------------


def gemm(op_a, op_b, M, N, K, A, lda, B, ldb, C, ldc, bias=None, act=ACT_NONE, slope=0.0, gate=None, ldg=0,
         accumulate=False, split_k=1):  # fmt: skip
    check(
        load().blvm_gemm_f32(op_a, op_b, M, N, K, ptr(A), lda, ptr(B), ldb, ptr(C), ldc, ptr(bias), act, slope,
                             ptr(gate), ldg, int(accumulate), split_k, stream_ptr()),
        "blvm_gemm_f32",
    )  # fmt: skip


def colsum(X2d: torch.Tensor, out: torch.Tensor, accumulate=False):
    M, N = X2d.shape
    check(load().blvm_colsum_f32(M, N, ptr(X2d), X2d.stride(0), ptr(out), int(accumulate), stream_ptr()), "blvm_colsum_f32")


def upload_i32(host, device):
    """Small host integer tensor -> int32 device tensor without blocking the host (the values travel in kernel arguments)."""
    h = host.detach().to(device="cpu", dtype=torch.int32).contiguous()
    out = torch.empty(h.shape, device=device, dtype=torch.int32)
    if h.numel():
        check(load().blvm_upload_i32(h.data_ptr(), h.numel(), ptr(out), stream_ptr()), "blvm_upload_i32")
    return out


def wgrad_group(jobs, rows: int):
    """Weight (+ bias) gradients over the same `rows` as ONE launch (blvm_wgrad_group_f32): jobs = [(D [rows, N], X [rows, K], dW [N, K]
    or None, db [N] or None), ...], each dW += D^T X, db += D.sum(0); D and X may be row-strided views."""
    jobs = [j for j in jobs if j[2] is not None or j[3] is not None]
    if not jobs:
        return
    n = len(jobs)
    ints = lambda v: (ctypes.c_int * n)(*v)  # noqa: E731

    def row_ptr(t):  # (row-strided views are fine: the leading dimension travels beside the pointer)
        if t is None:
            return None
        if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1:
            raise _hip.BlvmHipError("wgrad_group: operands must be float32 [rows, cols] HIP tensors with unit column stride")
        return t.data_ptr()

    ptrs = lambda v: (ctypes.c_void_p * n)(*[ptr(t) for t in v])  # noqa: E731
    rptrs = lambda v: (ctypes.c_void_p * n)(*[row_ptr(t) for t in v])  # noqa: E731
    for D, X, dW, db in jobs:
        if D.shape[0] != rows or X.shape[0] != rows:
            raise _hip.BlvmHipError(f"wgrad_group: operands must be [rows={rows}, *], got {tuple(D.shape)} / {tuple(X.shape)}")
    check(
        load().blvm_wgrad_group_f32(n, ints([j[0].shape[1] for j in jobs]), ints([j[1].shape[1] for j in jobs]), rows,
                                    rptrs([j[0] for j in jobs]), ints([j[0].stride(0) for j in jobs]), rptrs([j[1] for j in jobs]),
                                    ints([j[1].stride(0) for j in jobs]), ptrs([j[2] for j in jobs]),
                                    ints([j[2].stride(0) if j[2] is not None else j[1].shape[1] for j in jobs]), ptrs([j[3] for j in jobs]),
                                    stream_ptr()),
        "blvm_wgrad_group_f32",
    )  # fmt: skip


def _zeros_like_many(tensors):
    """Zero-initialised gradient buffers for `tensors` carved out of ONE allocation (one fill launch instead of one per
    tensor; offsets kept 16-byte aligned)."""
    sizes = [(t.numel() + 3) // 4 * 4 for t in tensors]
    flat = torch.zeros(sum(sizes), device=tensors[0].device, dtype=torch.float32)
    out, off = [], 0
    for t, n in zip(tensors, sizes):
        out.append(flat[off : off + t.numel()].view(t.shape))
        off += n
    return out


def _pick_split(M, N, K):
    """Split-K factor of a weight-gradient GEMM [M,N] += A^T B over K rows: enough workgroups to fill 256 CUs."""
    if K >= 65536 and M >= 128 and N >= 128:  # conv-coder wgrads: K = L*B ~ 4e5 rows, 128x128 tiles, ~4 workgroups per CU
        tiles = ((M + 127) // 128) * ((N + 127) // 128)
        return max(1, min((1024 + tiles - 1) // tiles, K // 2048))
    bm = 64  # gemm_f32 cuts weight-gradient GEMMs into 64x64 tiles (csrc/common.h: gemm_pick_split)
    tiles = ((M + bm - 1) // bm) * ((N + bm - 1) // bm)
    s = (768 + tiles - 1) // tiles
    return max(1, min(s, (K + 255) // 256))


# ----------------------------------------------------------------------------------------------------------------------
# K6: MLP = chain of Linear + (Leaky)ReLU, one autograd node for the whole chain
# ----------------------------------------------------------------------------------------------------------------------


class _MLPFunction(torch.autograd.Function):
    """y = act(...act(x W1^T + b1)... Wn^T + bn) for a 2-D x; activation after EVERY layer (the reference's
    encoders/decoders end in an activation)."""

    @staticmethod
    def forward(ctx, x, act, slope, head_gates, *params):
        """`head_gates`: the consumer of the output is a fused likelihood head whose backward applies the derivative of the LAST
        activation itself (`mlp_dmol_log_prob`), so the incoming gradient is already that of the last pre-activation."""
        x = _f32c(x)
        n_layers = len(params) // 2
        acts = [x]
        for l in range(n_layers):
            W, b = params[2 * l], params[2 * l + 1]
            inp = acts[-1]
            M, K = inp.shape
            N = W.shape[0]
            out = torch.empty(M, N, device=x.device, dtype=torch.float32)
            gemm(0, 0, M, N, K, inp, inp.stride(0), _f32c(W), K, out, N, bias=_f32c(b) if b is not None else None, act=act,
                 slope=slope)
            acts.append(out)
        ctx.act, ctx.slope, ctx.n_layers, ctx.head_gates = act, slope, n_layers, bool(head_gates)
        ctx.save_for_backward(*acts, *params)
        return acts[-1]

    @staticmethod
    def backward(ctx, dy):
        return _MLPFunction._backward(ctx, dy, 4)

    @staticmethod
    def _backward(ctx, dy, first_param):
        """`first_param`: position of the first weight among the node's inputs (what `ctx.needs_input_grad` is indexed by)."""
        n = ctx.n_layers
        saved = ctx.saved_tensors
        acts, params = saved[: n + 1], saved[n + 1 :]
        slope = ctx.slope if ctx.act == ACT_LEAKY else 0.0
        dy = _f32c(dy)
        # derivative of the last activation (no producing GEMM to fuse it into; a fused likelihood head has applied it already)
        if ctx.act != ACT_NONE and not ctx.head_gates:
            dz = torch.empty_like(dy)
            check(load().blvm_act_bwd_f32(ptr(dy), ptr(acts[n]), slope, ptr(dz), dz.numel(), stream_ptr()), "blvm_act_bwd_f32")
        else:
            dz = dy
        grads: List[Optional[torch.Tensor]] = [None] * (2 * n)
        # every weight / bias gradient of the chain as a view of ONE zero-filled buffer (one fill launch instead of 2n)
        want = [ctx.needs_input_grad[first_param + i] and params[i] is not None for i in range(2 * n)]
        sizes = [(params[i].numel() + 3) // 4 * 4 if want[i] else 0 for i in range(2 * n)]
        flat = torch.zeros(sum(sizes), device=dy.device, dtype=torch.float32)
        views, off = [], 0
        for i in range(2 * n):
            views.append(flat[off : off + params[i].numel()].view(params[i].shape) if want[i] else None)
            off += sizes[i]
        jobs = []  # every layer's weight + bias gradient: ONE grouped launch after the chain of dgrads (all share the rows)
        for l in range(n - 1, -1, -1):
            W, b = params[2 * l], params[2 * l + 1]
            inp = acts[l]
            M, K = inp.shape
            N = W.shape[0]
            # weight and bias gradient in one launch (the GEMM's first column block also sums the dz tiles it stages)
            dW, db = views[2 * l], views[2 * l + 1]
            jobs.append((dz, inp, dW, db))  # (keeps this layer's dz alive until the grouped launch below)
            grads[2 * l], grads[2 * l + 1] = dW, db
            if l > 0 or ctx.needs_input_grad[0]:
                dx = torch.empty(M, K, device=dz.device, dtype=torch.float32)
                # dgrad with the derivative of the PREVIOUS layer's activation fused into the epilogue
                gate = acts[l] if (l > 0 and ctx.act != ACT_NONE) else None
                gemm(0, 1, M, K, N, dz, N, _f32c(W), K, dx, K, slope=slope, gate=gate, ldg=K)
                dz = dx
        wgrad_group(jobs, acts[0].shape[0])
        return (dz if ctx.needs_input_grad[0] else None, *(None,) * (first_param - 1), *grads)


class _MLPGivenFunction(torch.autograd.Function):
    """`_MLPFunction` whose forward was already computed elsewhere (the VRNN forward launch runs its decoder as a follower of the
    recurrent chain): `given` = the activations of `x`, one per layer, of the first layers or of all of them.  The remaining layers run
    here; the backward is `_MLPFunction`'s."""

    @staticmethod
    def forward(ctx, x, act, slope, head_gates, given, *params):
        x = _f32c(x)
        n_layers = len(params) // 2
        acts = [x, *given]
        for l in range(len(given), n_layers):  # the layers that were not: K6, as `_MLPFunction` runs them
            W, b = params[2 * l], params[2 * l + 1]
            inp = acts[-1]
            out = torch.empty(inp.shape[0], W.shape[0], device=x.device, dtype=torch.float32)
            gemm(0, 0, inp.shape[0], W.shape[0], inp.shape[1], inp, inp.stride(0), _f32c(W), inp.shape[1], out, W.shape[0],
                 bias=_f32c(b) if b is not None else None, act=act, slope=slope)
            acts.append(out)
        ctx.act, ctx.slope, ctx.n_layers, ctx.head_gates = act, slope, n_layers, bool(head_gates)
        ctx.save_for_backward(*acts, *params)
        return acts[-1]

    @staticmethod
    def backward(ctx, dy):
        return _MLPFunction._backward(ctx, dy, 5)


def mlp(x2d: torch.Tensor, layers: Sequence[torch.nn.Linear], act: int = ACT_LEAKY, slope: float = LEAKY_SLOPE):
    params = []
    for lin in layers:
        params += [lin.weight, lin.bias]
    return _MLPFunction.apply(x2d, act, slope, False, *params)


def linear(x2d: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, act: int = ACT_NONE, slope: float = 0.0):
    """act(x W^T + b) for a raw [out,in] weight (e.g. a 1x1 Conv1d weight viewed as a matrix)."""
    return _MLPFunction.apply(x2d, act, slope, False, weight, bias)


# ----------------------------------------------------------------------------------------------------------------------
# K7: DMoL head (Linear + log-likelihood + masked per-utterance sums)
# ----------------------------------------------------------------------------------------------------------------------


def _dmol_check_shapes(dec, W, y, B, T, Tp, S, num_mix):
    """The fused head is the per-frame [F,F] Linear of the stacked-frame models (F = 3 * num_mix); a head with another
    input width (e.g. CW-VAE's h -> F) runs as a K6 GEMM in front and the kernel gets W = None."""
    F = 3 * num_mix
    if dec.dim() != 2 or dec.shape[0] != B * Tp or dec.shape[1] != S * F:
        raise _hip.BlvmHipError(f"DMoL: activations must be [B*T'={B * Tp}, S*3*num_mix={S * F}], got {tuple(dec.shape)}")
    if W is not None and tuple(W.shape) != (F, F):
        raise _hip.BlvmHipError(f"DMoL: fused head weight must be [{F},{F}], got {tuple(W.shape)}")
    if tuple(y.shape) != (B, T) or Tp * S < T:
        raise _hip.BlvmHipError(f"DMoL: targets must be [B={B}, T={T}] with T <= T'*S={Tp * S}, got {tuple(y.shape)}")


def _head_linear_grads(d_par, dec, W, b, F, n_frames, need_w, need_b):
    """Gradients of a likelihood head's per-frame Linear(F, F): dW = d_par^T dec and db = column sums of d_par over all frames, in one
    launch when both are wanted (the bias gradient rides in the weight-gradient GEMM)."""
    dW = db = None
    if need_w and F % 4 != 0 and F % 2 == 0 and n_frames % 2 == 0 and n_frames >= 4096:
        # F = 30: rows of 120 bytes are not 16-byte aligned and a 30 x 30 output uses a fifth of the GEMM's 64 x 64 tile (measured:
        # 147 us for 246 MB at [64,16000], scalar loads).  Two frames per row -> [n/2, 2F] operands with aligned 240-byte rows and a
        # 60 x 60 product over half the rows whose two diagonal blocks are the wanted sums (even frames | odd frames).
        T2 = torch.zeros(2 * F, 2 * F, device=W.device, dtype=torch.float32)
        tb = torch.zeros(2 * F, device=W.device, dtype=torch.float32) if need_b else None
        half = n_frames // 2
        check(load().blvm_wgrad_f32(2 * F, 2 * F, half, ptr(d_par), 2 * F, ptr(dec), 2 * F, ptr(T2), T2.stride(0), ptr(tb),
                                    max(128, min(512, half // 1024)), stream_ptr()), "blvm_wgrad_f32")  # fmt: skip
        dW = T2[:F, :F] + T2[F : 2 * F, F : 2 * F]
        db = tb[:F] + tb[F:] if need_b else None
        return dW, db
    if need_w:
        dW = torch.zeros_like(W)
        db = torch.zeros_like(b) if need_b else None
        check(load().blvm_wgrad_f32(F, F, n_frames, ptr(d_par), F, ptr(dec), F, ptr(dW), F, ptr(db), max(256, min(1024, n_frames // 1024)),
                                    stream_ptr()), "blvm_wgrad_f32")  # fmt: skip
    elif need_b:
        db = torch.empty_like(b)
        colsum(d_par.view(n_frames, F), db)
    return dW, db


_F32_TWINS = {}  # data_ptr of a float64 gradient vector written by blvm_elbo_bwd -> (that tensor, its version, its float32 rounding)


def _grad_f32(g: torch.Tensor) -> torch.Tensor:
    """Incoming float64 per-utterance gradient as the contiguous float32 vector the kernels read.  When `g` is the very tensor the ELBO
    backward kernel wrote (same storage, not modified since), that kernel's own float32 copy is taken instead of a cast launch."""
    twin = _F32_TWINS.get(g.data_ptr()) if g.dtype == torch.float64 else None
    if twin is not None and twin[0].shape == g.shape and g.is_contiguous() and g._version == twin[1]:
        return twin[2]
    return g.to(torch.float32).contiguous()


_DMOL_WS = {}  # (device index, stream) -> workspace of the fused DMoL backward (tickets zero between launches)


def _dmol_workspace(device, floats: int) -> torch.Tensor:
    key = (device.index, stream_ptr())
    ws = _DMOL_WS.get(key)
    if ws is None or ws.numel() < floats:
        ws = _DMOL_WS[key] = torch.zeros(floats, device=device, dtype=torch.float32)
    return ws


BLVM_NOT_APPLICABLE = _hip.CONSTANTS["BLVM_NOT_APPLICABLE"]


class _DMoLFunction(torch.autograd.Function):
    """`act_slope` >= 0: `dec` is the output of `_MLPFunction(..., head_gates=True)` with that (leaky) ReLU slope, and the gradient
    returned for it is that of the last PRE-activation; < 0: the plain gradient of `dec`."""

    @staticmethod
    def forward(ctx, dec, W, b, y, x_sl_dev, layout, B, T, Tp, S, num_mix, num_bins, log_eps, act_slope):
        dec, y = _f32c(dec), _f32c(y)
        W, b = (_f32c(W), _f32c(b)) if W is not None else (None, None)
        _dmol_check_shapes(dec, W, y, B, T, Tp, S, num_mix)
        log_prob = torch.zeros(B, device=dec.device, dtype=torch.float64)
        check(
            load().blvm_dmol_fwd(ptr(dec), layout, ptr(W), ptr(b), ptr(y), ptr(x_sl_dev), B, T, Tp, S, num_mix, num_bins,
                                 log_eps, ptr(log_prob), None, stream_ptr()),
            "blvm_dmol_fwd",
        )  # fmt: skip
        ctx.has_linear = W is not None
        ctx.save_for_backward(dec, y, x_sl_dev, *((W, b) if W is not None else ()))
        ctx.cfg = (layout, B, T, Tp, S, num_mix, num_bins, log_eps, float(act_slope))
        return log_prob

    @staticmethod
    def backward(ctx, g):
        dec, y, x_sl_dev, *lin = ctx.saved_tensors
        W, b = lin if ctx.has_linear else (None, None)
        layout, B, T, Tp, S, num_mix, num_bins, log_eps, act_slope = ctx.cfg
        g32 = _grad_f32(g)
        F = 3 * num_mix
        lib = load()
        need_w, need_b = ctx.has_linear and ctx.needs_input_grad[1], ctx.has_linear and ctx.needs_input_grad[2]
        ws_floats = lib.blvm_dmol_bwd_fused_workspace_floats(B, Tp, S) if ctx.has_linear else 0
        if ws_floats:
            # one launch: dz (the activation derivative applied), dW and db; d_par is never stored
            dz = torch.empty_like(dec)
            dW = torch.empty_like(W) if need_w else None
            db = torch.empty_like(b) if need_b else None
            ws = _dmol_workspace(dec.device, ws_floats) if (need_w or need_b) else None
            rc = lib.blvm_dmol_bwd_fused(ptr(dec), layout, ptr(W), ptr(b), ptr(y), ptr(x_sl_dev), ptr(g32), B, T, Tp, S, num_mix,
                                         num_bins, log_eps, act_slope, ptr(dz), ptr(dW), ptr(db), ptr(ws), stream_ptr())  # fmt: skip
            if rc == 0:
                return (dz if ctx.needs_input_grad[0] else None, dW, db) + (None,) * 11
            if rc != BLVM_NOT_APPLICABLE:
                check(rc, "blvm_dmol_bwd_fused")
        d_dec = torch.empty_like(dec)
        d_par = torch.empty_like(dec) if ctx.has_linear else None
        check(
            load().blvm_dmol_bwd(ptr(dec), layout, ptr(W), ptr(b), ptr(y), ptr(x_sl_dev), ptr(g32), B, T, Tp, S, num_mix,
                                 num_bins, log_eps, ptr(d_dec), ptr(d_par), stream_ptr()),
            "blvm_dmol_bwd",
        )  # fmt: skip
        n_frames = dec.numel() // F
        dW, db = _head_linear_grads(d_par, dec, W, b, F, n_frames, need_w, need_b)
        if act_slope >= 0.0 and ctx.needs_input_grad[0]:
            dz = torch.empty_like(d_dec)
            check(lib.blvm_act_bwd_f32(ptr(d_dec), ptr(dec), act_slope, ptr(dz), dz.numel(), stream_ptr()), "blvm_act_bwd_f32")
            d_dec = dz
        return (d_dec if ctx.needs_input_grad[0] else None, dW, db) + (None,) * 11


def mlp_given(x2d, layers, given, act: int = ACT_LEAKY, slope: float = LEAKY_SLOPE, head_gates: bool = False):
    """`mlp(x2d, layers, act, slope)` whose activations `given` (one tensor per layer) were computed already."""
    params = []
    for lin in layers:
        params += [lin.weight, lin.bias]
    return _MLPGivenFunction.apply(x2d, act, slope, head_gates, tuple(given), *params)


def mlp_dmol_log_prob(x2d, layers, W, b, y, x_sl_dev, layout, B, T, Tp, S, act: int = ACT_LEAKY, slope: float = LEAKY_SLOPE,
                      num_mix=10, num_bins=256, log_eps=-7.0, given=None, dec_node=None):  # fmt: skip
    """`mlp(x2d, layers, act, slope)` feeding `dmol_log_prob(., W, b, ...)` as one pair of autograd nodes whose backward never writes
    d_par or d_dec: the head's backward kernel hands the MLP the gradient of its last pre-activation and accumulates dW / db itself.
    Returns (dec DETACHED — the activations [rows, S*3*num_mix] for samplers / modes —, log_prob [B] float64)."""
    if dec_node is not None:
        # `dec_node`: the MLP's output as an output of another node that takes the gradient of the last PRE-activation (the VRNN
        # cell's node with its decoder, `DecoderFold(head_gates=True)`): only the head remains to be built
        if act != ACT_LEAKY or W is None:
            raise _hip.BlvmHipError("mlp_dmol_log_prob: a decoder output with head gates needs the leaky ReLU and the fused head Linear")
        return dec_node.detach(), _DMoLFunction.apply(dec_node, W, b, y, x_sl_dev, layout, B, T, Tp, S, num_mix, num_bins, log_eps, slope)
    if act == ACT_NONE or W is None:
        dec = mlp(x2d, layers, act, slope) if given is None else mlp_given(x2d, layers, given, act, slope)
        return dec.detach(), dmol_log_prob(dec, W, b, y, x_sl_dev, layout, B, T, Tp, S, num_mix, num_bins, log_eps)
    params = []
    for lin in layers:
        params += [lin.weight, lin.bias]
    # (differentiable ONLY through the head below; `given`: the activations, computed already)
    dec = _MLPFunction.apply(x2d, act, slope, True, *params) if given is None else mlp_given(x2d, layers, given, act, slope, True)
    gate = slope if act == ACT_LEAKY else 0.0
    return dec.detach(), _DMoLFunction.apply(dec, W, b, y, x_sl_dev, layout, B, T, Tp, S, num_mix, num_bins, log_eps, gate)


def dmol_log_prob(dec, W, b, y, x_sl_dev, layout, B, T, Tp, S, num_mix=10, num_bins=256, log_eps=-7.0):
    """Per-utterance masked DMoL log-likelihood sums [B] (float64) of targets y [B,T] given decoder activations
    `dec` ([rows, S*3*num_mix], rows ordered by `layout`)."""
    return _DMoLFunction.apply(dec, W, b, y, x_sl_dev, layout, B, T, Tp, S, num_mix, num_bins, log_eps, -1.0)


class _GaussHeadFunction(torch.autograd.Function):
    """K7b (kind 1, Gaussian mixture, F = 3*num_mix) / K7c (kind 2, single Gaussian, F = 2): decoder activations -> per-frame
    Linear(F->F) (optional) -> log-likelihood -> masked per-utterance float64 sums [B]."""

    @staticmethod
    def forward(ctx, dec, W, b, y, x_sl_dev, kind, layout, B, T, Tp, S, num_mix, sd_beta, sd_eps):
        dec, y = _f32c(dec), _f32c(y)
        W, b = (_f32c(W), _f32c(b)) if W is not None else (None, None)
        F = 3 * num_mix if kind == 1 else 2
        if dec.dim() != 2 or dec.shape[0] != B * Tp or dec.shape[1] != S * F:
            raise _hip.BlvmHipError(f"Gaussian head: activations must be [B*T'={B * Tp}, S*F={S * F}], got {tuple(dec.shape)}")
        if W is not None and tuple(W.shape) != (F, F):
            raise _hip.BlvmHipError(f"Gaussian head: fused head weight must be [{F},{F}], got {tuple(W.shape)}")
        if tuple(y.shape) != (B, T) or Tp * S < T:
            raise _hip.BlvmHipError(f"Gaussian head: targets must be [B={B}, T={T}] with T <= T'*S={Tp * S}, got {tuple(y.shape)}")
        log_prob = torch.zeros(B, device=dec.device, dtype=torch.float64)
        lib = load()
        if kind == 1:
            rc = lib.blvm_gmm_fwd(ptr(dec), layout, ptr(W), ptr(b), ptr(y), ptr(x_sl_dev), B, T, Tp, S, num_mix, sd_beta, sd_eps,
                                  ptr(log_prob), None, stream_ptr())  # fmt: skip
        else:
            rc = lib.blvm_gauss_head_fwd(ptr(dec), layout, ptr(W), ptr(b), ptr(y), ptr(x_sl_dev), B, T, Tp, S, sd_beta, sd_eps,
                                         ptr(log_prob), None, stream_ptr())  # fmt: skip
        check(rc, "blvm_gmm_fwd" if kind == 1 else "blvm_gauss_head_fwd")
        ctx.has_linear = W is not None
        ctx.save_for_backward(dec, y, x_sl_dev, *((W, b) if W is not None else ()))
        ctx.cfg = (kind, layout, B, T, Tp, S, num_mix, sd_beta, sd_eps, F)
        return log_prob

    @staticmethod
    def backward(ctx, g):
        dec, y, x_sl_dev, *lin = ctx.saved_tensors
        W, b = lin if ctx.has_linear else (None, None)
        kind, layout, B, T, Tp, S, num_mix, sd_beta, sd_eps, F = ctx.cfg
        g32 = g.to(torch.float32).contiguous()
        d_dec = torch.empty_like(dec)
        d_par = torch.empty_like(dec) if ctx.has_linear else None
        lib = load()
        if kind == 1:
            rc = lib.blvm_gmm_bwd(ptr(dec), layout, ptr(W), ptr(b), ptr(y), ptr(x_sl_dev), ptr(g32), B, T, Tp, S, num_mix, sd_beta,
                                  sd_eps, ptr(d_dec), ptr(d_par), stream_ptr())  # fmt: skip
        else:
            rc = lib.blvm_gauss_head_bwd(ptr(dec), layout, ptr(W), ptr(b), ptr(y), ptr(x_sl_dev), ptr(g32), B, T, Tp, S, sd_beta,
                                         sd_eps, ptr(d_dec), ptr(d_par), stream_ptr())  # fmt: skip
        check(rc, "blvm_gmm_bwd" if kind == 1 else "blvm_gauss_head_bwd")
        n_frames = dec.numel() // F
        dW, db = _head_linear_grads(d_par, dec, W, b, F, n_frames, ctx.has_linear and ctx.needs_input_grad[1], ctx.has_linear and ctx.needs_input_grad[2])
        return (d_dec if ctx.needs_input_grad[0] else None, dW, db) + (None,) * 11


GMM_MAX_MIX = 16  # blvm_gmm_fwd / blvm_gmm_bwd: 1 <= num_mix <= 16 (csrc/dmol.hip)


def _gmm_check_count(num_mix: int):
    """The library refuses a count outside 1..16 before any launch; here that refusal is a NotImplementedError."""
    if not 1 <= int(num_mix) <= GMM_MAX_MIX:
        raise NotImplementedError(f"libblvm_hip: the Gaussian-mixture head is built for 1 <= num_mix <= {GMM_MAX_MIX}, got num_mix = {num_mix}")


def gmm_log_prob(dec, W, b, y, x_sl_dev, layout, B, T, Tp, S, num_mix, sd_beta, sd_eps):
    """Per-utterance masked Gaussian-mixture log-likelihood sums [B] (float64); dec [rows, S*3*num_mix], 1 <= num_mix <= 16 (K7b: ten
    components on the path of the audio models, any other count on the general arm)."""
    _gmm_check_count(num_mix)
    return _GaussHeadFunction.apply(dec, W, b, y, x_sl_dev, 1, layout, B, T, Tp, S, num_mix, float(sd_beta), float(sd_eps))


def gauss_log_prob(dec, W, b, y, x_sl_dev, layout, B, T, Tp, S, sd_beta, sd_eps):
    """Per-utterance masked Gaussian log-likelihood sums [B] (float64); dec [rows, S*2]."""
    return _GaussHeadFunction.apply(dec, W, b, y, x_sl_dev, 2, layout, B, T, Tp, S, 10, float(sd_beta), float(sd_eps))


def mix_sample(par, u, v, kind: int, log_eps: float = -7.0, sd_beta: float = 1.0, sd_eps: float = 0.0):
    """Sample / mode of a 10-component mixture head (no autograd): par [..., 30] head outputs, u [..., 10] uniforms or None (mode),
    v [...] component noise or None (location).  kind 0 DMoL, 1 GMM.  Returns [...]."""
    par = _f32c(par)
    lead = par.shape[:-1]
    n = par.numel() // par.shape[-1]
    out = torch.empty(n, device=par.device, dtype=torch.float32)
    u = _f32c(u.reshape(n, -1)) if u is not None else None
    v = _f32c(v.reshape(n)) if v is not None else None
    check(load().blvm_mix_sample(ptr(par), ptr(u), ptr(v), n, par.shape[-1] // 3, kind, log_eps, sd_beta, sd_eps, ptr(out), stream_ptr()),
          "blvm_mix_sample")  # fmt: skip
    return out.view(*lead)


def dmol_ll_twise(dec, W, b, y, x_sl_dev, layout, B, T, Tp, S, num_mix=10, num_bins=256, log_eps=-7.0):
    """Masked frame-wise log-likelihood [B,T] (no autograd)."""
    dec, y = _f32c(dec), _f32c(y)
    W, b = (_f32c(W), _f32c(b)) if W is not None else (None, None)
    _dmol_check_shapes(dec, W, y, B, T, Tp, S, num_mix)
    lp = torch.zeros(B, device=dec.device, dtype=torch.float64)
    ll = torch.zeros(B, T, device=dec.device, dtype=torch.float32)  # (caller zeroes: the kernel writes the unmasked frames only)
    check(
        load().blvm_dmol_fwd(ptr(dec), layout, ptr(W), ptr(b), ptr(y), ptr(x_sl_dev), B, T, Tp, S, num_mix, num_bins,
                             log_eps, ptr(lp), ptr(ll), stream_ptr()),
        "blvm_dmol_fwd",
    )  # fmt: skip
    return ll, lp


def _gauss_ll_twise(kind, dec, W, b, y, x_sl_dev, layout, B, T, Tp, S, num_mix, sd_beta, sd_eps):
    dec, y = _f32c(dec), _f32c(y)
    W, b = (_f32c(W), _f32c(b)) if W is not None else (None, None)
    F = 3 * num_mix if kind == 1 else 2
    if dec.dim() != 2 or dec.shape[0] != B * Tp or dec.shape[1] != S * F:
        raise _hip.BlvmHipError(f"Gaussian head: activations must be [B*T'={B * Tp}, S*F={S * F}], got {tuple(dec.shape)}")
    if W is not None and tuple(W.shape) != (F, F):
        raise _hip.BlvmHipError(f"Gaussian head: fused head weight must be [{F},{F}], got {tuple(W.shape)}")
    if tuple(y.shape) != (B, T) or Tp * S < T:
        raise _hip.BlvmHipError(f"Gaussian head: targets must be [B={B}, T={T}] with T <= T'*S={Tp * S}, got {tuple(y.shape)}")
    lp = torch.zeros(B, device=dec.device, dtype=torch.float64)
    ll = torch.zeros(B, T, device=dec.device, dtype=torch.float32)  # (caller zeroes: the kernel writes the unmasked frames only)
    lib = load()
    if kind == 1:
        check(lib.blvm_gmm_fwd(ptr(dec), layout, ptr(W), ptr(b), ptr(y), ptr(x_sl_dev), B, T, Tp, S, num_mix, float(sd_beta), float(sd_eps),
                               ptr(lp), ptr(ll), stream_ptr()), "blvm_gmm_fwd")  # fmt: skip
    else:
        check(lib.blvm_gauss_head_fwd(ptr(dec), layout, ptr(W), ptr(b), ptr(y), ptr(x_sl_dev), B, T, Tp, S, float(sd_beta), float(sd_eps),
                                      ptr(lp), ptr(ll), stream_ptr()), "blvm_gauss_head_fwd")  # fmt: skip
    return ll, lp


def gmm_ll_twise(dec, W, b, y, x_sl_dev, layout, B, T, Tp, S, num_mix, sd_beta, sd_eps):
    """Masked frame-wise Gaussian-mixture log-likelihood [B,T] and its sums [B] float64 (no autograd); arguments as `gmm_log_prob`."""
    _gmm_check_count(num_mix)
    return _gauss_ll_twise(1, dec, W, b, y, x_sl_dev, layout, B, T, Tp, S, num_mix, sd_beta, sd_eps)


def gauss_ll_twise(dec, W, b, y, x_sl_dev, layout, B, T, Tp, S, sd_beta, sd_eps):
    """Masked frame-wise Gaussian log-likelihood [B,T] and its sums [B] float64 (no autograd); arguments as `gauss_log_prob`."""
    return _gauss_ll_twise(2, dec, W, b, y, x_sl_dev, layout, B, T, Tp, S, 0, sd_beta, sd_eps)


# ----------------------------------------------------------------------------------------------------------------------
# K7d: categorical head fused with its Linear(C -> V) — the [frames, V] logits are never stored
# ----------------------------------------------------------------------------------------------------------------------

BLVM_ENOSUP = _hip.CONSTANTS["BLVM_ENOSUP"]


def categorical_check_widths(C: int, V: int):
    """The widths the fused categorical head is built for (host arithmetic: raises before any device work)."""
    if C % 16 != 0 or not 16 <= C <= 512 or not 2 <= V <= 65536:
        raise NotImplementedError(f"libblvm_hip: the categorical head takes C % 16 == 0, 16 <= C <= 512 and 2 <= V <= 65536, got C = {C}, V = {V}")


def _cat_check(rc: int, what: str):
    if rc == BLVM_ENOSUP:
        raise NotImplementedError(f"libblvm_hip: {load().blvm_last_error().decode(errors='replace')}")
    check(rc, what)


def _cat_operands(dec, W, b, y, B, T, Tp, S):
    if W.dim() != 2 or b.dim() != 1 or b.shape[0] != W.shape[0]:
        raise _hip.BlvmHipError(f"categorical head: weight [V,C] and bias [V], got {tuple(W.shape)} and {tuple(b.shape)}")
    V, C = W.shape
    categorical_check_widths(C, V)
    if dec.dim() != 2 or dec.shape[0] != B * Tp or dec.shape[1] != S * C:
        raise _hip.BlvmHipError(f"categorical head: activations must be [B*T'={B * Tp}, S*C={S * C}], got {tuple(dec.shape)}")
    if tuple(y.shape) != (B, T) or Tp * S < T:
        raise _hip.BlvmHipError(f"categorical head: targets must be [B={B}, T={T}] with T <= T'*S={Tp * S}, got {tuple(y.shape)}")
    if y.dtype not in (torch.int32, torch.int64):
        raise _hip.BlvmHipError(f"categorical head: targets are integer classes, got {y.dtype}")
    y32 = y if y.dtype == torch.int32 else y.to(torch.int32)  # a class beyond int32 is beyond V: it wraps to another wrong class
    return _f32c(dec), _f32c(W), _f32c(b), y32.contiguous(), V, C


def _cat_forward(dec, W, b, y32, x_sl_dev, B, T, Tp, S, C, V, want_sums: bool):
    lse = torch.empty(B * Tp * S, device=dec.device, dtype=torch.float32)
    ll = torch.empty(B, T, device=dec.device, dtype=torch.float32)
    log_prob = torch.zeros(B, device=dec.device, dtype=torch.float64) if want_sums else None
    _cat_check(load().blvm_cat_fwd(ptr(dec), ptr(W), ptr(b), ptr(y32), ptr(x_sl_dev), B, T, Tp, S, C, V, ptr(lse), ptr(ll), ptr(log_prob),
                                   stream_ptr()), "blvm_cat_fwd")  # fmt: skip
    return lse, ll, log_prob


class _CategoricalFunction(torch.autograd.Function):
    """Saves the activations, the targets and one log-sum-exp per frame; the backward recomputes the logits tile by tile."""

    @staticmethod
    def forward(ctx, dec, W, b, y, x_sl_dev, B, T, Tp, S):
        dec, W, b, y32, V, C = _cat_operands(dec, W, b, y, B, T, Tp, S)
        lse, _, log_prob = _cat_forward(dec, W, b, y32, x_sl_dev, B, T, Tp, S, C, V, True)
        ctx.save_for_backward(dec, W, b, y32, x_sl_dev, lse)
        ctx.cfg = (B, T, Tp, S, C, V)
        return log_prob

    @staticmethod
    def backward(ctx, g):
        dec, W, b, y32, x_sl_dev, lse = ctx.saved_tensors
        B, T, Tp, S, C, V = ctx.cfg
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        g32 = _grad_f32(g)
        lib = load()
        d_dec = torch.empty_like(dec) if need_x else None
        dW = torch.empty_like(W) if need_w else None
        db = torch.empty_like(b) if need_b else None
        ws_floats = lib.blvm_cat_bwd_workspace_floats(B * Tp * S, C, V) if (need_w or need_b) else 0
        ws = torch.empty(ws_floats, device=dec.device, dtype=torch.float32) if ws_floats else None
        _cat_check(lib.blvm_cat_bwd(ptr(dec), ptr(W), ptr(b), ptr(y32), ptr(x_sl_dev), ptr(lse), ptr(g32), B, T, Tp, S, C, V, ptr(d_dec),
                                    ptr(dW), ptr(db), ptr(ws), stream_ptr()), "blvm_cat_bwd")  # fmt: skip
        return (d_dec, dW, db) + (None,) * 6


def categorical_log_prob(dec, W, b, y, x_sl_dev, B, T, Tp, S):
    """Per-utterance masked categorical log-likelihood sums [B] (float64) of integer targets y [B,T] under softmax(dec W^T + b);
    `dec` [B*T', S*C] time-major rows.  Gradients for dec, W and b, each only where it is needed."""
    return _CategoricalFunction.apply(dec, W, b, y, x_sl_dev, B, T, Tp, S)


def categorical_ll_twise(dec, W, b, y, x_sl_dev, B, T, Tp, S):
    """Masked frame-wise log-likelihood [B,T] (no autograd)."""
    dec, W, b, y32, V, C = _cat_operands(dec.detach(), W.detach(), b.detach(), y, B, T, Tp, S)
    return _cat_forward(dec, W, b, y32, x_sl_dev, B, T, Tp, S, C, V, False)[1]


def categorical_sample(logits, u=None):
    """Classes [...] (int64) from logits [..., V] (no autograd): the arg-max (lowest index on a tie) without `u`, else the inverse
    CDF at the uniforms u [...]."""
    logits = _f32c(logits.detach())
    V = logits.shape[-1]
    lead = logits.shape[:-1]
    n = logits.numel() // V
    out = torch.empty(n, device=logits.device, dtype=torch.int32)
    u = _f32c(u.to(device=logits.device, dtype=torch.float32).reshape(n)) if u is not None else None
    _cat_check(load().blvm_cat_sample(ptr(logits), ptr(u), n, V, ptr(out), stream_ptr()), "blvm_cat_sample")
    return out.view(*lead).to(torch.int64)


# ----------------------------------------------------------------------------------------------------------------------
# K8: Gaussian KL + free nats + masked sums (stand-alone form; the VRNN path fuses the backward into K1)
# ----------------------------------------------------------------------------------------------------------------------


class _KLFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu_q, sd_q, mu_p, sd_p, x_sl_dev, layout, B, Tp, Z, stride, fn_floor):
        mu_q, sd_q, mu_p, sd_p = (_f32c(t) for t in (mu_q, sd_q, mu_p, sd_p))
        kld = torch.zeros(B, device=mu_q.device, dtype=torch.float64)
        kld_fn = torch.zeros(B, device=mu_q.device, dtype=torch.float64)
        check(
            load().blvm_kl_fwd(ptr(mu_q), ptr(sd_q), ptr(mu_p), ptr(sd_p), layout, ptr(x_sl_dev), B, Tp, Z, stride,
                               fn_floor, ptr(kld), ptr(kld_fn), stream_ptr()),
            "blvm_kl_fwd",
        )  # fmt: skip
        ctx.save_for_backward(mu_q, sd_q, mu_p, sd_p, x_sl_dev)
        ctx.cfg = (layout, B, Tp, Z, stride, fn_floor)
        return kld, kld_fn

    @staticmethod
    def backward(ctx, g_raw, g_fn):
        mu_q, sd_q, mu_p, sd_p, x_sl_dev = ctx.saved_tensors
        layout, B, Tp, Z, stride, fn_floor = ctx.cfg
        c_raw = g_raw.to(torch.float32).contiguous()
        c_fn = g_fn.to(torch.float32).contiguous()
        outs = [torch.empty_like(mu_q) for _ in range(4)]
        check(
            load().blvm_kl_bwd(ptr(mu_q), ptr(sd_q), ptr(mu_p), ptr(sd_p), layout, ptr(x_sl_dev), ptr(c_raw), ptr(c_fn),
                               B, Tp, Z, stride, fn_floor, *(ptr(o) for o in outs), stream_ptr()),
            "blvm_kl_bwd",
        )  # fmt: skip
        return (*outs, None, None, None, None, None, None, None)


def gaussian_kl_sums(mu_q, sd_q, mu_p, sd_p, x_sl_dev, layout, B, Tp, Z, stride, free_nats=0.0):
    """(kld[B], kld_fn[B]) in float64: masked sums of the analytic KL and of max(KL, free_nats/Z)."""
    fn_floor = float(free_nats) / Z if free_nats else 0.0
    return _KLFunction.apply(mu_q, sd_q, mu_p, sd_p, x_sl_dev, layout, B, Tp, Z, stride, fn_floor)


# ----------------------------------------------------------------------------------------------------------------------
# K8m: the importance-weighted bound's reductions (evaluation only: none of these builds an autograd graph)
# ----------------------------------------------------------------------------------------------------------------------


def gauss_log_ratio_sums(mu_q, sd_q, mu_p, sd_p, z, eps, x_sl_dev, layout, B, Tp, Z, stride):
    """[B] float64: masked per-utterance sums of log q(z) - log p(z) at the drawn z = mu_q + sd_q eps (`blvm_gauss_logratio_fwd`).
    The six operands are [Tp*B, Z] fp32 in `layout`; step t of row b counts iff t * stride < x_sl_dev[b]."""
    ts = [_f32c(t.detach()) for t in (mu_q, sd_q, mu_p, sd_p, z, eps)]
    n = int(B) * int(Tp) * int(Z)
    if any(t.numel() != n for t in ts):
        raise _hip.BlvmHipError(f"gauss_log_ratio_sums: operands must hold B*Tp*Z = {n} elements, got {[t.numel() for t in ts]}")
    if x_sl_dev.dtype != torch.int32 or x_sl_dev.numel() != B:
        raise _hip.BlvmHipError("gauss_log_ratio_sums: x_sl_dev must be int32 [B]")
    ptrs = [ptr(t) for t in ts]  # (refuses CPU tensors before anything is allocated)
    out = torch.empty(B, device=ts[0].device, dtype=torch.float64)
    check(load().blvm_gauss_logratio_fwd(*ptrs, int(layout), ptr(x_sl_dev), int(B), int(Tp), int(Z), int(stride), ptr(out),
                                         stream_ptr()), "blvm_gauss_logratio_fwd")  # fmt: skip
    return out


def iw_reduce(log_w):
    """log_w [K, B] float64 -> (bound [B], ess [B]) float64: bound = logsumexp_k(log_w) - log K, ess = (sum w)^2 / sum w^2 with the
    weights normalised by the column's maximum (`blvm_iw_reduce`)."""
    if log_w.dtype != torch.float64 or log_w.ndim != 2:
        raise _hip.BlvmHipError("iw_reduce: log_w must be float64 [K, B]")
    log_w = log_w.detach().contiguous()
    K, B = log_w.shape
    p = ptr(log_w)  # (refuses a CPU tensor before anything is allocated)
    bound, ess = (torch.empty(B, device=log_w.device, dtype=torch.float64) for _ in range(2))
    check(load().blvm_iw_reduce(p, K, B, ptr(bound), ptr(ess), stream_ptr()), "blvm_iw_reduce")
    return bound, ess


def iw_chunks(K: int, B: int, max_rows: int) -> List[int]:
    """Particle counts per pass for K particles of B utterances: every pass carries c particles with c * B <= max_rows (c = 1 where
    B alone exceeds max_rows), as many as fit, the remainder last; the counts sum to K.  Host arithmetic."""
    K, B, max_rows = int(K), int(B), int(max_rows)
    if K < 1 or B < 1 or max_rows < 1:
        raise ValueError(f"iw_chunks: K, B and max_rows must be positive, got {K}, {B}, {max_rows}")
    c = max(1, max_rows // B)
    return [c] * (K // c) + ([K % c] if K % c else [])


def iw_max_rows(B: int, max_rows: Optional[int] = None) -> int:
    """The rows of one `iw_bound` pass: `max_rows`, or by default max(B, blvm_pchain_max_batch()), which keeps the recurrent chains
    on their persistent path."""
    return int(max_rows) if max_rows is not None else max(int(B), int(load().blvm_pchain_max_batch()))


# ----------------------------------------------------------------------------------------------------------------------
# K8r: the mean over particles with the padding zeroed, the last launch of every `represent()` level (evaluation only)
# ----------------------------------------------------------------------------------------------------------------------


def particle_mean(z, lens_dev, B: int, out=None, first: bool = True, last: bool = True, scale: float = 1.0):
    """z [T, c*B, Z] fp32 time-major (row k * B + b) -> out [T, B, Z] (`blvm_particle_mean`): out = (0 if `first` else out) + the c
    particles in ascending order, one fp32 add each; with `last`, times `scale` on frames t < lens_dev[b] and +0 beyond.  `out` is
    allocated where None (then `first` must hold: there is nothing to add to).  c = 1, scale = 1: z with the padding zeroed."""
    if z.ndim != 3 or z.shape[1] % int(B) or z.shape[1] < int(B):
        raise _hip.BlvmHipError(f"particle_mean: z must be [T, c*B, Z] with B = {B}, got {tuple(z.shape)}")
    z = _f32c(z.detach())
    T, rows, Z = z.shape
    if lens_dev.dtype != torch.int32 or lens_dev.numel() != B:
        raise _hip.BlvmHipError("particle_mean: lens_dev must be int32 [B]")
    pz = ptr(z)  # (refuses a CPU tensor before anything is allocated)
    if out is None:
        if not first:
            raise _hip.BlvmHipError("particle_mean: a pass that is not the first needs the `out` of the passes before it")
        out = torch.empty(T, B, Z, device=z.device, dtype=torch.float32)
    elif out.shape != (T, B, Z) or out.dtype != torch.float32:
        raise _hip.BlvmHipError(f"particle_mean: out must be fp32 [{T}, {B}, {Z}], got {out.dtype} {tuple(out.shape)}")
    check(load().blvm_particle_mean(pz, ptr(lens_dev), T, rows // int(B), int(B), Z, int(bool(first)), int(bool(last)), float(scale),
                                    ptr(out), stream_ptr()), "blvm_particle_mean")  # fmt: skip
    return out


class _ELBOFunction(torch.autograd.Function):
    """(log_prob, kld, kld_fn [B] float64) -> (loss scalar, elbo [B], sums [4]) in one launch; backward one launch (`blvm_elbo_bwd`)."""

    @staticmethod
    def forward(ctx, log_prob, kld, kld_fn, beta, n_frames, kl_raw):
        B = log_prob.numel()
        for t in (log_prob, kld, kld_fn):
            if t.dtype != torch.float64 or t.shape != (B,):
                raise _hip.BlvmHipError("elbo_assemble: log_prob, kld and kld_fn must be float64 [B]")
        log_prob, kld, kld_fn = log_prob.contiguous(), kld.contiguous(), kld_fn.contiguous()
        f64 = dict(device=log_prob.device, dtype=torch.float64)
        loss, elbo, sums = torch.empty((), **f64), torch.empty(B, **f64), torch.empty(4, **f64)
        check(load().blvm_elbo_fwd(ptr(log_prob), ptr(kld), ptr(kld_fn), float(beta), float(n_frames), B, int(kl_raw), ptr(elbo), ptr(loss),
                                   ptr(sums), stream_ptr()), "blvm_elbo_fwd")  # fmt: skip
        ctx.cfg = (float(beta), float(n_frames), B)
        ctx.mark_non_differentiable(sums)
        ctx.set_materialize_grads(False)
        return loss, elbo, sums

    @staticmethod
    def backward(ctx, g_loss, g_elbo, _g_sums):
        beta, n_frames, B = ctx.cfg
        if g_loss is None and g_elbo is None:
            return (None,) * 6
        dev = g_loss.device if g_loss is not None else g_elbo.device
        g_loss = g_loss.to(torch.float64).contiguous() if g_loss is not None else None  # (no launch: it is float64 already)
        g_elbo = g_elbo.to(torch.float64).contiguous() if g_elbo is not None else None
        g64 = torch.empty(3, B, device=dev, dtype=torch.float64)
        g32 = torch.empty(3, B, device=dev, dtype=torch.float32)
        check(load().blvm_elbo_bwd(ptr(g_loss), ptr(g_elbo), beta, n_frames, B, ptr(g64), ptr(g32), stream_ptr()), "blvm_elbo_bwd")
        _F32_TWINS.clear()  # (the consumers of the previous step's vectors have run)
        outs = []
        for i in range(3):
            v = g64[i]
            _F32_TWINS[v.data_ptr()] = (v, v._version, g32[i])
            outs.append(v)
        d_lp, d_fn, d_raw = outs
        return d_lp, (d_raw if g_elbo is not None else None), d_fn, None, None, None


def elbo_assemble(log_prob, kld, kld_fn, beta: float, n_frames: float, kl_raw: bool = False):
    """(loss, elbo [B], sums [4]) float64: elbo = log_prob - kld, loss = -(log_prob - beta * kld_fn).sum() / n_frames, sums = (loss,
    elbo.sum(), log_prob.sum(), kl.sum()) with kl = kld if `kl_raw` else kld_fn — `sums` detached, for `DeferredScalars`."""
    return _ELBOFunction.apply(log_prob, kld, kld_fn, beta, n_frames, kl_raw)


# ----------------------------------------------------------------------------------------------------------------------
# K1: VRNN cell over a sequence
# ----------------------------------------------------------------------------------------------------------------------

_VRNN_PARAM_ORDER = (
    ["prior_w0", "prior_b0", "prior_w1", "prior_b1", "prior_w2", "prior_b2", "prior_hw", "prior_hb"]
    + ["post_w0", "post_b0", "post_w1", "post_b1", "post_w2", "post_b2", "post_hw", "post_hb"]
    + ["phi_w0", "phi_b0", "phi_w1", "phi_b1", "phi_w2", "phi_b2", "phi_w3", "phi_b3"]
    + ["gru_wih", "gru_whh", "gru_bih", "gru_bhh"]
)


class _GaussLatentFunction(torch.autograd.Function):
    """(mu_p, sd_p_raw, mu_q_raw, sd_q_raw, eps) -> (sd_p, mu_q, sd_q, z): softplus heads, posterior combination and the
    reparameterised sample of one STCN latent level, elementwise (K8b)."""

    @staticmethod
    def forward(ctx, mu_p, sp_raw, mq, sq_raw, eps, cfg):
        mu_p, sp_raw, mq, sq_raw, eps = (_f32c(t) for t in (mu_p, sp_raw, mq, sq_raw, eps))
        beta_p, beta_q, sd_eps, mode = cfg
        outs = [torch.empty_like(mu_p) for _ in range(4)]
        check(load().blvm_gauss_latent_fwd(ptr(mu_p), ptr(sp_raw), ptr(mq), ptr(sq_raw), ptr(eps), mu_p.numel(), beta_p, beta_q,
                                           sd_eps, mode, *(ptr(o) for o in outs), stream_ptr()), "blvm_gauss_latent_fwd")  # fmt: skip
        ctx.cfg = cfg
        ctx.save_for_backward(mu_p, sp_raw, mq, sq_raw, eps)
        return tuple(outs)

    @staticmethod
    def backward(ctx, g_sd_p, g_mu_q, g_sd_q, g_z):
        mu_p, sp_raw, mq, sq_raw, eps = ctx.saved_tensors
        beta_p, beta_q, sd_eps, mode = ctx.cfg
        gs = [_f32c(g) if g is not None else None for g in (g_sd_p, g_mu_q, g_sd_q, g_z)]
        outs = [torch.empty_like(mu_p) for _ in range(4)]
        check(load().blvm_gauss_latent_bwd(ptr(mu_p), ptr(sp_raw), ptr(mq), ptr(sq_raw), ptr(eps), *(ptr(g) for g in gs),
                                           mu_p.numel(), beta_p, beta_q, sd_eps, mode, *(ptr(o) for o in outs), stream_ptr()),
              "blvm_gauss_latent_bwd")  # fmt: skip
        return (*outs, None, None)


def gauss_latent(mu_p, sd_p_raw, mu_q_raw, sd_q_raw, eps, beta_p: float, beta_q: float, sd_eps: float, mode: int):
    return _GaussLatentFunction.apply(mu_p, sd_p_raw, mu_q_raw, sd_q_raw, eps, (float(beta_p), float(beta_q), float(sd_eps), int(mode)))


def _pack(struct, order, ts: Sequence[Optional[torch.Tensor]]):
    """A weights or grads struct of the C ABI from tensors in the Python-side parameter order (None -> NULL)."""
    return _hip.fill(struct(), order, [ptr(t) for t in ts])


def _pack_weights(ts, struct=VrnnWeights):
    return _pack(struct, _VRNN_PARAM_ORDER, ts)


# The one-launch roll-outs (blvm_vrnn_generate, blvm_srnn_generate, blvm_lstm_generate_any_stack) keep one slab per step of every activation in
# their scratch: at one sample per step a second of audio is 16 000 steps and gigabytes.  A roll-out whose scratch would exceed this
# many floats (1 GiB) runs as consecutive launches of as many steps as fit, each starting from the previous one's last stack and state.
MAX_SCRATCH_FLOATS = 2**28


def _steps_per_launch(scratch_floats, T, max_scratch_floats, who):
    """The most steps n <= T with scratch_floats(n) <= max_scratch_floats (scratch_floats: steps -> floats, increasing)."""
    bound = MAX_SCRATCH_FLOATS if max_scratch_floats is None else int(max_scratch_floats)
    if scratch_floats(T) <= bound:
        return T
    one = scratch_floats(1)
    if one > bound:
        raise ValueError(f"{who}: one step needs {one} floats of scratch, max_scratch_floats is {bound}")
    n = max(1, min(T, 1 + (bound - one) // max(1, scratch_floats(2) - one)))
    while n > 1 and scratch_floats(n) > bound:
        n -= 1
    return n


def _rollout(scratch_floats, T, max_scratch_floats, who, x, call, carry):
    """The driver of the one-launch roll-outs: one launch when the scratch of T steps fits the bound, else consecutive launches of as
    many steps as fit.  scratch_floats: steps -> floats; x [B,T,S] receives the samples; call(t0, t1, state, x_chunk, scratch) runs
    steps [t0, t1) from `state` (None: the caller's own start) into x_chunk [B,t1-t0,S]; carry(x_chunk, t1) -> the next chunk's
    state, taken from what the previous call put out (its last frame stack, copies of its final states)."""
    n = _steps_per_launch(scratch_floats, T, max_scratch_floats, who) if T > 0 else 0
    scratch = torch.empty(scratch_floats(n), device=x.device, dtype=torch.float32)
    if n == T:
        call(0, T, None, x, scratch)
        return
    state = None
    for t0 in range(0, T, n):
        t1 = min(T, t0 + n)
        xc = torch.empty(x.shape[0], t1 - t0, x.shape[2], device=x.device, dtype=torch.float32)
        call(t0, t1, state, xc, scratch)
        x[:, t0:t1] = xc
        state = carry(xc, t1)


def _decode_weight_ptrs(w, first, first_lin, dec_lin, lik_lin):
    """Fills the `first`_w / `first`_b ("enc" | "emb"), dec_w / dec_b and lik_w / lik_b pointers of a decode-weights struct from the
    3 + 3 + 1 nn.Linear; -> the float32 contiguous tensors, which must stay alive while `w` is used."""
    keep = [_f32c(t) for lin in (*first_lin, *dec_lin, lik_lin) for t in (lin.weight, lin.bias)]
    names = [f"{part}_{k}{i}" for part in (first, "dec") for i in range(3) for k in "wb"] + ["lik_w", "lik_b"]
    _hip.fill(w, names, [ptr(t) for t in keep])
    return keep


def _head_scalars(head):
    """A roll-out head (`DmolHead`, `GmmHead`, `GaussHead`) -> the five scalars the *_head entry points take in place of `num_mix,
    log_eps`: (head_kind, num_mix, log_eps, head_sd_beta, head_sd_eps)."""
    if isinstance(head, DmolHead):
        return 0, int(head.num_mix), float(head.log_eps), 0.0, 0.0
    if isinstance(head, GmmHead):
        return 1, int(head.num_mix), 0.0, float(head.sd_beta), float(head.sd_eps)
    if isinstance(head, GaussHead):
        return 2, 0, 0.0, float(head.sd_beta), float(head.sd_eps)
    raise TypeError(f"head: one of ops.DmolHead, ops.GmmHead, ops.GaussHead (got {type(head).__name__})")


@torch.no_grad()
def vrnn_decode(enc_lin, cell_params, dec_lin, lik_lin, x0, h0, eps, u, v, S, H, Z, R, num_mix, sd_eps, slope, log_eps, whole_chip=None,
                max_scratch_floats=None, head=None):  # fmt: skip
    """K1c: T = eps.shape[0] steps of ancestral sampling for all B utterances in one launch.  enc_lin / dec_lin: 3 nn.Linear each;
    cell_params in `_VRNN_PARAM_ORDER`; lik_lin the DMoL head's Linear.  x0 [B,S], h0 [B,R] or None, eps [T,B,Z],
    u [T,B,S,num_mix] / v [T,B,S] uniforms (None: the mode).  -> (x [B,T,S], h_n [B,R]).
    whole_chip: True = `blvm_vrnn_generate` (every layer of a step dealt over all CUs, B <= 128, any S >= 1), False =
    `blvm_vrnn_decode` (16 utterances per CU, S a multiple of 16), None = the former whenever it applies.
    max_scratch_floats (whole chip; None: MAX_SCRATCH_FLOATS): a roll-out whose scratch would be larger runs as consecutive launches
    of as many steps as fit — the same samples and state, bit for bit.
    head (None: the DMoL head `num_mix, log_eps`, through the entry points above): `DmolHead`, `GmmHead` (lik_lin [30,30], u as for
    DMoL, v standard normals) or `GaussHead` (lik_lin [2,2], u None, v [T,B,S] standard normals or None: the mean; whole chip only)
    through `blvm_vrnn_generate_head` / `blvm_vrnn_decode_head`; num_mix and log_eps are then not read."""
    from ._hip import VrnnDecodeWeights

    lib = load()
    T, B = eps.shape[0], x0.shape[0]
    dev = x0.device
    cp = [_f32c(p) for p in cell_params]
    cw = _pack_weights(cp)
    w = VrnnDecodeWeights()
    keep = _decode_weight_ptrs(w, "enc", enc_lin, dec_lin, lik_lin)  # noqa: F841  (alive until the calls below are enqueued)
    w.cell = ctypes.pointer(cw)
    x0, eps = _f32c(x0), _f32c(eps)
    h0 = _f32c(h0) if h0 is not None else None
    u = _f32c(u) if u is not None else None
    v = _f32c(v) if v is not None else None
    if whole_chip is None:
        whole_chip = B <= lib.blvm_pchain_max_batch()
    hs5 = None if head is None else _head_scalars(head)
    x = torch.empty(B, T, S, device=dev, dtype=torch.float32)
    hn = torch.empty(B, R, device=dev, dtype=torch.float32)
    if whole_chip:

        def call(t0, t1, state, xc, scratch):
            xs, hs = (x0, h0) if state is None else state
            uc, vc = (None if u is None else u[t0:t1]), (None if v is None else v[t0:t1])
            if hs5 is None:
                check(lib.blvm_vrnn_generate(ctypes.byref(w), ptr(xs), ptr(hs), ptr(eps[t0:t1]), ptr(uc), ptr(vc), t1 - t0, B, S, H, Z, R, num_mix,
                                             sd_eps, slope, log_eps, ptr(xc), ptr(hn), ptr(scratch), stream_ptr()), "blvm_vrnn_generate")  # fmt: skip
            else:
                check(lib.blvm_vrnn_generate_head(ctypes.byref(w), ptr(xs), ptr(hs), ptr(eps[t0:t1]), ptr(uc), ptr(vc), t1 - t0, B, S, H, Z, R, *hs5,
                                                  sd_eps, slope, ptr(xc), ptr(hn), ptr(scratch), stream_ptr()), "blvm_vrnn_generate_head")  # fmt: skip

        floats = ((lambda n: lib.blvm_vrnn_generate_scratch_floats(n, B, S, H, Z, R)) if hs5 is None
                  else (lambda n: lib.blvm_vrnn_generate_scratch_floats_head(n, B, S, H, Z, R, hs5[0])))  # fmt: skip
        _rollout(floats, T, max_scratch_floats, "vrnn_decode", x, call, lambda xc, t1: (xc[:, -1].contiguous(), hn.clone()))
        return x, hn
    scratch = torch.empty(lib.blvm_vrnn_decode_scratch_floats(S, H, Z, R), device=dev, dtype=torch.float32)
    if hs5 is None:
        check(lib.blvm_vrnn_decode(ctypes.byref(w), ptr(x0), ptr(h0), ptr(eps), ptr(u), ptr(v), T, B, S, H, Z, R, num_mix, sd_eps, slope,
                                   log_eps, ptr(x), ptr(hn), ptr(scratch), stream_ptr()), "blvm_vrnn_decode")  # fmt: skip
    else:
        check(lib.blvm_vrnn_decode_head(ctypes.byref(w), ptr(x0), ptr(h0), ptr(eps), ptr(u), ptr(v), T, B, S, H, Z, R, *hs5, sd_eps, slope,
                                        ptr(x), ptr(hn), ptr(scratch), stream_ptr()), "blvm_vrnn_decode_head")  # fmt: skip
    return x, hn


class _VRNNSeqFunction(torch.autograd.Function):
    """(enc, h0, eps, 28 params) -> decin [T'+1,B,H+R], kld [B], kld_fn [B]  (+ non-differentiable mu/sd/z).
    With the decoder's six parameters behind the 28 (`DecoderFold(head_gates=True)`, `blvm_vrnn_dec_bwd_fold` on) and a forward launch
    that folded all three layers, the node is the cell AND its decoder: a ninth output `dec` [T'*B, S*F] whose incoming gradient is
    that of the decoder's last pre-activation; the backward runs the decoder's data gradients inside the cell's backward launch
    (`blvm_vrnn_seq_bwd_dec`) or, where that does not fold, as the K6 products `_MLPFunction` runs, and then the decoder's three
    weight gradients.  (A node cannot return weight gradients that a later node's kernel will fill.)"""

    @staticmethod
    def forward(ctx, enc, h0, eps, x_sl_dev, cfg, dec, *params):
        """`dec`: None or a `DecoderFold`: the decoder is handed down and, where the launch folds it (blvm_vrnn_seq_fwd_dec), its
        three activations are left in `dec.given`."""
        Tp, B, X, H, Z, R, residual, sd_eps, stride, fn_floor = cfg
        enc, eps = _f32c(enc), _f32c(eps)
        params, dparams = tuple(_f32c(p) for p in params[:28]), tuple(_f32c(p) for p in params[28:])
        dev = enc.device
        lib = load()
        f32 = dict(device=dev, dtype=torch.float32)
        decin = torch.empty(Tp + 1, B, H + R, **f32)  # (the driver clears the phi-part of the extra row, which no step writes)
        mu_q, sd_q, mu_p, sd_p, z = (torch.empty(Tp, B, Z, **f32) for _ in range(5))
        w = _pack_weights(params)
        if dec is None:
            reserve = torch.empty(lib.blvm_vrnn_reserve_floats(Tp, B, X, H, Z, R), **f32)
            _tick("fwd_begin")
            check(
                lib.blvm_vrnn_seq_fwd(w, ptr(enc), ptr(_f32c(h0)) if h0 is not None else None, ptr(eps), Tp, B, X, H, Z, R,
                                      int(residual), sd_eps, ptr(decin), ptr(mu_q), ptr(sd_q), ptr(mu_p), ptr(sd_p), ptr(z),
                                      ptr(reserve), stream_ptr()),
                "blvm_vrnn_seq_fwd",
            )  # fmt: skip
        else:
            keep = [_f32c(t.detach()) for lin in dec.layers for t in (lin.weight, lin.bias)]
            DH, SF = keep[0].shape[0], keep[4].shape[0]
            ys = [torch.empty(Tp * B, n, **f32) for n in (DH, DH, SF)]
            three = ctypes.c_void_p * 3  # host arrays of device pointers: weights, biases, activations
            dw, db, dy = three(*(ptr(t) for t in keep[0::2])), three(*(ptr(t) for t in keep[1::2])), three(*(ptr(t) for t in ys))
            reserve = torch.empty(lib.blvm_vrnn_fwd_reserve_floats(Tp, B, X, H, Z, R, DH, SF), **f32)
            folded = ctypes.c_int(0)
            _tick("fwd_begin")
            check(
                lib.blvm_vrnn_seq_fwd_dec(w, ptr(enc), ptr(_f32c(h0)) if h0 is not None else None, ptr(eps), Tp, B, X, H, Z, R,
                                          int(residual), sd_eps, ptr(decin), ptr(mu_q), ptr(sd_q), ptr(mu_p), ptr(sd_p), ptr(z),
                                          ptr(reserve), dw, db, dy, DH, SF, dec.slope, ctypes.byref(folded), stream_ptr()),
                "blvm_vrnn_seq_fwd_dec",
            )  # fmt: skip
            dec.given = tuple(ys[: folded.value]) if folded.value else None  # (2: the last layer is left to the caller)
        joint = dec is not None and len(dparams) == 6 and dec.given is not None and len(dec.given) == 3
        _tick("fwd_end")
        kld = torch.zeros(B, device=dev, dtype=torch.float64)
        kld_fn = torch.zeros(B, device=dev, dtype=torch.float64)
        check(
            lib.blvm_kl_fwd(ptr(mu_q), ptr(sd_q), ptr(mu_p), ptr(sd_p), LAYOUT_TIME_MAJOR, ptr(x_sl_dev), B, Tp, Z, stride,
                            fn_floor, ptr(kld), ptr(kld_fn), stream_ptr()),
            "blvm_kl_fwd",
        )  # fmt: skip
        ctx.cfg = cfg
        ctx.has_h0 = h0 is not None
        ctx.joint, ctx.n_dpar, ctx.dec_slope = joint, len(dparams), dec.slope if joint else 0.0
        ctx.save_for_backward(enc, eps, x_sl_dev, decin, mu_q, sd_q, mu_p, sd_p, z, reserve, *params, *((*dparams, ys[0], ys[1]) if joint else ()))
        ctx.mark_non_differentiable(mu_q, sd_q, mu_p, sd_p, z)
        ctx.set_materialize_grads(False)  # (else autograd fills a [T',B,Z] zero gradient per statistics output: 16 MB each at [64,16000])
        return decin, kld, kld_fn, mu_q, sd_q, mu_p, sd_p, z, (ys[2] if joint else None)

    @staticmethod
    def backward(ctx, d_decin, g_kld, g_kld_fn, *rest):
        Tp, B, X, H, Z, R, residual, sd_eps, stride, fn_floor = ctx.cfg
        enc, eps, x_sl_dev, decin, mu_q, sd_q, mu_p, sd_p, z, reserve, *params = ctx.saved_tensors
        dev = enc.device
        lib = load()
        f32 = dict(device=dev, dtype=torch.float32)
        c_raw = _grad_f32(g_kld) if g_kld is not None else None
        c_fn = _grad_f32(g_kld_fn) if g_kld_fn is not None else None
        d_dec = rest[5] if ctx.joint else None
        dgrads = (None,) * ctx.n_dpar
        if d_dec is not None:
            # the cell and its decoder: the decoder's data gradients inside the launch where it folds, else as K6 in front of it
            params, (W1, b1, W2, b2, W3, b3, y1, y2) = params[:28], params[28:]
            dz3, M, DH, SF, slope = _f32c(d_dec), Tp * B, W2.shape[0], W3.shape[0], ctx.dec_slope
            dy2, dy1 = torch.empty(M, DH, **f32), torch.empty(M, DH, **f32)
            grads = _zeros_like_many(params)
            d_enc = torch.empty_like(enc) if ctx.needs_input_grad[0] else None  # (not asked for: the library skips its products)
            d_h0 = torch.empty(B, R, **f32) if ctx.has_h0 else None
            w, g = _pack_weights(params), _pack_weights(grads, _hip.VrnnGrads)
            folded = ctypes.c_int(0)
            if d_decin is None:
                ws = torch.empty(lib.blvm_vrnn_bwd_dec_workspace_floats(Tp, B, X, H, Z, R, DH, SF), **f32)
                dw = (ctypes.c_void_p * 3)(ptr(W1), ptr(W2), ptr(W3))
                _tick("bwd_begin")
                check(
                    lib.blvm_vrnn_seq_bwd_dec(w, ptr(enc), ptr(eps), ptr(decin), ptr(mu_q), ptr(sd_q), ptr(mu_p), ptr(sd_p), ptr(z),
                                              ptr(reserve), ptr(x_sl_dev), ptr(c_raw), ptr(c_fn), stride, fn_floor, Tp, B, X, H, Z, R,
                                              int(residual), sd_eps, ptr(d_enc), ptr(d_h0), g, ptr(ws), ptr(dz3), ptr(y1), ptr(y2), dw,
                                              ptr(dy2), ptr(dy1), DH, SF, slope, ctypes.byref(folded), stream_ptr()),
                    "blvm_vrnn_seq_bwd_dec",
                )  # fmt: skip
            if not folded.value:  # nothing was done: the data gradients as `_MLPFunction._backward` runs them, then the cell
                gemm(0, 1, M, DH, SF, dz3, SF, W3, DH, dy2, DH, slope=slope, gate=y2, ldg=DH)
                gemm(0, 1, M, DH, DH, dy2, DH, W2, DH, dy1, DH, slope=slope, gate=y1, ldg=DH)
                dx = torch.empty(M, H + R, **f32)
                gemm(0, 1, M, H + R, DH, dy1, DH, W1, H + R, dx, H + R, slope=slope)
                dd = torch.zeros_like(decin)
                dd[:Tp] = dx.view(Tp, B, H + R)
                if d_decin is not None:
                    dd = dd + _f32c(d_decin)
                ws = torch.empty(lib.blvm_vrnn_bwd_workspace_floats(Tp, B, X, H, Z, R), **f32)
                _tick("bwd_begin")
                check(
                    lib.blvm_vrnn_seq_bwd(w, ptr(enc), ptr(eps), ptr(decin), ptr(mu_q), ptr(sd_q), ptr(mu_p), ptr(sd_p), ptr(z),
                                          ptr(reserve), ptr(dd), ptr(x_sl_dev), ptr(c_raw), ptr(c_fn), stride, fn_floor, Tp, B,
                                          X, H, Z, R, int(residual), sd_eps, ptr(d_enc), ptr(d_h0), g, ptr(ws), stream_ptr()),
                    "blvm_vrnn_seq_bwd",
                )  # fmt: skip
            _tick("bwd_end")
            # the decoder's weight and bias gradients: one grouped launch, as `_MLPFunction._backward` (views of one zero-filled buffer)
            dpar = (W1, b1, W2, b2, W3, b3)
            want = [ctx.needs_input_grad[6 + 28 + i] for i in range(6)]
            sizes = [(dpar[i].numel() + 3) // 4 * 4 if want[i] else 0 for i in range(6)]
            flat = torch.zeros(sum(sizes), **f32)
            views, off = [], 0
            for i in range(6):
                views.append(flat[off : off + dpar[i].numel()].view(dpar[i].shape) if want[i] else None)
                off += sizes[i]
            x2d = decin[:Tp].view(M, H + R)
            wgrad_group([(dz3, y2, views[4], views[5]), (dy2, y1, views[2], views[3]), (dy1, x2d, views[0], views[1])], M)
            return (d_enc, d_h0, None, None, None, None, *grads, *views)
        params = params[:28]  # (a decoder whose output went unused: no gradient)
        d_decin = _f32c(d_decin) if d_decin is not None else torch.zeros_like(decin)
        grads = _zeros_like_many(params)
        d_enc = torch.empty_like(enc) if ctx.needs_input_grad[0] else None  # (not asked for: the library skips its products)
        d_h0 = torch.empty(B, R, **f32) if ctx.has_h0 else None
        ws = torch.empty(lib.blvm_vrnn_bwd_workspace_floats(Tp, B, X, H, Z, R), **f32)
        w, g = _pack_weights(params), _pack_weights(grads, _hip.VrnnGrads)
        _tick("bwd_begin")
        check(
            lib.blvm_vrnn_seq_bwd(w, ptr(enc), ptr(eps), ptr(decin), ptr(mu_q), ptr(sd_q), ptr(mu_p), ptr(sd_p), ptr(z),
                                  ptr(reserve), ptr(d_decin), ptr(x_sl_dev), ptr(c_raw), ptr(c_fn), stride, fn_floor, Tp, B,
                                  X, H, Z, R, int(residual), sd_eps, ptr(d_enc), ptr(d_h0), g, ptr(ws), stream_ptr()),
            "blvm_vrnn_seq_bwd",
        )  # fmt: skip
        _tick("bwd_end")
        return (d_enc, d_h0, None, None, None, None, *grads, *dgrads)


def vrnn_sequence(enc, h0, eps, x_sl_dev, params: Sequence[torch.Tensor], X, H, Z, R, residual_posterior, stride,
                  free_nats=0.0, sd_eps=1e-6, decoder=None):  # fmt: skip
    """Run the VRNN cell over enc [T',B,X].  `params` in `_VRNN_PARAM_ORDER`.  Returns
    (decin [T'+1,B,H+R], kld [B] f64, kld_fn [B] f64, mu_q, sd_q, mu_p, sd_p, z).
    `decoder`: a `DecoderFold` — the decoder MLP on decin[:T'] handed down so that the forward launch can run it on its spare
    workgroups; its `given` is set to the three activations [T'*B, .], or to None where the launch did not fold the decoder."""
    Tp, B, _ = enc.shape
    fn_floor = float(free_nats) / Z if free_nats else 0.0
    cfg = (Tp, B, X, H, Z, R, int(residual_posterior), float(sd_eps), int(stride), fn_floor)  # 0 plain, 1 residual, 3 generate
    if decoder is None:
        return _VRNNSeqFunction.apply(enc, h0, eps, x_sl_dev, cfg, None, *params)[:8]
    decoder.given = decoder.dec = None
    dparams = ()
    if decoder.head_gates and load().blvm_vrnn_dec_bwd_fold(-1):  # the cell's node takes the decoder in (where the forward folds it)
        dparams = tuple(t for lin in decoder.layers for t in (lin.weight, lin.bias))
    *out, decoder.dec = _VRNNSeqFunction.apply(enc, h0, eps, x_sl_dev, cfg, decoder, *params, *dparams)
    return tuple(out)


class DecoderFold:
    """The VRNN decoder MLP handed down to the cell's forward (`vrnn_sequence`): `layers` = its three nn.Linear, LeakyReLU(`slope`)
    after each.  After the call `given` holds the three activations (plain tensors outside the graph; `mlp_given` builds the decoder's
    autograd node from them) where the launch computed them, else None.
    `head_gates`: the caller will feed the decoder's output to a fused likelihood head whose backward returns the gradient of the
    last PRE-activation (`mlp_dmol_log_prob(..., dec_node=)`).  Then, with `blvm_vrnn_dec_bwd_fold` on and a forward launch that
    folded the whole decoder, `dec` holds that output as an output of the cell's own node (the decoder's backward then runs with the
    cell's, `_VRNNSeqFunction`) and the caller builds no decoder node; else `dec` is None."""

    def __init__(self, layers, slope: float = LEAKY_SLOPE, head_gates: bool = False):
        self.layers, self.slope, self.given, self.head_gates, self.dec = list(layers), float(slope), None, bool(head_gates), None


# ----------------------------------------------------------------------------------------------------------------------
# K4: LSTM over a sequence (packed-sequence semantics through `lens`)
# ----------------------------------------------------------------------------------------------------------------------


class _LSTMSeqFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inp, h0, c0, lens_dev, Wih, Whh, bih, bhh):
        inp, Wih, Whh, bih, bhh = (_f32c(t) for t in (inp, Wih, Whh, bih, bhh))
        T, B, I = inp.shape
        H = Whh.shape[1]
        lib = load()
        f32 = dict(device=inp.device, dtype=torch.float32)
        out = torch.empty(T, B, H, **f32)
        hn, cn = torch.empty(B, H, **f32), torch.empty(B, H, **f32)
        reserve = torch.empty(lib.blvm_lstm_reserve_floats(T, B, H), **f32)
        check(
            lib.blvm_lstm_seq_fwd(ptr(Wih), ptr(Whh), ptr(bih), ptr(bhh), ptr(inp), ptr(_f32c(h0)) if h0 is not None else None,
                                  ptr(_f32c(c0)) if c0 is not None else None, ptr(lens_dev), T, B, I, H, ptr(out), ptr(hn), ptr(cn),
                                  ptr(reserve), stream_ptr()),
            "blvm_lstm_seq_fwd",
        )  # fmt: skip
        ctx.dims = (T, B, I, H)
        ctx.has_state = (h0 is not None, c0 is not None)
        ctx.save_for_backward(inp, Wih, Whh, reserve)
        ctx.mark_non_differentiable(hn, cn)
        return out, hn, cn

    @staticmethod
    def backward(ctx, d_out, _dhn, _dcn):
        T, B, I, H = ctx.dims
        inp, Wih, Whh, reserve = ctx.saved_tensors
        lib = load()
        f32 = dict(device=inp.device, dtype=torch.float32)
        d_out = _f32c(d_out)
        d_in = torch.empty_like(inp) if ctx.needs_input_grad[0] else None
        d_h0 = torch.empty(B, H, **f32) if ctx.has_state[0] and ctx.needs_input_grad[1] else None
        d_c0 = torch.empty(B, H, **f32) if ctx.has_state[1] and ctx.needs_input_grad[2] else None
        dWih, dWhh = torch.zeros_like(Wih), torch.zeros_like(Whh)
        dbih, dbhh = torch.zeros(4 * H, **f32), torch.zeros(4 * H, **f32)
        ws = torch.empty(lib.blvm_lstm_bwd_workspace_floats(T, B, H), **f32)
        check(
            lib.blvm_lstm_seq_bwd(ptr(Wih), ptr(Whh), ptr(inp), ptr(reserve), ptr(d_out), T, B, I, H, ptr(d_in), ptr(d_h0),
                                  ptr(d_c0), ptr(dWih), ptr(dWhh), ptr(dbih), ptr(dbhh), ptr(ws), stream_ptr()),
            "blvm_lstm_seq_bwd",
        )  # fmt: skip
        return d_in, d_h0, d_c0, None, dWih, dWhh, dbih, dbhh


def lstm_sequence(inp, h0, c0, lens_dev, Wih, Whh, bih, bhh):
    """inp [T,B,I] -> (out [T,B,H] zero past each row's length, h_n, c_n [B,H])."""
    return _LSTMSeqFunction.apply(inp, h0, c0, lens_dev, Wih, Whh, bih, bhh)


class _LSTMBidirSeqFunction(torch.autograd.Function):
    """K4b: both directions of one bidirectional layer in one launch.  forward returns None where the call does not apply."""

    @staticmethod
    def forward(ctx, inp, lens_dev, Wih_f, Whh_f, bih_f, bhh_f, Wih_r, Whh_r, bih_r, bhh_r):
        inp, *params = (_f32c(t) for t in (inp, Wih_f, Whh_f, bih_f, bhh_f, Wih_r, Whh_r, bih_r, bhh_r))
        T, B, I = inp.shape
        H = params[1].shape[1]
        lib = load()
        if not lib.blvm_lstm_bidir_applies(T, B, H):  # asked first: nothing is allocated for a call that would be refused
            return None
        f32 = dict(device=inp.device, dtype=torch.float32)
        out = torch.empty(T, B, 2 * H, **f32)
        reserve = torch.empty(lib.blvm_lstm_bidir_reserve_floats(T, B, H), **f32)
        rc = lib.blvm_lstm_bidir_fwd(*(ptr(p) for p in params), ptr(inp), ptr(lens_dev), T, B, I, H, ptr(out), ptr(reserve), stream_ptr())
        if rc == BLVM_NOT_APPLICABLE:
            return None
        check(rc, "blvm_lstm_bidir_fwd")
        ctx.dims = (T, B, I, H)
        ctx.save_for_backward(inp, lens_dev, reserve, *params)
        return out

    @staticmethod
    def backward(ctx, d_out):
        T, B, I, H = ctx.dims
        inp, lens_dev, reserve, Wih_f, Whh_f, bih_f, bhh_f, Wih_r, Whh_r, bih_r, bhh_r = ctx.saved_tensors
        lib = load()
        d_out = _f32c(d_out)
        d_in = torch.empty_like(inp) if ctx.needs_input_grad[0] else None
        grads = [torch.zeros_like(p) for p in (Wih_f, Whh_f, bih_f, bhh_f, Wih_r, Whh_r, bih_r, bhh_r)]
        ws = torch.empty(lib.blvm_lstm_bidir_bwd_workspace_floats(T, B, H), device=inp.device, dtype=torch.float32)
        check(
            lib.blvm_lstm_bidir_bwd(ptr(Wih_f), ptr(Whh_f), ptr(Wih_r), ptr(Whh_r), ptr(inp), ptr(lens_dev), ptr(reserve), ptr(d_out),
                                    T, B, I, H, ptr(d_in), *(ptr(g) for g in grads), ptr(ws), stream_ptr()),
            "blvm_lstm_bidir_bwd",
        )  # fmt: skip
        return (d_in, None, *grads)


def lstm_bidir_sequence(inp, lens_dev, fwd_params, rev_params):
    """inp [T,B,I], lens_dev [B] int32 on the device, each params = (Wih [4H,I], Whh [4H,H], bih [4H], bhh [4H]) of one direction
    -> out [T,B,2H] (forward | reverse halves, zeros past each row's length), both directions in one launch; or None where the
    one-launch form does not take the shape (nothing was launched: run two `lstm_sequence` calls)."""
    return _LSTMBidirSeqFunction.apply(inp, lens_dev, *fwd_params, *rev_params)


def lstm_bidir_path_counts():
    """(forward, backward) calls of this process that ran the one-launch bidirectional kernels."""
    out = (ctypes.c_ulonglong * 2)()
    check(load().blvm_lstm_bidir_path_counts(out), "blvm_lstm_bidir_path_counts")
    return int(out[0]), int(out[1])


def lstm_decode_weights(emb_lin, lstm, dec_lin, lik_lin):
    """-> (struct BlvmLstmDecodeWeights, what must stay alive while it is used)."""
    L = lstm.num_layers
    lk = [[_f32c(getattr(lstm, f"{n}_l{l}")) for l in range(L)] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    arrays = [(ctypes.c_void_p * L)(*[t.data_ptr() for t in ts]) for ts in lk]  # host arrays of device pointers
    w = _hip.LstmDecodeWeights()
    keep = _decode_weight_ptrs(w, "emb", emb_lin, dec_lin, lik_lin)
    w.wih, w.whh, w.bih, w.bhh = (ctypes.cast(a, ctypes.POINTER(ctypes.c_void_p)) for a in arrays)
    return w, (keep, lk, arrays)


def lstm_generate(emb_lin, lstm, dec_lin, lik_lin, x0, h0, c0, u, v, S, H, num_mix, log_eps, T=None, max_scratch_floats=None):
    """K4c: T = u.shape[0] steps of sampling from LSTMAudio for all B <= 128 utterances in one persistent launch.  emb_lin / dec_lin:
    3 nn.Linear each; lstm: the nn.LSTM (parameter container, input size H); lik_lin the DMoL head's Linear.  x0 [B,S]; h0, c0
    [num_layers,B,H] or None (zeros); u [T,B,S,num_mix], v [T,B,S] the sampler's draws (both None: the mode, `T` then says how many
    steps).  Any S >= 1; H a multiple of 16.  -> (x [B,T,S], h_n, c_n [num_layers,B,H]).
    max_scratch_floats (None: MAX_SCRATCH_FLOATS): a roll-out whose scratch would be larger runs as consecutive launches of as many
    steps as fit — the same samples and states, bit for bit."""
    lib = load()
    L, B, dev = lstm.num_layers, x0.shape[0], x0.device
    if (u is None) != (v is None) or (u is None and T is None):
        raise ValueError("lstm_generate: u and v are given together; the mode (neither) needs T")
    T = int(T) if u is None else u.shape[0]
    w, _keep = lstm_decode_weights(emb_lin, lstm, dec_lin, lik_lin)
    x0 = _f32c(x0)
    h0 = _f32c(h0) if h0 is not None else None
    c0 = _f32c(c0) if c0 is not None else None
    u, v = (None, None) if u is None else (_f32c(u), _f32c(v))
    f32 = dict(device=dev, dtype=torch.float32)
    x, hn, cn = torch.empty(B, T, S, **f32), torch.empty(L, B, H, **f32), torch.empty(L, B, H, **f32)

    def call(t0, t1, state, xc, scratch):
        xs, hs, cs = (x0, h0, c0) if state is None else state
        uc, vc = (None, None) if u is None else (u[t0:t1], v[t0:t1])
        check(lib.blvm_lstm_generate_any_stack(ctypes.byref(w), ptr(xs), ptr(hs), ptr(cs), ptr(uc), ptr(vc), t1 - t0, B, S, H, L, num_mix, log_eps, ptr(xc),
                                               ptr(hn), ptr(cn), ptr(scratch), stream_ptr()), "blvm_lstm_generate_any_stack")  # fmt: skip

    _rollout(lambda n: lib.blvm_lstm_generate_scratch_floats(n, B, S, H, L), T, max_scratch_floats, "lstm_generate", x, call,
             lambda xc, t1: (xc[:, -1].contiguous(), hn.clone(), cn.clone()))  # fmt: skip
    return x, hn, cn


# ----------------------------------------------------------------------------------------------------------------------
# K2: GRU over a sequence, optionally reversed per row (reverse_sequences folded into the kernel's index map)
# ----------------------------------------------------------------------------------------------------------------------


class _GRUSeqFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inp, h0, lens_dev, reverse, Wih, Whh, bih, bhh):
        inp, Wih, Whh, bih, bhh = (_f32c(t) for t in (inp, Wih, Whh, bih, bhh))
        T, B, I = inp.shape
        R = Whh.shape[1]
        lib = load()
        f32 = dict(device=inp.device, dtype=torch.float32)
        out = torch.empty(T, B, R, **f32)
        hn = torch.empty(B, R, **f32)
        reserve = torch.empty(lib.blvm_gru_reserve_floats(T, B, R), **f32)
        check(
            lib.blvm_gru_seq_fwd(ptr(Wih), ptr(Whh), ptr(bih), ptr(bhh), ptr(inp), I, ptr(_f32c(h0)) if h0 is not None else None,
                                 ptr(lens_dev), int(reverse), T, B, I, R, ptr(out), B * R, R, ptr(hn), ptr(reserve), stream_ptr()),
            "blvm_gru_seq_fwd",
        )  # fmt: skip
        ctx.dims = (T, B, I, R, int(reverse))
        ctx.has_h0 = h0 is not None
        ctx.save_for_backward(inp, Wih, Whh, reserve, lens_dev)
        ctx.mark_non_differentiable(hn)
        return out, hn

    @staticmethod
    def backward(ctx, d_out, _dhn):
        T, B, I, R, reverse = ctx.dims
        inp, Wih, Whh, reserve, lens_dev = ctx.saved_tensors
        lib = load()
        f32 = dict(device=inp.device, dtype=torch.float32)
        d_out = _f32c(d_out)
        d_in = torch.empty_like(inp) if ctx.needs_input_grad[0] else None
        d_h0 = torch.empty(B, R, **f32) if ctx.has_h0 and ctx.needs_input_grad[1] else None
        dWih, dWhh = torch.zeros_like(Wih), torch.zeros_like(Whh)
        dbih, dbhh = torch.zeros(3 * R, **f32), torch.zeros(3 * R, **f32)
        ws = torch.empty(lib.blvm_gru_bwd_workspace_floats(T, B, R), **f32)
        check(
            lib.blvm_gru_seq_bwd(ptr(Wih), ptr(Whh), ptr(inp), I, ptr(lens_dev), reverse, ptr(reserve), ptr(d_out), B * R, R, T, B,
                                 I, R, ptr(d_in), I, 0, ptr(d_h0), ptr(dWih), ptr(dWhh), ptr(dbih), ptr(dbhh), ptr(ws),
                                 stream_ptr()),
            "blvm_gru_seq_bwd",
        )  # fmt: skip
        return d_in, d_h0, None, None, dWih, dWhh, dbih, dbhh


def gru_sequence(inp, h0, Wih, Whh, bih, bhh, lens_dev=None, reverse=False):
    """inp [T,B,I] -> (out [T,B,R], h_n [B,R]).  reverse=True: per-row time reversal that leaves right padding in
    place (needs lens_dev [B] int32) — equivalent to reverse_sequences -> GRU -> reverse_sequences."""
    return _GRUSeqFunction.apply(inp, h0, lens_dev, reverse, Wih, Whh, bih, bhh)


# ----------------------------------------------------------------------------------------------------------------------
# K3: SRNN latent chain
# ----------------------------------------------------------------------------------------------------------------------

_SRNN_PARAM_ORDER = (
    ["prior_w0", "prior_b0", "prior_w1", "prior_b1", "prior_w2", "prior_b2", "prior_hw", "prior_hb"]
    + ["post_w0", "post_b0", "post_w1", "post_b1", "post_w2", "post_b2", "post_hw", "post_hb"]
)


def srnn_generate(enc_lin, gru, chain_params, dec_lin, lik_lin, x0, d0, z0, eps, u, v, S, H, Z, R, num_mix, sd_eps, slope, log_eps,
                  max_scratch_floats=None, head=None):  # fmt: skip
    """K3c: T = eps.shape[0] steps of ancestral sampling from SRNNAudio for all B <= 128 utterances in one persistent launch.
    enc_lin / dec_lin: 3 nn.Linear each; gru: the forward nn.GRU (parameter container); chain_params in `_SRNN_PARAM_ORDER`;
    lik_lin the DMoL head's Linear.  x0 [B,S]; d0 [B,R], z0 [B,Z] or None; eps [T,B,Z]; u [T,B,S,num_mix] / v [T,B,S] (None: the
    mode).  Any S >= 1; H, Z, R multiples of 16.  -> (x [B,T,S], d_T [B,R], z [T,B,Z]).
    max_scratch_floats (None: MAX_SCRATCH_FLOATS): a roll-out whose scratch would be larger runs as consecutive launches of as many
    steps as fit — the same samples, latents and state, bit for bit.
    head (None: the DMoL head `num_mix, log_eps`, through `blvm_srnn_generate`): `DmolHead`, `GmmHead` or `GaussHead` as in
    `vrnn_decode`, through `blvm_srnn_generate_head`."""
    lib = load()
    T, B = eps.shape[0], x0.shape[0]
    dev = x0.device
    hs5 = None if head is None else _head_scalars(head)
    gk = [_f32c(t) for t in (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)]
    cp = [_f32c(p) for p in chain_params]
    cw = _pack(_hip.SrnnWeights, _SRNN_PARAM_ORDER, cp)
    w = _hip.SrnnDecodeWeights()
    keep = _decode_weight_ptrs(w, "enc", enc_lin, dec_lin, lik_lin)  # noqa: F841  (alive until the calls below are enqueued)
    w.gru_wih, w.gru_whh, w.gru_bih, w.gru_bhh = (ptr(t) for t in gk)
    w.chain = ctypes.pointer(cw)
    x0, eps = _f32c(x0), _f32c(eps)
    d0 = _f32c(d0) if d0 is not None else None
    z0 = _f32c(z0) if z0 is not None else None
    u = _f32c(u) if u is not None else None
    v = _f32c(v) if v is not None else None
    f32 = dict(device=dev, dtype=torch.float32)
    x, dn, zs = torch.empty(B, T, S, **f32), torch.empty(B, R, **f32), torch.empty(T, B, Z, **f32)

    def call(t0, t1, state, xc, scratch):
        xs, ds, z_prev = (x0, d0, z0) if state is None else state
        uc, vc = (None if u is None else u[t0:t1]), (None if v is None else v[t0:t1])
        if hs5 is None:
            check(lib.blvm_srnn_generate(ctypes.byref(w), ptr(xs), ptr(ds), ptr(z_prev), ptr(eps[t0:t1]), ptr(uc), ptr(vc), t1 - t0, B, S, H, Z, R, num_mix,
                                         sd_eps, slope, log_eps, ptr(xc), ptr(dn), ptr(zs[t0:t1]), ptr(scratch), stream_ptr()), "blvm_srnn_generate")  # fmt: skip
        else:
            check(lib.blvm_srnn_generate_head(ctypes.byref(w), ptr(xs), ptr(ds), ptr(z_prev), ptr(eps[t0:t1]), ptr(uc), ptr(vc), t1 - t0, B, S, H, Z, R, *hs5,
                                              sd_eps, slope, ptr(xc), ptr(dn), ptr(zs[t0:t1]), ptr(scratch), stream_ptr()), "blvm_srnn_generate_head")  # fmt: skip

    floats = ((lambda n: lib.blvm_srnn_generate_scratch_floats(n, B, S, H, Z, R)) if hs5 is None
              else (lambda n: lib.blvm_srnn_generate_scratch_floats_head(n, B, S, H, Z, R, hs5[0])))  # fmt: skip
    _rollout(floats, T, max_scratch_floats, "srnn_generate", x, call, lambda xc, t1: (xc[:, -1].contiguous(), dn.clone(), zs[t1 - 1]))
    return x, dn, zs


class _SRNNLatentFunction(torch.autograd.Function):
    """(d, a, z0, eps, 16 params) -> zs [T'+1,B,Z], kld [B], kld_fn [B]  (+ non-differentiable mu/sd)."""

    @staticmethod
    def forward(ctx, d, a, z0, eps, x_sl_dev, cfg, *params):
        Tp, B, H, Z, R, residual, sd_eps, slope, stride, fn_floor = cfg
        d, a, eps = _f32c(d), _f32c(a), _f32c(eps)
        params = tuple(_f32c(p) for p in params)
        lib = load()
        f32 = dict(device=d.device, dtype=torch.float32)
        zs = torch.empty(Tp + 1, B, Z, **f32)
        mu_q, sd_q, mu_p, sd_p = (torch.empty(Tp, B, Z, **f32) for _ in range(4))
        reserve = torch.empty(lib.blvm_srnn_reserve_floats(Tp, B, H, Z, R), **f32)
        w = _pack(_hip.SrnnWeights, _SRNN_PARAM_ORDER, params)
        _tick("fwd_begin")
        check(
            lib.blvm_srnn_latent_fwd(w, ptr(d), ptr(a), ptr(_f32c(z0)) if z0 is not None else None, ptr(eps),
                                     Tp, B, H, Z, R, int(residual), sd_eps, slope, ptr(zs), ptr(mu_q), ptr(sd_q), ptr(mu_p),
                                     ptr(sd_p), ptr(reserve), stream_ptr()),
            "blvm_srnn_latent_fwd",
        )  # fmt: skip
        _tick("fwd_end")
        kld = torch.zeros(B, device=d.device, dtype=torch.float64)
        kld_fn = torch.zeros(B, device=d.device, dtype=torch.float64)
        check(
            lib.blvm_kl_fwd(ptr(mu_q), ptr(sd_q), ptr(mu_p), ptr(sd_p), LAYOUT_TIME_MAJOR, ptr(x_sl_dev), B, Tp, Z, stride,
                            fn_floor, ptr(kld), ptr(kld_fn), stream_ptr()),
            "blvm_kl_fwd",
        )  # fmt: skip
        ctx.cfg = cfg
        ctx.has_z0 = z0 is not None
        ctx.save_for_backward(d, a, eps, x_sl_dev, zs, mu_q, sd_q, mu_p, sd_p, reserve, *params)
        ctx.mark_non_differentiable(mu_q, sd_q, mu_p, sd_p)
        ctx.set_materialize_grads(False)  # (else autograd fills a [T',B,Z] zero gradient per statistics output: 16 MB each at [64,16000])
        return zs, kld, kld_fn, mu_q, sd_q, mu_p, sd_p

    @staticmethod
    def backward(ctx, d_zs, g_kld, g_kld_fn, *_unused):
        Tp, B, H, Z, R, residual, sd_eps, slope, stride, fn_floor = ctx.cfg
        d, a, eps, x_sl_dev, zs, mu_q, sd_q, mu_p, sd_p, reserve, *params = ctx.saved_tensors
        lib = load()
        f32 = dict(device=d.device, dtype=torch.float32)
        d_zs = _f32c(d_zs) if d_zs is not None else torch.zeros_like(zs)
        d_z = d_zs[1:]  # rows 1.. are the sampled latents; row 0 is z0 (its direct gradient is added below)
        c_raw = _grad_f32(g_kld) if g_kld is not None else None
        c_fn = _grad_f32(g_kld_fn) if g_kld_fn is not None else None
        grads = _zeros_like_many(params)
        d_d, d_a = torch.empty_like(d), torch.empty_like(a)
        d_z0 = torch.empty(B, Z, **f32) if ctx.has_z0 else None
        ws = torch.empty(lib.blvm_srnn_bwd_workspace_floats(Tp, B, H, Z, R), **f32)
        w, g = _pack(_hip.SrnnWeights, _SRNN_PARAM_ORDER, params), _pack(_hip.SrnnGrads, _SRNN_PARAM_ORDER, grads)
        _tick("bwd_begin")
        check(
            lib.blvm_srnn_latent_bwd(w, ptr(d), ptr(a), ptr(eps), ptr(zs), ptr(mu_q), ptr(sd_q), ptr(mu_p),
                                     ptr(sd_p), ptr(reserve), ptr(d_z), ptr(x_sl_dev), ptr(c_raw), ptr(c_fn), stride, fn_floor,
                                     Tp, B, H, Z, R, int(residual), sd_eps, slope, ptr(d_d), ptr(d_a), ptr(d_z0),
                                     g, ptr(ws), stream_ptr()),
            "blvm_srnn_latent_bwd",
        )  # fmt: skip
        _tick("bwd_end")
        if d_z0 is not None:
            d_z0 = d_z0 + d_zs[0]
        return (d_d, d_a, d_z0, None, None, None, *grads)


def srnn_latent_chain(d, a, z0, eps, x_sl_dev, params, H, Z, R, residual_posterior, stride, free_nats=0.0, sd_eps=1e-6,
                      slope=LEAKY_SLOPE):  # fmt: skip
    """d, a [T',B,R] -> (zs [T'+1,B,Z] with zs[0]=z0, kld [B] f64, kld_fn [B] f64, mu_q, sd_q, mu_p, sd_p)."""
    Tp, B, _ = d.shape
    fn_floor = float(free_nats) / Z if free_nats else 0.0
    cfg = (Tp, B, H, Z, R, int(residual_posterior), float(sd_eps), float(slope), int(stride), fn_floor)  # 3: generate
    return _SRNNLatentFunction.apply(d, a, z0, eps, x_sl_dev, cfg, *params)


# ----------------------------------------------------------------------------------------------------------------------
# K10: WaveNet — dilated causal convolution (k=2) and the gated residual stack
# ----------------------------------------------------------------------------------------------------------------------


class _ScaleActFunction(torch.autograd.Function):
    """y = act(scale * x) (ReLU / LeakyReLU) element-wise."""

    @staticmethod
    def forward(ctx, x, scale, slope):
        x = _f32c(x)
        y = torch.empty_like(x)
        check(load().blvm_scale_act_f32(ptr(x), scale, slope, ptr(y), x.numel(), stream_ptr()), "blvm_scale_act_f32")
        ctx.save_for_backward(y)
        ctx.cfg = (scale, slope)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        scale, slope = ctx.cfg
        dy = _f32c(dy)
        dz = torch.empty_like(dy)
        check(load().blvm_act_bwd_f32(ptr(dy), ptr(y), slope, ptr(dz), dz.numel(), stream_ptr()), "blvm_act_bwd_f32")
        if scale != 1.0:  # chain rule through the scale: one more streaming pass over dz
            dx = torch.empty_like(dz)
            check(load().blvm_scale_act_f32(ptr(dz), scale, 1.0, ptr(dx), dz.numel(), stream_ptr()), "blvm_scale_act_f32")
            dz = dx
        return dz, None, None


def scale_act(x, scale: float = 1.0, slope: float = 0.0):
    return _ScaleActFunction.apply(x, float(scale), float(slope))


class _Conv1dK2Function(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, b, dilation):
        x, W, b = _f32c(x), _f32c(W), _f32c(b)
        L, B, Cin = x.shape
        Cout = W.shape[0]
        lib = load()
        f32 = dict(device=x.device, dtype=torch.float32)
        out = torch.empty(L - dilation, B, Cout, **f32)
        ws = torch.empty(lib.blvm_conv1d_k2_workspace_floats(Cin, Cout), **f32)
        check(lib.blvm_conv1d_k2_fwd(ptr(x), ptr(W), ptr(b), L, B, Cin, Cout, dilation, ptr(out), ptr(ws), stream_ptr()),
              "blvm_conv1d_k2_fwd")  # fmt: skip
        ctx.save_for_backward(x, W)
        ctx.dims = (L, B, Cin, Cout, dilation)
        return out

    @staticmethod
    def backward(ctx, d_out):
        x, W = ctx.saved_tensors
        L, B, Cin, Cout, dilation = ctx.dims
        lib = load()
        f32 = dict(device=x.device, dtype=torch.float32)
        d_out = _f32c(d_out)
        d_x = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dW, db = torch.zeros_like(W), torch.zeros(Cout, **f32)
        ws = torch.empty(lib.blvm_conv1d_k2_workspace_floats(Cin, Cout), **f32)
        check(lib.blvm_conv1d_k2_bwd(ptr(x), ptr(W), ptr(d_out), L, B, Cin, Cout, dilation, ptr(d_x), ptr(dW), ptr(db), ptr(ws),
                                     stream_ptr()), "blvm_conv1d_k2_bwd")  # fmt: skip
        return d_x, dW, db, None


def conv1d_k2(x, weight, bias, dilation: int = 1):
    """Time-major dilated convolution with kernel size 2: x [L,B,Cin], weight [Cout,Cin,2] -> [L-dilation,B,Cout]."""
    return _Conv1dK2Function.apply(x, weight, bias, int(dilation))


def _embed_dims(emb, cw):
    """-> (V, E, C, m) of embedding.weight [V,E] and the grouped causal conv's weight [C,m,2] (groups = C)."""
    V, E = emb.shape
    C, m = cw.shape[0], cw.shape[1]
    if cw.ndim != 3 or cw.shape[2] != 2 or C * m != E:
        raise ValueError(f"wavenet_embed: embedding [{V},{E}] with a conv weight {tuple(cw.shape)}: need [C, E / C, 2]")
    return V, E, C, m


@torch.no_grad()
def wavenet_embed_tables(emb, cw):
    """K10e: embedding.weight [V,E] and the grouped causal conv's weight [C,E/C,2] -> the lookup tables P [2,V+1,C] (row V: zeros)."""
    emb, cw = _f32c(emb), _f32c(cw)
    V, _, C, m = _embed_dims(emb, cw)
    P = torch.empty(2, V + 1, C, device=emb.device, dtype=torch.float32)
    check(load().blvm_wavenet_embed_tables(ptr(emb), ptr(cw), V, C, m, ptr(P), stream_ptr()), "blvm_wavenet_embed_tables")
    return P


def _embed_classes(k, what="wavenet_embed_front"):
    if k.ndim != 2 or k.is_floating_point() or k.is_complex():
        raise TypeError(f"{what}: classes are an integer tensor [L,B] (time-major), got {k.dtype} {tuple(k.shape)}")
    return k.to(torch.int32).contiguous()


@torch.no_grad()
def wavenet_embed_lookup(P, bias, k, pad_causal: bool = True):
    """K10e forward on given tables: classes k [L,B] (integer, time-major; -1 = a zero-padded frame) ->
    out [L - 1 - pad_causal, B, C] = (P[0][k[t]] + P[1][k[t+1]]) + bias."""
    k, bias = _embed_classes(k), _f32c(bias)
    L, B = k.shape
    V, C = P.shape[1] - 1, P.shape[2]
    out = torch.empty(max(L - 1 - int(pad_causal), 0), B, C, device=P.device, dtype=torch.float32)
    check(load().blvm_wavenet_embed_fwd(ptr(P), ptr(bias), ptr(k), L, B, V, C, int(pad_causal), ptr(out), stream_ptr()), "blvm_wavenet_embed_fwd")
    return out


class _WaveNetEmbedFunction(torch.autograd.Function):
    """nn.Embedding(V, E) -> zero left-padding -> the causal convolution of kernel size 2 with groups = C, as one gather of two table
    rows per output frame (K10e); the gradients of all three parameters from per-class sums of d_out, without float atomics."""

    @staticmethod
    def forward(ctx, k, pad_causal, emb, cw, bias):
        emb, cw = _f32c(emb), _f32c(cw)
        k = _embed_classes(k)
        out = wavenet_embed_lookup(wavenet_embed_tables(emb, cw), bias, k, pad_causal)
        ctx.save_for_backward(k, emb, cw)
        return out

    @staticmethod
    def backward(ctx, d_out):
        k, emb, cw = ctx.saved_tensors
        V, E, C, m = _embed_dims(emb, cw)
        d_out = _f32c(d_out)
        Lo, B = d_out.shape[0], d_out.shape[1]
        lib = load()
        f32 = dict(device=emb.device, dtype=torch.float32)
        if Lo == 0:
            return None, None, torch.zeros(V, E, **f32), torch.zeros(C, m, 2, **f32), torch.zeros(C, **f32)
        # integer plumbing: the frames of every class, in frame order (a stable sort; padding sorts last, as class V)
        keys = k[: Lo + 1].reshape(-1)
        keys = torch.where((keys >= 0) & (keys < V), keys, torch.full_like(keys, V))
        skeys, perm = torch.sort(keys, stable=True)
        perm = perm.to(torch.int32)
        starts = torch.searchsorted(skeys, torch.arange(V + 1, device=keys.device, dtype=torch.int32)).to(torch.int32)
        n = keys.numel()
        G = torch.empty(2, V, C, **f32)
        ws = torch.empty(max(lib.blvm_wavenet_embed_bwd_workspace_floats(n, V, C, m), 1), **f32)
        d_emb, d_cw, d_bias = torch.empty(V, E, **f32), torch.empty(C, m, 2, **f32), torch.empty(C, **f32)
        check(lib.blvm_wavenet_embed_bwd(ptr(d_out), ptr(skeys), ptr(perm), ptr(starts), Lo, B, V, C, m, ptr(emb), ptr(cw), ptr(G), ptr(ws),
                                         ptr(d_emb), ptr(d_cw), ptr(d_bias), stream_ptr()), "blvm_wavenet_embed_bwd")  # fmt: skip
        return None, None, d_emb, d_cw, d_bias


def wavenet_embed_front(k, emb, cw, bias, pad_causal: bool = True):
    """K10e: classes k [L,B] (integer, time-major; -1 = a zero-padded frame), embedding.weight [V,E], the grouped causal conv's
    weight [C,E/C,2] and bias [C] -> [L - 1 - pad_causal, B, C]: `causal(pad(embedding(k)))` of the reference's embedded WaveNet."""
    return _WaveNetEmbedFunction.apply(k, bool(pad_causal), emb, cw, bias)


class _WaveNetStackFunction(torch.autograd.Function):
    """All gated residual blocks of a residual stack in one autograd node: x [L,B,C] -> G skip tensors [T_skip,B,S].
    `groups[i]` names the output that block i's skip branch is accumulated into; -1 = the block's skip is not used at all
    (its skip half of the 1x1 convolution is not computed; the weight rows get a zero gradient).
    params: (conv.weight [2C,C,2], conv.bias, conv1x1rs.weight [C+S,C,1], conv1x1rs.bias) per block."""

    @staticmethod
    def forward(ctx, x, dilations, groups, T_skip, inv_std, S, *params):
        x = _f32c(x)
        params = tuple(_f32c(p) for p in params)
        L, B, C = x.shape
        lib = load()
        f32 = dict(device=x.device, dtype=torch.float32)
        n_out = max(groups) + 1
        skips = [torch.zeros(T_skip, B, S, **f32) for _ in range(n_out)]
        n = max(i for i in range(len(dilations)) if groups[i] >= 0) + 1  # blocks after the last used skip cannot influence any output
        dil = (ctypes.c_int * n)(*dilations[:n])
        grp = (ctypes.c_int * n)(*groups[:n])
        na, nr = ctypes.c_size_t(0), ctypes.c_size_t(0)
        check(lib.blvm_wavenet_stack_floats(L, B, C, dil, n, ctypes.byref(na), ctypes.byref(nr)), "blvm_wavenet_stack_floats")
        acts = torch.empty(max(na.value, 1), **f32)  # residual outputs of blocks 0 .. n-2, back to back
        reserve = torch.empty(nr.value, **f32)
        ws = torch.empty(lib.blvm_wavenet_block_workspace_floats(L, B, C, S, 1), **f32)
        pp = (ctypes.c_void_p * (4 * n))(*[p.data_ptr() for p in params[: 4 * n]])
        sk = (ctypes.c_void_p * n_out)(*[t.data_ptr() for t in skips])
        check(lib.blvm_wavenet_stack_fwd(ptr(x), pp, dil, grp, n, L, B, C, S, T_skip, inv_std, ptr(acts), sk, ptr(reserve), ptr(ws),
                                         stream_ptr()), "blvm_wavenet_stack_fwd")  # fmt: skip
        ctx.cfg = (tuple(dilations), tuple(groups), T_skip, inv_std, S, L, B, C, n)
        ctx.save_for_backward(x, acts, reserve, *params)
        return tuple(skips)

    @staticmethod
    def backward(ctx, *d_skips):
        dilations, groups, T_skip, inv_std, S, L, B, C, n = ctx.cfg
        x, acts, reserve, *params = ctx.saved_tensors
        lib = load()
        f32 = dict(device=x.device, dtype=torch.float32)
        d_skips = [_f32c(g) if g is not None else torch.zeros(T_skip, B, S, **f32) for g in d_skips]
        ws = torch.empty(lib.blvm_wavenet_block_workspace_floats(L, B, C, S, 1), **f32)
        grads = _zeros_like_many(params)
        d_x, d_scratch = torch.empty_like(x), torch.empty_like(x)
        dil = (ctypes.c_int * n)(*dilations[:n])
        grp = (ctypes.c_int * n)(*groups[:n])
        pp = (ctypes.c_void_p * (4 * n))(*[p.data_ptr() for p in params[: 4 * n]])
        gp = (ctypes.c_void_p * (4 * n))(*[g.data_ptr() for g in grads[: 4 * n]])
        ds = (ctypes.c_void_p * len(d_skips))(*[t.data_ptr() for t in d_skips])
        check(lib.blvm_wavenet_stack_bwd(ptr(x), pp, dil, grp, n, L, B, C, S, T_skip, inv_std, ptr(acts), ptr(reserve), ds, ptr(d_x),
                                         ptr(d_scratch), gp, ptr(ws), stream_ptr()), "blvm_wavenet_stack_bwd")  # fmt: skip
        return (d_x, None, None, None, None, None, *grads)


def _conv1d_k2_bwd(x, W, d_out, dilation, need_dx, dW, db):
    """`blvm_conv1d_k2_bwd` with caller-chosen outputs: dW [Cout,Cin,2] and db [Cout] are accumulated into (None: not computed)."""
    L, B, Cin = x.shape
    d_x = torch.empty_like(x) if need_dx else None
    ws = torch.empty(load().blvm_conv1d_k2_workspace_floats(Cin, W.shape[0]), device=x.device, dtype=torch.float32)
    check(load().blvm_conv1d_k2_bwd(ptr(x), ptr(W), ptr(d_out), L, B, Cin, W.shape[0], dilation, ptr(d_x), ptr(dW), ptr(db), ptr(ws),
                                    stream_ptr()), "blvm_conv1d_k2_bwd")  # fmt: skip
    return d_x


def _wavenet_block_fwd(x, conv_w, conv_b, rs_w, rs_b, dilation, T_skip, inv_std, o, skip):
    """ONE gated residual block: x [L,B,C], conv_w [2C,C,2], rs_w [C+S,C] -> (pre [L-dilation,B,2C], act [L-dilation,B,C], reserve),
    pre and act being views of the reserve that `_wavenet_block_bwd` takes.  o [L-dilation,B,C] (None: no residual output) is written,
    skip [T_skip,B,S] (None with S = 0) is accumulated into; both are handed to the kernel as they are, wherever they start."""
    L, B, C = x.shape
    S, rows = rs_w.shape[0] - C, (L - dilation) * B
    lib = load()
    f32 = dict(device=x.device, dtype=torch.float32)
    reserve = torch.empty(lib.blvm_wavenet_block_reserve_floats(L, B, C, dilation), **f32)
    ws = torch.empty(lib.blvm_wavenet_block_workspace_floats(L, B, C, S, dilation), **f32)
    check(lib.blvm_wavenet_block_fwd(ptr(x), ptr(conv_w), ptr(conv_b), ptr(rs_w), ptr(rs_b), L, B, C, S, dilation, T_skip, inv_std, ptr(o),
                                     ptr(skip), ptr(reserve), ptr(ws), stream_ptr()), "blvm_wavenet_block_fwd")  # fmt: skip
    return reserve[: rows * 2 * C].view(L - dilation, B, 2 * C), reserve[rows * 2 * C : rows * 3 * C].view(L - dilation, B, C), reserve


def _wavenet_block_bwd(x, conv_w, rs_w, reserve, d_o, d_skip, dilation, T_skip, inv_std, dconv_w, dconv_b, drs_w, drs_b, d_x=None):
    """Backward of `_wavenet_block_fwd`: d_o [L-dilation,B,C] or None, d_skip [T_skip,B,S] (None with S = 0) -> d_x [L,B,C] (written
    into the buffer given, whatever it held); the parameter gradients are accumulated into the buffers given (None: not computed)."""
    L, B, C = x.shape
    S = rs_w.shape[0] - C
    d_x = torch.empty_like(x) if d_x is None else d_x
    ws = torch.empty(load().blvm_wavenet_block_workspace_floats(L, B, C, S, dilation), device=x.device, dtype=torch.float32)
    check(load().blvm_wavenet_block_bwd(ptr(x), ptr(conv_w), ptr(rs_w), ptr(reserve), ptr(d_o), ptr(d_skip), L, B, C, S, dilation, T_skip,
                                        inv_std, ptr(d_x), ptr(dconv_w), ptr(dconv_b), ptr(drs_w), ptr(drs_b), ptr(ws), stream_ptr()),
          "blvm_wavenet_block_bwd")  # fmt: skip
    return d_x


@torch.no_grad()
def wavenet_block_step(x2, params, inv_std: float, S: int, skip_acc, want_output: bool = True):
    """One gated residual block on ONE new frame for cached generation: x2 [2,B,C] = (the block's input `dilation` frames ago,
    its input now) -> the block's output now [1,B,C]; the skip branch is accumulated into skip_acc [1,B,S].  The same fused
    block kernel as training (K10) at L_in = 2, dilation = 1."""
    x2 = _f32c(x2)
    _, B, C = x2.shape
    cw, cb, rw, rb = (_f32c(p) for p in params)
    lib = load()
    f32 = dict(device=x2.device, dtype=torch.float32)
    o = torch.empty(1, B, C, **f32) if want_output else None
    res = torch.empty(lib.blvm_wavenet_block_reserve_floats(2, B, C, 1), **f32)
    ws = torch.empty(lib.blvm_wavenet_block_workspace_floats(2, B, C, S, 1), **f32)
    check(lib.blvm_wavenet_block_fwd(ptr(x2), ptr(cw), ptr(cb), ptr(rw), ptr(rb), 2, B, C, S, 1, 1, inv_std, ptr(o), ptr(skip_acc),
                                     ptr(res), ptr(ws), stream_ptr()), "blvm_wavenet_block_fwd")  # fmt: skip
    return o


class DmolHead(NamedTuple):
    """K10c's discretised-logistic-mixture head: the head Linear has 3 * num_mix <= 32 rows."""

    num_mix: int
    log_eps: float


class GmmHead(NamedTuple):
    """The diagonal Gaussian-mixture head of the VRNN / SRNN roll-outs: the DMoL head's layout and component pick, then x = mu + sd n
    with sd = softplus_beta(raw) + sd_eps (sd_beta == 0: raw is the sd)."""

    num_mix: int
    sd_beta: float
    sd_eps: float


class GaussHead(NamedTuple):
    """The plain Gaussian head of the VRNN / SRNN roll-outs: the head Linear is [2,2] -> (mu, raw), x = mu + sd n as for `GmmHead`."""

    sd_beta: float
    sd_eps: float


class CategoricalHead(NamedTuple):
    """K10c's softmax head: levels [V] are the class values, the head Linear is [V,O] (16 <= V <= 1024, a multiple of 16)."""

    levels: torch.Tensor


class WaveNetDecodeOut(NamedTuple):
    x: torch.Tensor  # [B,n_frames]
    k: Optional[torch.Tensor]  # [B,n_frames] int32 classes (the categorical head)
    scratch: torch.Tensor  # the buffer the call used; with the last two samples its rings (`wavenet_ring_views`) are the state
    samples: Optional[torch.Tensor]  # [B,2], the last two samples (a resumed call)


def _wavenet_decode_pack(weights, head):
    """The packed weight image of K10c and its sizes: -> (lib, C, S, O, device, packed, dilations as a C array, tables).  The image ends
    in the head Linear: padded with zeros to 32 rows (`DmolHead`, `GmmHead`, and `GaussHead`'s [2,O]), as it stands (`CategoricalHead`).  An embedded model (K10e) gives
    (tables [2,V+1,C], bias) as `causal`: the tables travel beside the image, whose causal weights are zeros nobody reads."""
    causal, in_transform, blocks_params, dilations, out_linear, (hw, hb) = weights
    lib = load()
    C, S, O = in_transform[0].shape[0], blocks_params[0][2].shape[0] - in_transform[0].shape[0], out_linear[0].shape[0]
    dev = causal[0].device
    tables = None
    if isinstance(head, CategoricalHead) and tuple(causal[0].shape) == (2, hw.shape[0] + 1, C):
        tables = _f32c(causal[0])
        causal = (torch.zeros(2 * C, device=dev), causal[1])
    if causal[0].numel() != 2 * C:
        raise NotImplementedError("libblvm_hip: wavenet_decode is built for in_channels = n_stack_frames = 1")
    if isinstance(head, (DmolHead, GmmHead, GaussHead)):
        rows = 2 if isinstance(head, GaussHead) else 3 * head.num_mix
        if hw.shape[0] > 32 or hw.shape[0] != rows:
            raise NotImplementedError("libblvm_hip: wavenet_decode head must have 3 * num_mix <= 32 outputs (2 for the Gaussian head)")
        pad_w = torch.zeros(32 - hw.shape[0], hw.shape[1], device=dev)
        tail = [hw, pad_w, hb, pad_w.new_zeros(32 - hb.numel())]
        want = lib.blvm_wavenet_decode_pack_floats(C, S, O, len(blocks_params))
    else:
        V = hw.shape[0]
        if head.levels.numel() != V or hb.numel() != V:
            raise ValueError(f"wavenet_decode: a head of {V} classes with {hb.numel()} biases and {head.levels.numel()} levels")
        tail = [hw, hb]
        want = lib.blvm_wavenet_cat_decode_pack_floats(C, S, O, len(blocks_params), V)
    parts = [*causal, *in_transform, *(p for blk in blocks_params for p in blk), *out_linear, *tail]
    packed = torch.cat([_f32c(p).reshape(-1) for p in parts])
    if packed.numel() != want:
        raise ValueError("wavenet_decode: parameter shapes do not match the packed layout")
    return lib, C, S, O, dev, packed, _c_ints(dilations), tables


@torch.no_grad()
def wavenet_decode(weights, head, B: int, n_frames: int, inv_std: float, skip_scale: float, draws=None, resume=None):
    """K10c: all frames of B utterances in one launch.  weights = (causal, in_transform, blocks_params, dilations, out_linear,
    head_linear): (weight, bias) pairs, blocks_params as for wavenet_stack.  head = `DmolHead` with draws = (u [n_frames,B,num_mix],
    v [n_frames,B]), or `CategoricalHead` with draws = u [n_frames,B]: uniform draws indexed from 0 (None: the mode, the arg-max class);
    `GmmHead` with draws = (u [n_frames,B,num_mix] uniforms, n [n_frames,B] standard normals) or `GaussHead` with draws = n [n_frames,B]
    (None: the arg-max component's mean / the mean; these two draws are not clamped).
    resume = (t0, samples [B,2], scratch) continues from a state: `scratch` holds the ring buffers after absolute frame t0 - 1
    (`wavenet_prime_rings` or an earlier call; updated in place), samples the last two samples.  -> `WaveNetDecodeOut`.
    An embedded model (K10e) with the categorical head: `causal` = (tables [2,V+1,C] of `wavenet_embed_tables`, bias); the class is fed
    back as a class, the zero start is a past of class 0, and samples (in and out) are the last two CLASSES, int32 [B,2]."""
    lib, C, S, O, dev, packed, dil, tables = _wavenet_decode_pack(weights, head)
    gauss = 1 if isinstance(head, GmmHead) else 2 if isinstance(head, GaussHead) else 0
    pair = isinstance(head, (DmolHead, GmmHead))  # two draws per frame
    dmol, n = pair or gauss == 2, len(dil)  # the float heads: one output x, no classes
    shapes = [(n_frames, B, head.num_mix), (n_frames, B)] if pair else [(n_frames, B)]
    if draws is None:
        draws = [None] * len(shapes)
    else:
        draws = [_f32c(t) for t in (draws if pair else (draws,))]
        if [tuple(t.shape) for t in draws] != shapes:
            raise ValueError("wavenet_decode: the draws must be (u [n_frames,B,num_mix], v [n_frames,B]) for the DMoL and the Gaussian-mixture "
                             "head and u [n_frames,B] for the categorical head, n [n_frames,B] for the Gaussian head")  # fmt: skip
    n_scratch = lib.blvm_wavenet_decode_scratch_floats(dil, n, B, C, S)
    f32 = dict(device=dev, dtype=torch.float32)
    if resume is None:
        scratch = torch.empty(n_scratch, **f32)
    else:
        t0, samples, scratch = resume
        if scratch.dtype != torch.float32 or scratch.numel() != n_scratch:
            raise ValueError("wavenet_decode: the scratch buffer does not belong to these shapes")
        if tables is not None and samples.dtype != torch.int32:
            raise ValueError("wavenet_decode: an embedded model continues from the last two classes, int32 [B,2]")
        samples = samples.contiguous() if tables is not None else _f32c(samples)
        if tuple(samples.shape) != (B, 2):
            raise ValueError("wavenet_decode: samples must be [B,2]")
    x = torch.empty(B, n_frames, **f32)
    k = None if dmol else torch.empty(B, n_frames, device=dev, dtype=torch.int32)
    width2 = ()
    if gauss:
        if not (head.sd_beta > 0.0 and head.sd_eps >= 0.0):
            raise ValueError("wavenet_decode: the Gaussian heads need sd_beta > 0 (the raw scales go through the softplus) and sd_eps >= 0")
        u_n = draws if gauss == 1 else (None, draws[0])
        name, width, width2 = "blvm_wavenet_gauss_decode", gauss, (head.num_mix if gauss == 1 else 0,)
        operands = (float(head.sd_beta), float(head.sd_eps), *map(ptr, u_n))
    elif dmol:
        name, width, operands = "blvm_wavenet_decode", head.num_mix, (head.log_eps, *map(ptr, draws))
    else:
        name, width = "blvm_wavenet_cat_decode", head.levels.numel()
        levels = _f32c(head.levels.to(dev)).reshape(width)  # (named: it must outlive the launch's enqueue)
        operands = (ptr(levels), ptr(draws[0]))
    sizes = (ptr(packed), dil, n, B, C, S, O, width, *width2, n_frames)
    if tables is not None:
        name, sizes = "blvm_wavenet_embed_cat_decode", (ptr(packed), ptr(tables), *sizes[1:])
    outs = (ptr(x),) if dmol else (ptr(x), ptr(k))
    if resume is None:
        check(getattr(lib, name)(*sizes, inv_std, skip_scale, *operands, ptr(scratch), *outs, stream_ptr()), name)
        return WaveNetDecodeOut(x, k, scratch, None)
    samples_out = torch.empty(B, 2, device=dev, dtype=samples.dtype)
    name += "_resume"
    check(getattr(lib, name)(*sizes, int(t0), inv_std, skip_scale, *operands, ptr(samples), ptr(scratch), *outs, ptr(samples_out),
                             stream_ptr()), name)  # fmt: skip
    return WaveNetDecodeOut(x, k, scratch, samples_out)


def _ring_views(scratch, off: int, dilations, B: int, C: int):
    """Consecutive views [dilation_i,B,C] of `scratch` from float offset `off`: block i's input over its last dilation_i frames."""
    views = []
    for d in dilations:
        views.append(scratch[off : off + d * B * C].view(d, B, C))
        off += d * B * C
    return views


def wavenet_ring_views(scratch, dilations, B: int, C: int, S: int):
    """The ring buffers inside a K10c scratch buffer: block i's input over its last dilation_i frames as a view [dilation_i,B,C]."""
    return _ring_views(scratch, load().blvm_wavenet_decode_ring_offset_floats(len(dilations), C, S), dilations, B, C)


def wavenet_decode_scratch(dilations, B: int, C: int, S: int, device):
    """An uninitialised K10c scratch buffer and its ring views."""
    scratch = torch.empty(load().blvm_wavenet_decode_scratch_floats(_c_ints(dilations), len(dilations), B, C, S), device=device, dtype=torch.float32)
    return scratch, wavenet_ring_views(scratch, dilations, B, C, S)


@torch.no_grad()
def wavenet_ring_fill(h, dilation: int, t0: int, ring):
    """h [L,B,C] (a block's input, last frame = absolute frame t0 - 1) -> its last `dilation` frames into ring [dilation,B,C],
    frame tau in slot tau mod dilation."""
    L, B, C = h.shape
    if h.dtype != torch.float32 or not h.is_contiguous() or not ring.is_contiguous() or tuple(ring.shape) != (dilation, B, C):
        raise ValueError("wavenet_ring_fill: h must be contiguous fp32 [L,B,C] and ring contiguous [dilation,B,C]")
    t0 = t0 % dilation + dilation  # only the phase matters
    check(load().blvm_wavenet_decode_ring_fill(ptr(h), L, B, C, dilation, t0, ptr(ring), stream_ptr()), "blvm_wavenet_decode_ring_fill")


@torch.no_grad()
def wavenet_prime_rings(h0, blocks_params, dilations, inv_std: float, S: int, t0: int, rings):
    """Fill every block's ring buffer from a window: h0 [L,B,C] = block 0's input whose last frame is absolute frame t0 - 1,
    L >= sum(dilations).  The time-parallel block kernel (K10) gives block i+1's input from block i's; each ring takes the
    tail of its block's input.  Two activation buffers (ping-pong), one reserve and one workspace, whatever the block count."""
    h0 = _f32c(h0)
    L, B, C = h0.shape
    if L < sum(dilations):
        raise ValueError(f"wavenet_prime_rings: {L} frames for dilations that sum to {sum(dilations)}")
    lib = load()
    f32 = dict(device=h0.device, dtype=torch.float32)
    n, d0 = len(dilations), dilations[0]
    bufs = [torch.empty(max(L - d0, 1) * B * C, **f32) for _ in range(min(n - 1, 2))]
    if n > 1:
        reserve = torch.empty(lib.blvm_wavenet_block_reserve_floats(L, B, C, d0), **f32)
        ws = torch.empty(lib.blvm_wavenet_block_workspace_floats(L, B, C, S, d0), **f32)
        skip = torch.zeros(1, B, S, **f32)  # the blocks' skip branch of the newest window frame: not used
    cur = h0
    for i, d in enumerate(dilations):
        wavenet_ring_fill(cur, d, t0, rings[i])
        if i == n - 1:
            break
        cw, cb, rw, rb = (_f32c(p) for p in blocks_params[i])
        o = bufs[i % 2][: (L - d) * B * C].view(L - d, B, C)
        check(lib.blvm_wavenet_block_fwd(ptr(cur), ptr(cw), ptr(cb), ptr(rw), ptr(rb), L, B, C, S, d, 1, inv_std, ptr(o), ptr(skip),
                                         ptr(reserve), ptr(ws), stream_ptr()), "blvm_wavenet_block_fwd")  # fmt: skip
        cur, L = o, L - d


def stcn_generate_pack(weights, S: int, num_mix: int):
    """The packed weight image of K10d (`blvm_stcn_generate`) and the host arrays that travel with it.  weights = (causal,
    in_transform, blocks_params, dilations, groups, priors, order, out_in, out_blocks_params, up_linear, head_linear, dense): causal /
    in_transform / out_in / up_linear / head_linear = (weight, bias); blocks_params as for wavenet_stack; groups[i] = the latent level
    that reads block i's skip (or -1); priors[l] = (the three nn.Linear of the mean MLP, those of the sd MLP); order = the levels in
    visiting order.  -> namespace(lib, packed, C, dil, groups, latent, order, n_blocks, n_out, n, dense, latent_sizes)."""
    from types import SimpleNamespace

    causal, in_transform, blocks_params, dilations, groups, priors, order, out_in, out_blocks_params, up_linear, head_linear, dense = weights
    lib = load()
    C = in_transform[0].shape[0]
    dev = causal[0].device
    F = 3 * num_mix
    hw, hb = head_linear
    uw, ub = up_linear
    if tuple(hw.shape) != (F, F) or F > 32 or uw.shape[0] != S * F:
        raise NotImplementedError("libblvm_hip: stcn_generate needs a [3K,3K] head with 3 * num_mix <= 32 and an up-sampling to S * 3K")
    if causal[0].numel() != 2 * S * C:
        raise NotImplementedError("libblvm_hip: stcn_generate is built for in_channels = 1, kernel_size = 2")
    up_rows = (S * F + 15) // 16 * 16
    z = lambda *shape: torch.zeros(*shape, device=dev, dtype=torch.float32)  # noqa: E731
    parts = [*causal, *in_transform, *(p for blk in blocks_params for p in blk)]
    for mu_layers, sd_layers in priors:
        parts += [t for layers in (mu_layers, sd_layers) for lin in layers for t in (lin.weight, lin.bias)]
    parts += [*out_in, *(p for blk in out_blocks_params for p in blk)]
    parts += [uw, z(up_rows - S * F, uw.shape[1]), ub, z(up_rows - S * F)]
    parts += [torch.nn.functional.pad(hw.detach(), (0, 32 - F, 0, 32 - F)), hb, z(32 - F)]
    packed = torch.cat([_f32c(p.detach()).reshape(-1) for p in parts])
    latent_sizes = [int(mu[2].weight.shape[0]) for mu, _ in priors]
    ns = SimpleNamespace(lib=lib, packed=packed, C=C, dil=_c_ints(dilations), groups=_c_ints(groups), latent=_c_ints(latent_sizes),
                         order=_c_ints(order),
                         n_blocks=len(dilations), n_out=len(out_blocks_params), n=len(priors), dense=int(bool(dense)), latent_sizes=latent_sizes)  # fmt: skip
    want = lib.blvm_stcn_generate_pack_floats(C, S, ns.n_blocks, ns.n_out, ns.latent, ns.order, ns.n, ns.dense, num_mix)
    if want == 0:
        raise _hip.BlvmHipError("blvm_stcn_generate: " + lib.blvm_last_error().decode(errors="replace"))
    if packed.numel() != want:
        raise ValueError("stcn_generate: parameter shapes do not match the packed layout")
    return ns


def stcn_generate_scratch_floats(dilations, n_out: int, latent_sizes, order, dense: bool, B: int, C: int, S: int, num_mix: int) -> int:
    """Size of a K10d scratch buffer (a host computation: no device needed)."""
    lib = load()
    n = lib.blvm_stcn_generate_scratch_floats(_c_ints(dilations), C, S, len(dilations), n_out, _c_ints(latent_sizes), _c_ints(order),
                                              len(latent_sizes), int(bool(dense)), num_mix, B)  # fmt: skip
    if n == 0:
        raise _hip.BlvmHipError("blvm_stcn_generate: " + lib.blvm_last_error().decode(errors="replace"))
    return max(int(n), 4)


@torch.no_grad()
def stcn_generate(weights, B: int, T: int, S: int, inv_std: float, out_scale: float, sd_beta: float, sd_eps: float, slope: float,
                  num_mix: int, log_eps: float, eps, u=None, v=None, resume=None):
    """K10d: T steps of ancestral sampling from the STCN for B rows in one launch (weights as `stcn_generate_pack`).  eps[l]
    [T,B,Z_l]; u [T,B,S,num_mix], v [T,B,S] uniform draws (None: the mode), all indexed from 0.  resume = (t0, x_in [B,2,S], scratch)
    continues from a state: `scratch` holds the rings after absolute step t0 - 1 (primed through `stcn_ring_views`, or an earlier
    call's; updated in place), x_in the two newest stacks.
    -> (x [B,T,S], z, mu, sd: lists of [T,B,Z_l], scratch, x_state [B,2,S] or None).  With the last two stacks of x (zero stacks in
    front of step 0) the rings in the scratch buffer a zero start hands back are the state after T steps."""
    p = stcn_generate_pack(weights, S, num_mix)
    lib, dev = p.lib, p.packed.device
    f32 = dict(device=dev, dtype=torch.float32)
    eps = [_f32c(e) for e in eps]
    if len(eps) != p.n or any(tuple(e.shape) != (T, B, Z) for e, Z in zip(eps, p.latent_sizes)):
        raise ValueError("stcn_generate: eps[l] must be [T,B,Z_l] for every level")
    if u is not None:
        u, v = _f32c(u), _f32c(v)
        if tuple(u.shape) != (T, B, S, num_mix) or tuple(v.shape) != (T, B, S):
            raise ValueError("stcn_generate: u must be [T,B,S,num_mix] and v [T,B,S]")
    n_scratch = stcn_generate_scratch_floats(p.dil, p.n_out, p.latent_sizes, p.order, p.dense, B, p.C, S, num_mix)
    if resume is None:
        scratch = torch.empty(n_scratch, **f32)
    else:
        t0, x_in, scratch = resume
        if scratch.dtype != torch.float32 or scratch.device != dev or scratch.numel() != n_scratch or not scratch.is_contiguous():
            raise ValueError("stcn_generate: the scratch buffer does not belong to these shapes")
        x_in = _f32c(x_in)
        if tuple(x_in.shape) != (B, 2, S):
            raise ValueError("stcn_generate: x_in must be [B,2,S]")
    x = torch.empty(B, T, S, **f32)
    zs, mus, sds = ([torch.empty(T, B, Z, **f32) for Z in p.latent_sizes] for _ in range(3))
    ptrs = lambda ts: (ctypes.c_void_p * len(ts))(*[ptr(t) for t in ts])  # noqa: E731
    args = (ptr(p.packed), p.dil, p.groups, p.n_blocks, p.n_out, p.latent, p.order, p.n, p.dense, B, p.C, S, num_mix, T, inv_std, out_scale,
            sd_beta, sd_eps, slope, log_eps, ptrs(eps), ptr(u), ptr(v), ptr(x), ptrs(zs), ptrs(mus), ptrs(sds), ptr(scratch))  # fmt: skip
    if resume is None:
        check(lib.blvm_stcn_generate(*args, stream_ptr()), "blvm_stcn_generate")
        return x, zs, mus, sds, scratch, None
    x_state = torch.empty(B, 2, S, **f32)
    check(lib.blvm_stcn_generate_resume(*args, int(t0), ptr(x_in), ptr(x_state), stream_ptr()), "blvm_stcn_generate_resume")
    return x, zs, mus, sds, scratch, x_state


def stcn_ring_views(scratch, dilations, n_out: int, latent_sizes, order, dense: bool, B: int, C: int, S: int, num_mix: int):
    """The state inside a K10d scratch buffer as views: (rings: dilated block i's input over its last dilation_i steps [dilation_i,B,C],
    orings: output block j's input at the last step [1,B,C])."""
    off = int(load().blvm_stcn_generate_ring_offset_floats(C, S, len(dilations), n_out, _c_ints(latent_sizes), _c_ints(order),
                                                           len(latent_sizes), int(bool(dense)), num_mix))  # fmt: skip
    if off == 0:
        raise _hip.BlvmHipError("blvm_stcn_generate: " + load().blvm_last_error().decode(errors="replace"))
    rings = _ring_views(scratch, off, [*dilations, *([1] * n_out)], B, C)
    return rings[: len(dilations)], rings[len(dilations) :]


def stcn_generate_scratch(dilations, n_out: int, latent_sizes, order, dense: bool, B: int, C: int, S: int, num_mix: int, device):
    """An uninitialised K10d scratch buffer and its state views: -> (scratch, (rings, orings))."""
    scratch = torch.empty(stcn_generate_scratch_floats(dilations, n_out, latent_sizes, order, dense, B, C, S, num_mix), device=device,
                          dtype=torch.float32)  # fmt: skip
    return scratch, stcn_ring_views(scratch, dilations, n_out, latent_sizes, order, dense, B, C, S, num_mix)


def wavenet_stack(x, blocks_params, dilations, T_skip: int, inv_std: float, S: int, groups=None):
    """x [L,B,C] -> skip output(s) [T_skip,B,S]: the sum over blocks of the last T_skip frames of each block's skip branch
    (groups=None: one sum over all blocks, returned as a tensor; otherwise a tuple, see _WaveNetStackFunction)."""
    flat = [p for blk in blocks_params for p in blk]
    g = tuple(0 for _ in dilations) if groups is None else tuple(int(v) for v in groups)
    out = _WaveNetStackFunction.apply(x, tuple(int(d) for d in dilations), g, int(T_skip), float(inv_std), int(S), *flat)
    return out[0] if groups is None else out


# ----------------------------------------------------------------------------------------------------------------------
# K5: RSSM cell (Clockwork-VAE) over a sequence
# ----------------------------------------------------------------------------------------------------------------------

_RSSM_PARAM_ORDER = (
    ["gin_w", "gin_b", "gru_wih", "gru_whh", "gru_bih", "gru_bhh"]
    + ["prior_w0", "prior_b0", "prior_w1", "prior_b1", "prior_w2", "prior_b2", "prior_hw", "prior_hb"]
    + ["post_w0", "post_b0", "post_w1", "post_b1", "post_w2", "post_b2", "post_hw", "post_hb"]
)
RSSM_PLAIN, RSSM_RESIDUAL, RSSM_PRECISION, RSSM_GENERATE = 0, 1, 2, 3  # 3: z drawn from the prior (generation)


class _RSSMSeqFunction(torch.autograd.Function):
    """(enc, ctx, z0, h0, eps, 22 params) -> zs [T+1,B,Z], hs [T+1,B,H], kld [B], kld_fn [B] (+ non-diff. mu/sd)."""

    @staticmethod
    def forward(ctx_, enc, ctx, z0, h0, eps, x_sl_dev, cfg, *params):
        T, B, H, Z, C, E, mode, sd_eps, stride, fn_floor = cfg
        enc, eps = _f32c(enc), _f32c(eps)
        ctx = _f32c(ctx) if ctx is not None else None
        params = tuple(_f32c(p) for p in params)
        lib = load()
        f32 = dict(device=enc.device, dtype=torch.float32)
        zs, hs = torch.empty(T + 1, B, Z, **f32), torch.empty(T + 1, B, H, **f32)
        mu_q, sd_q, mu_p, sd_p = (torch.empty(T, B, Z, **f32) for _ in range(4))
        reserve = torch.empty(lib.blvm_rssm_reserve_floats(T, B, H, Z), **f32)
        w = _pack(_hip.RssmWeights, _RSSM_PARAM_ORDER, params)
        check(
            lib.blvm_rssm_seq_fwd(w, ptr(enc), ptr(ctx), ptr(_f32c(z0)) if z0 is not None else None,
                                  ptr(_f32c(h0)) if h0 is not None else None, ptr(eps), T, B, H, Z, C, E, mode, sd_eps, ptr(zs),
                                  ptr(hs), ptr(mu_q), ptr(sd_q), ptr(mu_p), ptr(sd_p), ptr(reserve), stream_ptr()),
            "blvm_rssm_seq_fwd",
        )  # fmt: skip
        kld = torch.zeros(B, device=enc.device, dtype=torch.float64)
        kld_fn = torch.zeros(B, device=enc.device, dtype=torch.float64)
        check(
            lib.blvm_kl_fwd(ptr(mu_q), ptr(sd_q), ptr(mu_p), ptr(sd_p), LAYOUT_TIME_MAJOR, ptr(x_sl_dev), B, T, Z, stride,
                            fn_floor, ptr(kld), ptr(kld_fn), stream_ptr()),
            "blvm_kl_fwd",
        )  # fmt: skip
        ctx_.cfg = cfg
        ctx_.has = (ctx is not None, z0 is not None, h0 is not None)
        saved = [enc, eps, x_sl_dev, zs, hs, mu_q, sd_q, mu_p, sd_p, reserve] + ([ctx] if ctx is not None else [])
        ctx_.n_fixed = len(saved)
        ctx_.save_for_backward(*saved, *params)
        ctx_.mark_non_differentiable(mu_q, sd_q, mu_p, sd_p)
        ctx_.set_materialize_grads(False)  # (else autograd fills a [T',B,Z] zero gradient per statistics output: 16 MB each at [64,16000])
        return zs, hs, kld, kld_fn, mu_q, sd_q, mu_p, sd_p

    @staticmethod
    def backward(ctx_, d_zs, d_hs, g_kld, g_kld_fn, *_unused):
        T, B, H, Z, C, E, mode, sd_eps, stride, fn_floor = ctx_.cfg
        has_ctx, has_z0, has_h0 = ctx_.has
        saved = ctx_.saved_tensors
        enc, eps, x_sl_dev, zs, hs, mu_q, sd_q, mu_p, sd_p, reserve = saved[:10]
        ctx = saved[10] if has_ctx else None
        params = saved[ctx_.n_fixed :]
        lib = load()
        f32 = dict(device=enc.device, dtype=torch.float32)
        d_zs = _f32c(d_zs) if d_zs is not None else torch.zeros_like(zs)
        d_hs = _f32c(d_hs) if d_hs is not None else torch.zeros_like(hs)
        c_raw = g_kld.to(torch.float32).contiguous() if g_kld is not None else None
        c_fn = g_kld_fn.to(torch.float32).contiguous() if g_kld_fn is not None else None
        grads = _zeros_like_many(params)
        d_enc = torch.empty_like(enc)
        d_ctx = torch.empty_like(ctx) if has_ctx else None
        d_z0 = torch.empty(B, Z, **f32) if has_z0 else None
        d_h0 = torch.empty(B, H, **f32) if has_h0 else None
        ws = torch.empty(lib.blvm_rssm_bwd_workspace_floats(T, B, H, Z), **f32)
        w, g = _pack(_hip.RssmWeights, _RSSM_PARAM_ORDER, params), _pack(_hip.RssmGrads, _RSSM_PARAM_ORDER, grads)
        check(
            lib.blvm_rssm_seq_bwd(w, ptr(enc), ptr(ctx), ptr(eps), ptr(zs), ptr(hs), ptr(mu_q), ptr(sd_q),
                                  ptr(mu_p), ptr(sd_p), ptr(reserve), ptr(d_zs), ptr(d_hs), ptr(x_sl_dev), ptr(c_raw), ptr(c_fn),
                                  stride, fn_floor, T, B, H, Z, C, E, mode, sd_eps, ptr(d_enc), ptr(d_ctx), ptr(d_z0), ptr(d_h0),
                                  g, ptr(ws), stream_ptr()),
            "blvm_rssm_seq_bwd",
        )  # fmt: skip
        if d_h0 is not None:
            d_h0 = d_h0 + d_hs[0]  # the direct gradient wrt the carried state (tiny [B,H] add)
        return (d_enc, d_ctx, d_z0, d_h0, None, None, None, *grads)


def rssm_sequence(enc, ctx, z0, h0, eps, x_sl_dev, params, H, Z, mode, stride, free_nats=0.0, sd_eps=1e-6):
    """enc [T,B,E], ctx [T,B,C] or None -> (zs [T+1,B,Z], hs [T+1,B,H], kld [B], kld_fn [B], mu_q, sd_q, mu_p, sd_p)."""
    T, B, E = enc.shape
    C = ctx.shape[2] if ctx is not None else 0
    fn_floor = float(free_nats) / Z if free_nats else 0.0
    cfg = (T, B, H, Z, C, E, int(mode), float(sd_eps), int(stride), fn_floor)
    return _RSSMSeqFunction.apply(enc, ctx, z0, h0, eps, x_sl_dev, cfg, *params)


# ----------------------------------------------------------------------------------------------------------------------
# K11: Clockwork-VAE convolutional coders — time-major channel-last [L,B,C]
# ----------------------------------------------------------------------------------------------------------------------


def _norm_ws(N, device):
    return torch.empty(load().blvm_chan_norm_workspace_doubles(N), device=device, dtype=torch.float64)


def _chan_norm_fwd(x, gamma, beta, eps):
    L, B, C = x.shape
    y, mr = torch.empty_like(x), torch.empty(2, B * C, device=x.device, dtype=torch.float32)
    check(load().blvm_chan_norm_fwd(ptr(x), L, B * C, C, ptr(gamma), ptr(beta), eps, ptr(y), ptr(mr), ptr(_norm_ws(B * C, x.device)),
                                    stream_ptr()), "blvm_chan_norm_fwd")  # fmt: skip
    return y, mr


def _chan_norm_stats(x, gamma, beta, eps):
    """Statistics only: mr [2,N] = [mean | rstd] and the column affine ss [2,N] with norm(x) = x * ss[0] + ss[1]."""
    L, B, C = x.shape
    mr, ss = (torch.empty(2, B * C, device=x.device, dtype=torch.float32) for _ in range(2))
    check(load().blvm_chan_norm_stats(ptr(x), L, B * C, C, ptr(gamma), ptr(beta), eps, ptr(mr), ptr(ss),
                                      ptr(_norm_ws(B * C, x.device)), stream_ptr()), "blvm_chan_norm_stats")  # fmt: skip
    return mr, ss


def _chan_norm_bwd(x, dy, mr, gamma, relu_mask, dgamma, dbeta, dx_chan_sum=None):
    L, B, C = x.shape
    dx = torch.empty_like(x)
    check(load().blvm_chan_norm_bwd(ptr(x), ptr(dy), ptr(mr), ptr(gamma), L, B * C, C, int(relu_mask), ptr(dx), ptr(dgamma),
                                    ptr(dbeta), ptr(dx_chan_sum), ptr(_norm_ws(B * C, x.device)), stream_ptr()),
          "blvm_chan_norm_bwd")  # fmt: skip
    return dx


def _dwconv_fwd(x, w, bias, stride, dilation, transposed, relu, in_affine=None):
    L, B, C = x.shape
    k = w.shape[-1]
    L_out = load().blvm_dwconv_out_length(L, k, stride, dilation, int(transposed))
    if L_out <= 0:
        raise _hip.BlvmHipError(f"depthwise conv: input length {L} is shorter than the kernel ({k=}, {dilation=})")
    y = torch.empty(L_out, B, C, device=x.device, dtype=torch.float32)
    sc, sh = (in_affine[0], in_affine[1]) if in_affine is not None else (None, None)
    check(load().blvm_dwconv_fwd(ptr(x), ptr(sc), ptr(sh), ptr(w), ptr(bias), L, B * C, C, k, stride, dilation, int(transposed),
                                 int(relu), ptr(y), stream_ptr()), "blvm_dwconv_fwd")  # fmt: skip
    return y


def _dwconv_bwd(x, w, y, dy, stride, dilation, transposed, relu, need_dx, dw, dbias, in_affine=None):
    L, B, C = x.shape
    k = w.shape[-1]
    dx = torch.empty_like(x) if need_dx else None
    sc, sh = (in_affine[0], in_affine[1]) if in_affine is not None else (None, None)
    check(load().blvm_dwconv_bwd(ptr(x), ptr(sc), ptr(sh), ptr(w), ptr(y), ptr(dy), L, B * C, C, k, stride, dilation,
                                 int(transposed), int(relu), ptr(dx), ptr(dw), ptr(dbias), stream_ptr()), "blvm_dwconv_bwd")  # fmt: skip
    return dx


class _ChanNormFunction(torch.autograd.Function):
    """nn.GroupNorm(num_groups=C, C) on [L,B,C]: per-(sample, channel) normalisation over time."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        x, gamma, beta = _f32c(x), _f32c(gamma), _f32c(beta)
        y, mr = _chan_norm_fwd(x, gamma, beta, eps)
        ctx.save_for_backward(x, mr, gamma)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mr, gamma = ctx.saved_tensors
        dgamma, dbeta = torch.zeros_like(gamma), torch.zeros_like(gamma)
        dx = _chan_norm_bwd(x, _f32c(dy), mr, gamma, False, dgamma, dbeta)
        return dx, dgamma, dbeta, None


def chan_norm(x, gamma, beta, eps: float = 1e-5):
    return _ChanNormFunction.apply(x, gamma, beta, eps)


class _DwConvFunction(torch.autograd.Function):
    """Depthwise Conv1d / ConvTranspose1d (groups = channels, no padding) on [L,B,C], optional fused ReLU."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, dilation, transposed, relu):
        x, w = _f32c(x), _f32c(w)
        bias = _f32c(bias) if bias is not None else None
        y = _dwconv_fwd(x, w, bias, stride, dilation, transposed, relu)
        ctx.cfg = (stride, dilation, transposed, relu, bias is not None)
        ctx.save_for_backward(x, w, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        stride, dilation, transposed, relu, has_bias = ctx.cfg
        x, w, y = ctx.saved_tensors
        dw = torch.zeros_like(w)
        db = torch.zeros(w.shape[0], device=w.device, dtype=torch.float32) if has_bias else None
        dx = _dwconv_bwd(x, w, y, _f32c(dy), stride, dilation, transposed, relu, ctx.needs_input_grad[0], dw, db)
        return dx, dw, db, None, None, None, None


def dwconv(x, weight, bias, stride=1, dilation=1, transposed=False, relu=False):
    return _DwConvFunction.apply(x, weight, bias, int(stride), int(dilation), bool(transposed), bool(relu))


class _ResampleAddFunction(torch.autograd.Function):
    """TemporalResidual: y + nearest-resampled x (convolutional_coders.py:15-26); y [Ly,B,C], x [Lx,B,C]."""

    @staticmethod
    def forward(ctx, y, x):
        y, x = _f32c(y), _f32c(x)
        Ly, B, C = y.shape
        out = torch.empty_like(y)
        check(load().blvm_resample_add_fwd(ptr(y), ptr(x), Ly, x.shape[0], B * C, ptr(out), stream_ptr()), "blvm_resample_add_fwd")
        ctx.Lx = x.shape[0]
        return out

    @staticmethod
    def backward(ctx, dout):
        dout = _f32c(dout)
        Ly, B, C = dout.shape
        if ctx.Lx == Ly:
            return dout, dout
        dx = torch.zeros(ctx.Lx, B, C, device=dout.device, dtype=torch.float32)
        check(load().blvm_resample_add_bwd(ptr(dout), Ly, ctx.Lx, B * C, ptr(dx), stream_ptr()), "blvm_resample_add_bwd")
        return dout, dx


def resample_add(y, x):
    return _ResampleAddFunction.apply(y, x)


def dense_conv(x, weight, bias, stride: int = 1, dilation: int = 1, transposed: bool = False):
    """Dense k-tap Conv1d / ConvTranspose1d (groups = 1, no padding) on time-major x [L,B,Cin] -> [L_out,B,Cout]: the products of
    ALL taps are one K6 GEMM over every input row ([L*B, Cin] x [Cin, k*Cout], its weight and input gradients from the same node);
    the taps are then strided slices of that product, summed (convolution) or added into their strided output positions
    (transposed convolution) by autograd-tracked slicing.  weight: Conv1d [Cout,Cin,k], ConvTranspose1d [Cin,Cout,k].
    (`BlockSimple`, convolutional_coders.py:69-91 — not a BASELINE configuration: the stride-s convolution multiplies s times the
    rows it keeps.)"""
    L, B, Cin = x.shape
    k = weight.shape[-1]
    Cout = weight.shape[1] if transposed else weight.shape[0]
    wcat = (weight.permute(2, 1, 0) if transposed else weight.permute(2, 0, 1)).reshape(k * Cout, Cin)  # row j * Cout + co
    y = linear(x.reshape(L * B, Cin), wcat, None).view(L, B, k, Cout)
    if transposed:
        L_out = (L - 1) * stride + dilation * (k - 1) + 1
        out = x.new_zeros(L_out, B, Cout)
        for j in range(k):
            sl = slice(j * dilation, j * dilation + (L - 1) * stride + 1, stride)
            out[sl] = out[sl] + y[:, :, j]
    else:
        L_out = (L - dilation * (k - 1) - 1) // stride + 1
        if L_out < 1:
            raise ValueError(f"dense_conv: input of {L} frames is shorter than the kernel's extent {dilation * (k - 1) + 1}")
        out = sum(y[j * dilation : j * dilation + (L_out - 1) * stride + 1 : stride, :, j] for j in range(k))
    return out + bias if bias is not None else out


class _SepBlockFunction(torch.autograd.Function):
    """One `BlockSeparable` (convolutional_coders.py:29-66) as a single autograd node on [L,B,C]:
    1x1 conv C->4C + ReLU (K6 epilogue) -> channel norm -> depthwise (transposed) conv k, stride s + ReLU -> channel norm
    -> 1x1 conv 4C->C (no bias) -> + nearest-resampled input.  params: w1 [4C,C], b1, g1, be1, wd [4C,k], bd, g2, be2,
    wp [C,4C]."""

    @staticmethod
    def forward(ctx, x, cfg, w1, b1, g1, be1, wd, bd, g2, be2, wp):
        stride, dilation, transposed, eps = cfg
        x = _f32c(x)
        w1, b1, g1, be1, wd, bd, g2, be2, wp = (_f32c(p) for p in (w1, b1, g1, be1, wd, bd, g2, be2, wp))
        L, B, C = x.shape
        Cb = w1.shape[0]
        a1 = torch.empty(L, B, Cb, device=x.device, dtype=torch.float32)
        gemm(0, 0, L * B, Cb, C, x, C, w1, C, a1, Cb, bias=b1, act=ACT_RELU)
        mr1, ss1 = _chan_norm_stats(a1, g1, be1, eps)  # norm 1 is applied inside the stencil's loads: never materialised
        d = _dwconv_fwd(a1, wd, bd, stride, dilation, transposed, True, in_affine=ss1)
        n2, mr2 = _chan_norm_fwd(d, g2, be2, eps)
        L2 = d.shape[0]
        r = torch.empty(L2, B, C, device=x.device, dtype=torch.float32)
        gemm(0, 0, L2 * B, C, Cb, n2, Cb, wp, Cb, r, C)
        out = torch.empty_like(r)
        check(load().blvm_resample_add_fwd(ptr(r), ptr(x), L2, L, B * C, ptr(out), stream_ptr()), "blvm_resample_add_fwd")
        ctx.cfg = cfg
        ctx.save_for_backward(x, a1, mr1, ss1, d, mr2, n2, w1, g1, wd, g2, wp)
        return out

    @staticmethod
    def backward(ctx, dout):
        stride, dilation, transposed, eps = ctx.cfg
        x, a1, mr1, ss1, d, mr2, n2, w1, g1, wd, g2, wp = ctx.saved_tensors
        dout = _f32c(dout)
        L, B, C = x.shape
        L2, Cb = d.shape[0], w1.shape[0]
        M, M2 = L * B, L2 * B
        dev = x.device
        # pointwise 4C->C
        dwp, dg2, dbe2, dwd, dbd, dg1, dbe1, dw1, db1 = _zeros_like_many([wp, g2, g2, wd, g2, g1, g1, w1, g1])
        gemm(1, 1, C, Cb, M2, dout, C, n2, Cb, dwp, Cb, accumulate=True, split_k=_pick_split(C, Cb, M2))
        dn2 = torch.empty(L2, B, Cb, device=dev, dtype=torch.float32)
        gemm(0, 1, M2, Cb, C, dout, C, wp, Cb, dn2, Cb)
        # norm 2 (+ the ReLU in front of it: d > 0 <=> pre-activation > 0)
        dd = _chan_norm_bwd(d, dn2, mr2, g2, True, dg2, dbe2)
        del dn2
        # depthwise conv
        dn1 = _dwconv_bwd(a1, wd, None, dd, stride, dilation, transposed, False, True, dwd, dbd, in_affine=ss1)
        del dd
        # norm 1 (+ ReLU of the 1x1 conv)
        da1 = _chan_norm_bwd(a1, dn1, mr1, g1, True, dg1, dbe1, dx_chan_sum=db1)  # db1 = column sums of da1, same pass
        del dn1
        # 1x1 conv C->4C
        gemm(1, 1, Cb, C, M, da1, Cb, x, C, dw1, C, accumulate=True, split_k=_pick_split(Cb, C, M))
        dx = None
        if ctx.needs_input_grad[0]:
            if L2 == L:
                dx = dout.clone()
            else:
                dx = torch.zeros_like(x)
                check(load().blvm_resample_add_bwd(ptr(dout), L2, L, B * C, ptr(dx), stream_ptr()), "blvm_resample_add_bwd")
            gemm(0, 1, M, C, Cb, da1, Cb, w1, C, dx, C, accumulate=True)
        return dx, None, dw1, db1, dg1, dbe1, dwd, dbd, dg2, dbe2, dwp


def sep_block(x, stride, dilation, transposed, w1, b1, g1, be1, wd, bd, g2, be2, wp, eps: float = 1e-5):
    return _SepBlockFunction.apply(x, (int(stride), int(dilation), bool(transposed), float(eps)), w1, b1, g1, be1, wd, bd, g2, be2, wp)


# ----------------------------------------------------------------------------------------------------------------------
# K9: CTC loss on un-normalised logits (log-softmax fused) and the greedy CTC decode
# ----------------------------------------------------------------------------------------------------------------------


def _ctc_call(logits, targets, il, tl, blank, d_nll, want_grad):
    T, B, C = logits.shape
    Lmax = targets.shape[1]
    lib = load()
    f32 = dict(device=logits.device, dtype=torch.float32)
    nll = torch.empty(B, **f32)
    d_logits = torch.empty_like(logits) if want_grad else None
    scratch = torch.empty(lib.blvm_ctc_scratch_floats(T, B, C, Lmax), **f32)
    check(
        lib.blvm_ctc_loss(ptr(logits), ptr(targets) if Lmax else None, ptr(il), ptr(tl), T, B, C, Lmax, int(blank), ptr(d_nll), ptr(nll),
                          ptr(d_logits), ptr(scratch), stream_ptr()),
        "blvm_ctc_loss",
    )  # fmt: skip
    return nll, d_logits


class _CTCFunction(torch.autograd.Function):
    """The forward is the loss-only call (the alpha recursion alone); the backward is the full call with the upstream gradient as d_nll:
    both recursions run side by side there, so it costs one serial pass as well."""

    @staticmethod
    def forward(ctx, logits, targets, il, tl, blank):
        nll, _ = _ctc_call(logits, targets, il, tl, blank, None, False)
        ctx.blank = blank
        ctx.save_for_backward(logits, targets, il, tl)
        return nll

    @staticmethod
    def backward(ctx, g):
        logits, targets, il, tl = ctx.saved_tensors
        _, d_logits = _ctc_call(logits, targets, il, tl, ctx.blank, g.to(torch.float32).contiguous(), True)
        return d_logits, None, None, None, None


def _ctc_lens(v, B, device, what):
    if torch.is_tensor(v) and v.is_cuda and v.dtype == torch.int32:
        out = v.contiguous()
    else:
        out = upload_i32(torch.as_tensor(v).reshape(-1), device)
    if out.shape != (B,):
        raise _hip.BlvmHipError(f"ctc: {what} must hold one length per row, [{B}], got {tuple(out.shape)}")
    return out


def ctc_loss(logits, targets, input_lens, target_lens, blank: int = 0):
    """nll [B] of `log_softmax(logits, 2)` + `nn.CTCLoss(blank, reduction="none", zero_infinity=False)`, differentiable wrt the
    UN-normalised time-major logits [T,B,C].  targets [B,Lmax] integers (host or device, right-padded); the lengths are host
    integers (uploaded like x_sl) or int32 device tensors."""
    ptr(logits)  # refuses a CPU tensor before anything else is touched
    if logits.dim() != 3:
        raise _hip.BlvmHipError(f"ctc_loss: logits must be time-major [T,B,C], got {tuple(logits.shape)}")
    T, B, C = logits.shape
    dev = logits.device
    targets = torch.as_tensor(targets)
    if targets.dim() != 2 or targets.shape[0] != B:
        raise _hip.BlvmHipError(f"ctc_loss: targets must be [B={B},Lmax], got {tuple(targets.shape)}")
    if not (targets.is_cuda and targets.dtype == torch.int32):
        targets = upload_i32(targets, dev) if not targets.is_cuda else targets.to(torch.int32)
    il, tl = _ctc_lens(input_lens, B, dev, "input_lens"), _ctc_lens(target_lens, B, dev, "target_lens")
    logits = _f32c(logits)
    return _CTCFunction.apply(logits, targets.contiguous(), il, tl, int(blank))


def ctc_greedy_device(logits, input_lens, blank: int = 0):
    """Greedy CTC decode of time-major logits [T,B,C], kept on the device: (hyp [B,T] int32, hyp_lens [B] int32).  Row b holds the
    arg-max labels of its first input_lens[b] frames with repeats collapsed and blanks dropped, hyp_lens[b] of them, -1 behind."""
    ptr(logits)
    if logits.dim() != 3:
        raise _hip.BlvmHipError(f"ctc_greedy: logits must be time-major [T,B,C], got {tuple(logits.shape)}")
    T, B, C = logits.shape
    logits = _f32c(logits.detach())
    il = _ctc_lens(input_lens, B, logits.device, "input_lens")
    hyp = torch.empty(B, T, device=logits.device, dtype=torch.int32)
    hyp_lens = torch.empty(B, device=logits.device, dtype=torch.int32)
    check(load().blvm_ctc_greedy(ptr(logits), ptr(il), T, B, C, int(blank), ptr(hyp), ptr(hyp_lens), stream_ptr()), "blvm_ctc_greedy")
    return hyp, hyp_lens


def ctc_greedy(logits, input_lens, blank: int = 0):
    """Greedy CTC decode of time-major logits [T,B,C] on the device: per row the arg-max labels of its first input_lens[b] frames with
    repeats collapsed and blanks dropped, as a list of lists of ints (`blvm.utils.decoding.greedy_ctc` is the host twin).  Only the
    [B,T] labels and [B] lengths are copied to the host."""
    hyp, hyp_lens = ctc_greedy_device(logits, input_lens, blank)
    hyp, hyp_lens = hyp.cpu().tolist(), hyp_lens.cpu().tolist()
    return [row[:n] for row, n in zip(hyp, hyp_lens)]


EDIT_MAX_REF_UNITS = 8192  # blvm_edit_distance: the expanded reference of a row (EDIT_MAX_REF, csrc/editdist.hip)
EDIT_STRIP_UNITS = 512  # hypothesis units the kernel walks per strip (EDIT_STRIP)
_edit_tables_cache = {}


def _edit_tables(tables, device):
    """(unit_offsets [n,V + 1], units, separators [n]) int32 on `device` for a tuple of `blvm.data.token_map.UnitTable`s over the same
    V tokens, the offsets shifted into one shared `units` array; uploaded once per tuple of tables and device."""
    key = (tuple(id(t) for t in tables), str(device))
    hit = _edit_tables_cache.get(key)
    if hit is None:
        V = len(tables[0])
        if V < 1 or any(len(t) != V for t in tables):
            raise _hip.BlvmHipError(f"edit_distance: the tables must share one V >= 1, got {[len(t) for t in tables]}")
        offsets, units = [], []
        for t in tables:
            offsets.append([len(units) + o for o in t.offsets])
            units.extend(t.units)
        i32 = dict(dtype=torch.int32, device=device)
        hit = (torch.tensor(offsets, **i32), torch.tensor(units or [0], **i32), torch.tensor([t.separator for t in tables], **i32),
               tuple(tables))  # the tables themselves: their ids stay taken while the entry lives
        _edit_tables_cache[key] = hit
    return hit[:3]


def edit_distance_fits(ref_stride: int, tables=None) -> bool:
    """Whether reference rows of `ref_stride` tokens are within blvm_edit_distance's limit under `tables` (None: compared as they
    are): the bound of a row's expansion, every token at its table's longest and a separator after all but the last."""
    if not tables:
        return ref_stride <= EDIT_MAX_REF_UNITS
    return ref_stride * (max(t.max_units for t in tables) + 1) - 1 <= EDIT_MAX_REF_UNITS


def _edit_seq(v, device, what):
    v = torch.as_tensor(v)
    if v.dim() != 2:
        raise _hip.BlvmHipError(f"edit_distance: {what} must be [B,stride], got {tuple(v.shape)}")
    if not (v.is_cuda and v.dtype == torch.int32):
        v = upload_i32(v, device) if not v.is_cuda else v.to(torch.int32)
    return v.contiguous()


def _edit_call(ref, ref_lens, hyp, hyp_lens, tables, want_totals):
    hyp = torch.as_tensor(hyp)
    if not hyp.is_cuda:
        ptr(hyp)  # refuses a CPU tensor before anything else is touched: the hypotheses name the device
    dev = hyp.device
    hyp, ref = _edit_seq(hyp, dev, "hyp"), _edit_seq(ref, dev, "ref")
    B = hyp.shape[0]
    if ref.shape[0] != B:
        raise _hip.BlvmHipError(f"edit_distance: ref has {ref.shape[0]} rows, hyp {B}")
    rl, hl = _ctc_lens(ref_lens, B, dev, "ref_lens"), _ctc_lens(hyp_lens, B, dev, "hyp_lens")
    n = len(tables)
    off, units, seps = _edit_tables(tables, dev) if n else (None, None, None)
    i32 = dict(device=dev, dtype=torch.int32)
    edits, ref_units = torch.empty(max(n, 1), B, **i32), torch.empty(max(n, 1), B, **i32)
    totals = torch.empty(max(n, 1), 3, **i32) if want_totals else None
    check(
        load().blvm_edit_distance(ptr(ref) if ref.shape[1] else None, ptr(rl), ref.shape[1], ptr(hyp) if hyp.shape[1] else None, ptr(hl),
                                  hyp.shape[1], B, n, len(tables[0]) if n else 0, ptr(off), ptr(units), ptr(seps),
                                  max(t.max_units for t in tables) if n else 0, ptr(edits), ptr(ref_units), ptr(totals), stream_ptr()),
        "blvm_edit_distance",
    )  # fmt: skip
    return edits, ref_units, totals


def edit_distance(ref, ref_lens, hyp, hyp_lens, table=None):
    """Levenshtein distance (unit-cost substitutions, insertions, deletions) per row between ref[b,:ref_lens[b]] and
    hyp[b,:hyp_lens[b]] -> (edits, ref_units) int32 device tensors.  `hyp` [B,stride] is a device tensor of integers (as
    `ctc_greedy_device` gives it; what lies behind a row's length is never read); `ref` [B,stride] may be host or device integers,
    the lengths host integers or int32 device tensors.  table: None compares the sequences as they are; a
    `blvm.data.token_map.UnitTable` expands every token to its units first (`expand_units` is the host twin) and gives [B]
    results; a list or tuple of tables over the same tokens is served by ONE launch and gives [n_tables,B].  ref_units is the
    expanded reference's length.  A row with a token outside the table or a length outside its stride gets -1 in both."""
    single = table is None or not isinstance(table, (list, tuple))
    tables = () if table is None else ((table,) if single else tuple(table))
    edits, ref_units, _ = _edit_call(ref, ref_lens, hyp, hyp_lens, tables, False)
    return (edits[0], ref_units[0]) if single else (edits, ref_units)


def ctc_error_totals(logits, input_lens, targets, target_lens, tables, blank: int = 0):
    """The greedy decode of time-major logits [T,B,C] and its edit distances to the targets under each of `tables`
    (`blvm.data.token_map.UnitTable`s, e.g. `TokenMap.unit_tables()`), with nothing copied to the host -> (totals [n_tables,3] int32,
    hyp [B,T] int32, hyp_lens [B] int32).  totals[k] = (sum of edits, sum of reference units, number of refused rows) under table k;
    refused rows (a label outside the table, a length outside its row) add to neither sum.  Three launches: the decode, the
    distances of every (row, table), and the batch sums, a one-wave kernel per table that adds in a fixed order (no atomics)."""
    hyp, hyp_lens = ctc_greedy_device(logits, input_lens, blank)
    tables = tuple(tables)
    if not tables:
        raise _hip.BlvmHipError("ctc_error_counts: needs at least one unit table")
    _, _, totals = _edit_call(targets, target_lens, hyp, hyp_lens, tables, True)
    return totals, hyp, hyp_lens


def ctc_error_counts(logits, input_lens, targets, target_lens, tables, blank: int = 0):
    """`ctc_error_totals` as (counts [n_tables,2] int32: the sum of edits and of reference units over the batch's accepted rows,
    invalid [n_tables] int32: the number of refused rows), both views of one device tensor."""
    totals, _, _ = ctc_error_totals(logits, input_lens, targets, target_lens, tables, blank)
    return totals[:, :2], totals[:, 2]


# ----------------------------------------------------------------------------------------------------------------------
# K10: log-mel spectrogram front end
# ----------------------------------------------------------------------------------------------------------------------


def logmel_check_geometry(n_fft: int, win_length: int, hop_length: int, n_mels: int):
    """The range blvm_logmel takes (the library checks it again): raises BlvmHipError with the offending value."""
    if not (n_fft % 2 == 0 and 2 <= n_fft <= 1024):
        raise _hip.BlvmHipError(f"log_mel_spectrogram: n_fft = {n_fft}: need an even n_fft of at most 1024")
    if not 16 <= win_length <= n_fft:
        raise _hip.BlvmHipError(f"log_mel_spectrogram: win_length = {win_length}: need 16 <= win_length <= n_fft = {n_fft}")
    if hop_length < 1:
        raise _hip.BlvmHipError(f"log_mel_spectrogram: hop_length = {hop_length}: need hop_length >= 1")
    if not 1 <= n_mels <= 128:
        raise _hip.BlvmHipError(f"log_mel_spectrogram: n_mels = {n_mels}: need 1 <= n_mels <= 128")


def logmel_check_lengths(lengths, n_fft: int, Lmax: int):
    """Host lengths of the rows of a [B,Lmax] batch: every row needs more than n_fft // 2 samples (one reflection about its own
    ends must reach every tap of its first and last frame, as in torch.stft) and no more than the batch holds."""
    for b, v in enumerate(lengths):
        if not n_fft // 2 < int(v) <= Lmax:
            raise _hip.BlvmHipError(f"log_mel_spectrogram: row {b} has {int(v)} samples: every row needs more than n_fft // 2 = "
                                    f"{n_fft // 2} (reflect padding) and at most Lmax = {Lmax}")


def logmel_frames(length: int, hop_length: int) -> int:
    """Frames of an utterance of `length` samples: centred frames, one per hop, the last one centred at or before the end."""
    return 1 + int(length) // int(hop_length)


def logmel_basis(n_fft: int, win_length: int) -> torch.Tensor:
    """float64 [win_length, 2, n_fft // 2 + 1]: the windowed DFT of the win_length non-zero taps of a frame.  [n, 0, k] =
    w[n] cos(2 pi k (left + n) / n_fft), [n, 1, k] = w[n] sin(same), w the periodic Hann window of win_length and left =
    (n_fft - win_length) // 2 the zero taps in front of it.  The phase is reduced in integers before it is scaled."""
    n = torch.arange(win_length, dtype=torch.int64)
    k = torch.arange(n_fft // 2 + 1, dtype=torch.int64)
    left = (n_fft - win_length) // 2
    w = 0.5 - 0.5 * torch.cos(2.0 * torch.pi * n.double() / win_length)
    phase = ((left + n)[:, None] * k[None, :] % n_fft).double() * (2.0 * torch.pi / n_fft)
    return torch.stack([w[:, None] * torch.cos(phase), w[:, None] * torch.sin(phase)], dim=1)


def logmel_filterbank(sample_rate: int, n_fft: int, n_mels: int) -> torch.Tensor:
    """float64 [n_fft // 2 + 1, n_mels]: triangular filters on the HTK mel scale from 0 to sample_rate / 2, not normalised
    (torchaudio's `melscale_fbanks(norm=None, mel_scale="htk")`)."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_fft // 2 + 1, dtype=torch.float64)
    m_max = 2595.0 * torch.log10(torch.tensor(1.0 + (sample_rate / 2) / 700.0, dtype=torch.float64))
    m_pts = torch.linspace(0.0, float(m_max), n_mels + 2, dtype=torch.float64)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]
    down, up = -slopes[:, :-2] / f_diff[:-1], slopes[:, 2:] / f_diff[1:]
    return torch.clamp_min(torch.minimum(down, up), 0.0)


_logmel_operands_cache = {}


def _round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def _logmel_operands(device, sample_rate: int, n_fft: int, win_length: int, n_mels: int):
    """(basis [WP,2,NBP], fbank [NBP,NMP]) in fp32 on `device`, zero-padded as blvm_logmel reads them; built once per geometry."""
    key = (str(device), sample_rate, n_fft, win_length, n_mels)
    hit = _logmel_operands_cache.get(key)
    if hit is None:
        n_bins = n_fft // 2 + 1
        WP, NBP, NMP = _round_up(win_length, 8), _round_up(n_bins, 32), _round_up(n_mels, 32)
        basis = torch.zeros(WP, 2, NBP, dtype=torch.float32)
        basis[:win_length, :, :n_bins] = logmel_basis(n_fft, win_length).to(torch.float32)
        fbank = torch.zeros(NBP, NMP, dtype=torch.float32)
        fbank[:n_bins, :n_mels] = logmel_filterbank(sample_rate, n_fft, n_mels).to(torch.float32)
        hit = _logmel_operands_cache[key] = (basis.to(device), fbank.to(device))
    return hit


def log_mel_spectrogram(wave, lens, sample_rate: int, n_fft: int, win_length: int, hop_length: int, n_mels: int, normalize: bool = True):
    """(features [B,n_mels,T_max], feature_lens [B] int32 on the device) of a batch of right-padded waveforms [B,Lmax]: power
    spectrogram of centred, reflect-padded frames (periodic Hann of win_length) -> HTK mel filters -> 10 log10(max(., 1e-10)) and,
    with `normalize`, per utterance and mel bin (x - mean) / (std + 1e-10) over the utterance's own T_b = 1 + L_b // hop_length
    frames (unbiased std: an utterance of a single frame normalises to NaN, as torch.std gives).  Columns behind T_b are 0.
    `lens` are host integers (checked here: every row needs more than n_fft // 2 samples, as torch.stft's reflect padding does) or
    an int32 device tensor (not read back: a row with a length outside (n_fft // 2, Lmax] comes out NaN with feature length 0)."""
    ptr(wave)  # refuses a CPU tensor before anything else is touched
    if wave.dim() != 2:
        raise _hip.BlvmHipError(f"log_mel_spectrogram: wave must be [B,Lmax], got {tuple(wave.shape)}")
    n_fft, win_length, hop_length, n_mels = int(n_fft), int(win_length), int(hop_length), int(n_mels)
    logmel_check_geometry(n_fft, win_length, hop_length, n_mels)
    B, Lmax = wave.shape
    dev = wave.device
    if torch.is_tensor(lens) and lens.is_cuda and lens.dtype == torch.int32:
        lens_dev = lens.contiguous()
    else:
        host = torch.as_tensor(lens).reshape(-1).to(torch.int64)
        logmel_check_lengths(host.tolist(), n_fft, Lmax)
        lens_dev = upload_i32(host, dev)
    if lens_dev.shape != (B,):
        raise _hip.BlvmHipError(f"log_mel_spectrogram: lens must hold one length per row, [{B}], got {tuple(lens_dev.shape)}")
    wave = _f32c(wave.detach())
    basis, fbank = _logmel_operands(dev, int(sample_rate), n_fft, win_length, n_mels)
    out = torch.empty(B, n_mels, logmel_frames(Lmax, hop_length), device=dev, dtype=torch.float32)
    out_lens = torch.empty(B, device=dev, dtype=torch.int32)
    check(
        load().blvm_logmel(ptr(wave), ptr(lens_dev), B, Lmax, n_fft, win_length, hop_length, n_mels, ptr(basis), ptr(fbank),
                           int(bool(normalize)), ptr(out), ptr(out_lens), stream_ptr()),
        "blvm_logmel",
    )  # fmt: skip
    return out, out_lens
