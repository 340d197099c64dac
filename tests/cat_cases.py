"""Cases and float64 truth for the categorical head (K7d, csrc/cathead.hip): one place that defines the op-level inputs (shapes x
regimes), the truth (`log_softmax` + gather + mask in float64, with its autograd), the same composition in float32 — the arithmetic of
the reference's `CategoricalDense` + `categorical_ll(reduce_dim=None)`, which tests/golden/categorical.npz pins on sampled elements —,
the any-order fp32 floors of the per-element bar, and the sampler's draw check.  TEST INFRASTRUCTURE: not imported by the product.

Inputs come from numpy's RandomState (stable across versions), so the fixture's generator and the tests build identical cases.
"""
import numpy as np
import torch

U = 2.0**-24

# (B, skip = T', S, C, V): what each shape exercises is tabulated in tests/test_gpu_categorical.py
SHAPES = [(3, 43, 1, 16, 10), (2, 33, 2, 32, 256), (1, 130, 1, 96, 1000), (5, 13, 1, 64, 4096), (2, 9, 1, 512, 256)]
REGIMES = ["random", "peaked", "equal", "last_class", "empty_utterance", "garbage_padding"]
N_SAMPLED = 8  # frames / classes per case whose reference gradients the fixture stores


def case_id(shape, regime):
    return "B{}_T{}_S{}_C{}_V{}_{}".format(*shape, regime)


def lengths(B, T, regime):
    x_sl = torch.tensor([max(1, T - (k * T) // (B + 1) - (k % 3)) for k in range(B)])
    if regime == "empty_utterance":
        x_sl[B - 1] = 0
    if regime == "garbage_padding":
        x_sl = (x_sl - 3).clamp(min=1)
    return x_sl


def make_case(shape, regime):
    """X [B, T'*S, C] frames (batch-major, zeros where a frame does not count), W [V,C], b [V], y [B,T] int64 (0 where masked), g [B]
    the incoming gradient, x_sl [B], valid [B, T'*S].  `X_in` / `y_in` are what the kernels get: the same, except that in the
    garbage_padding regime every frame that does not count holds NaN activations and an out-of-range target (-7 or V + 5)."""
    B, Tp, S, C, V = shape
    seed = 1000 * SHAPES.index(tuple(shape)) + REGIMES.index(regime)
    rng = np.random.RandomState(seed)
    T = Tp * S - S // 2
    x_sl = lengths(B, T, regime)
    tau = torch.arange(Tp * S)
    valid = tau.unsqueeze(0) < torch.minimum(x_sl, torch.tensor(T)).unsqueeze(1)  # [B, T'*S]
    X = torch.from_numpy(rng.standard_normal((B, Tp * S, C)).astype(np.float32))
    W = torch.from_numpy((rng.standard_normal((V, C)) / np.sqrt(C)).astype(np.float32))
    b = torch.from_numpy((0.1 * rng.standard_normal(V)).astype(np.float32))
    y = torch.from_numpy(rng.randint(0, V, size=(B, T)).astype(np.int64))
    g = torch.from_numpy((0.5 + rng.rand(B)).astype(np.float32)) * torch.tensor([1.0, -1.0])[torch.arange(B) % 2]
    if regime == "peaked":  # per-frame range of the logits about 80: random targets then have probabilities down to ~e^-100
        l = X.double() @ W.double().t() + b.double()
        k = 80.0 / float((l.max(-1).values - l.min(-1).values).mean())
        W, b = (W.double() * k).float(), (b.double() * k).float()
    elif regime == "equal":
        W, b = torch.zeros_like(W), torch.full_like(b, 0.3)
    elif regime == "last_class":  # the maximum and the target both in the last class of the last (partial) class tile
        b[V - 1] += 10.0
        y[:] = V - 1
    X = X * valid.unsqueeze(-1)
    y = y * valid[:, :T]
    X_in, y_in = X.clone(), y.clone()
    if regime == "garbage_padding":
        X_in[~valid] = float("nan")
        wild = torch.where(torch.arange(T) % 2 == 0, torch.tensor(-7), torch.tensor(V + 5)).expand(B, T)
        y_in = torch.where(valid[:, :T], y, wild)
    return dict(shape=tuple(shape), regime=regime, B=B, Tp=Tp, S=S, C=C, V=V, T=T, x_sl=x_sl, valid=valid, X=X, W=W, b=b, y=y, g=g,
                X_in=X_in, y_in=y_in)  # fmt: skip


def to_rows(frames, B, Tp, S):
    """batch-major frames [B, T'*S, F] -> the kernels' time-major rows [T'*B, S*F]."""
    F = frames.shape[-1]
    return frames.reshape(B, Tp, S * F).transpose(0, 1).reshape(Tp * B, S * F).contiguous()


def from_rows(rows, B, Tp, S):
    """time-major rows [T'*B, S*F] -> batch-major frames [B, T'*S, F]."""
    F = rows.shape[-1] // S
    return rows.reshape(Tp, B, S * F).transpose(0, 1).reshape(B, Tp * S, F).contiguous()


def compose(case, dtype):
    """Linear -> log_softmax -> gather at y -> mask -> per-utterance sums, and autograd of sum_b g_b log_prob_b, all in `dtype` on the
    CPU.  float64: the truth.  float32: the reference's arithmetic (`nn.Linear`, `logits - logits.logsumexp`, `.gather`)."""
    T, valid = case["T"], case["valid"]
    X = case["X"].detach().clone().to(dtype).requires_grad_(True)
    W = case["W"].detach().clone().to(dtype).requires_grad_(True)
    b = case["b"].detach().clone().to(dtype).requires_grad_(True)
    logits = torch.nn.functional.linear(X, W, b)  # [B, T'*S, V]
    lse = logits.logsumexp(dim=-1)
    lsm = logits - lse.unsqueeze(-1)
    ll = lsm[:, :T].gather(-1, case["y"].unsqueeze(-1)).squeeze(-1) * valid[:, :T].to(dtype)
    log_prob = ll.sum(1)
    (log_prob * case["g"].to(dtype)).sum().backward()
    return dict(logits=logits.detach(), lse=lse.detach(), ll=ll.detach(), log_prob=log_prob.detach(), d_x=X.grad, dW=W.grad, db=b.grad)


def floors(case, t64):
    """The any-order fp32 bounds of the bar, from the float64 truth `t64` (u = 2^-24, A_r = max_k (sum_c |x_rc w_kc| + |b_k|)):
        floor_ll   = 2 (C + 2) u A_r + 64 u (1 + |l_y| + |lse|)
        eps_rk     = 2 (C + 2) u A_r + 64 u (1 + |l_k| + |lse|)                    (relative error of p_k = exp(l_k - lse))
        floor_ddec = sum_k |w_kc| |g| p_k eps_rk + (V + 2) u sum_k |d_rk w_kc|
        floor_dW   = sum_r |x_rc| |g| p_k eps_rk + 2 n u sum_r |d_rk x_rc|         (n counted frames);  floor_db: the same with x = 1
    -> dict(ll [B,T], d_x [B,T'*S,C], dW [V,C], db [V])."""
    B, T, C, V, valid = case["B"], case["T"], case["C"], case["V"], case["valid"]
    X, W, b = case["X"].double(), case["W"].double(), case["b"].double()
    l, lse = t64["logits"], t64["lse"]
    A = (X.abs() @ W.abs().t() + b.abs()).max(-1).values  # [B, T'*S]
    prod = 2 * (C + 2) * U * A
    Tall = valid.shape[1]
    ypad = torch.zeros(B, Tall, dtype=torch.int64)
    ypad[:, :T] = case["y"]
    l_y = l.gather(-1, ypad.unsqueeze(-1)).squeeze(-1)
    floor_ll = (prod + 64 * U * (1 + l_y.abs() + lse.abs()))[:, :T]
    eps = prod.unsqueeze(-1) + 64 * U * (1 + l.abs() + lse.abs().unsqueeze(-1))  # [B, T'*S, V]
    gm = (case["g"].double().unsqueeze(1) * valid.double()).unsqueeze(-1)  # [B, T'*S, 1]
    p = (l - lse.unsqueeze(-1)).exp()
    onehot = torch.zeros_like(p).scatter_(-1, ypad.unsqueeze(-1), 1.0)
    d = gm * (onehot - p)
    pe = gm.abs() * p * eps
    n = float(valid.sum())
    floor_dx = pe @ W.abs() + (V + 2) * U * (d.abs() @ W.abs())
    pe2, d2, X2 = pe.reshape(-1, V), d.reshape(-1, V), X.reshape(-1, C)
    floor_dW = pe2.t() @ X2.abs() + 2 * n * U * (d2.abs().t() @ X2.abs())
    floor_db = pe2.sum(0) + 2 * n * U * d2.abs().sum(0)
    return dict(ll=floor_ll, d_x=floor_dx, dW=floor_dW, db=floor_db)


def check_bar(name, got, truth, ref32, floor, where=None):
    """Per element |got - truth| <= max(4 |ref32 - truth|, floor); the message names the quantity, the worst element and its margin."""
    got, truth, ref32 = (t.detach().double().cpu().reshape(-1) for t in (got, truth, ref32))
    floor = floor.double().reshape(-1)
    err = (got - truth).abs()
    bar = torch.maximum(4 * (ref32 - truth).abs(), floor)
    ratio = torch.nan_to_num(err / bar, nan=float("inf"))
    ratio = torch.where((err == 0) & (bar == 0), torch.zeros_like(ratio), ratio)
    i = int(ratio.argmax())
    at = where(i) if where is not None else i
    msg = (f"{name}: worst at {at}: hip {float(got[i]):.9g} truth {float(truth[i]):.9g} err {float(err[i]):.3e} bar {float(bar[i]):.3e} "
           f"(ref32 err {float((ref32[i] - truth[i]).abs()):.3e}, floor {float(floor[i]):.3e}); margin err/bar {float(ratio[i]):.3g}")  # fmt: skip
    print(msg)
    assert float(ratio[i]) <= 1.0, msg
    return float(ratio[i])


def sampled(case):
    """The frames (flat batch-major indices into [B * T'*S]) and classes whose reference gradients the fixture stores: the first, the
    last, and an even spread in between (the last class is the class-tile tail)."""
    n_fr, V = case["B"] * case["Tp"] * case["S"], case["V"]
    fr = torch.linspace(0, n_fr - 1, N_SAMPLED).round().long().unique()
    cl = torch.linspace(0, V - 1, N_SAMPLED).round().long().unique()
    return fr, cl


# ---- sampler ---------------------------------------------------------------------------------------------------------------------

SAMPLER_V = [10, 256, 65536]
SAMPLER_REGIMES = ["random", "peaked", "equal"]
SAMPLER_ROWS = 64


def sampler_case(V, regime):
    """logits [64, V] float32 and uniforms [64] (the ends 0 and 1 - 2^-24 included)."""
    rng = np.random.RandomState(7000 + 10 * SAMPLER_V.index(V) + SAMPLER_REGIMES.index(regime))
    l = rng.standard_normal((SAMPLER_ROWS, V))
    if regime == "peaked":
        l = l * 20.0
    elif regime == "equal":
        l = np.zeros_like(l) + 0.3
    u = rng.rand(SAMPLER_ROWS)
    u[0], u[1] = 0.0, 1.0 - U
    return torch.from_numpy(l.astype(np.float32)), torch.from_numpy(u.astype(np.float32))


def check_draws(logits, u, k_hat):
    """Every draw: c_{k-1} - tol <= u S <= c_k + tol with c the float64 prefix sums of e = exp(l - max l), S their total and
    tol = V 2^-23 S, the any-order bound of a V-term fp32 sum plus the roundings of the exponentials.  -> the worst margin."""
    l = logits.double()
    V = l.shape[-1]
    e = (l - l.max(-1, keepdim=True).values).exp()
    c = e.cumsum(-1)
    S = c[:, -1]
    tol = V * 2.0**-23 * S
    k = k_hat.long().cpu()
    assert k.shape == u.shape and int(k.min()) >= 0 and int(k.max()) < V, f"draws outside [0, {V}): {k.min()} .. {k.max()}"
    target = u.double() * S
    c_k = c.gather(-1, k.unsqueeze(-1)).squeeze(-1)
    c_km1 = torch.where(k > 0, c.gather(-1, (k - 1).clamp(min=0).unsqueeze(-1)).squeeze(-1), torch.zeros_like(S))
    low, high = (c_km1 - target) / tol, (target - c_k) / tol  # each <= 1 passes
    worst = torch.maximum(low, high)
    i = int(worst.argmax())
    assert float(worst[i]) <= 1.0, (f"draw {i}: class {int(k[i])} for u = {float(u[i])}: c[k-1] {float(c_km1[i]):.9g} u*S {float(target[i]):.9g} "
                                    f"c[k] {float(c_k[i]):.9g} tol {float(tol[i]):.3e}")  # fmt: skip
    return float(worst[i])
