"""GPU (MI355X): K7b, the Gaussian-mixture head, at component counts other than ten (the general arm of csrc/dmol.hip), per frame and
per element against the CPU oracle in float64.

Inputs: the trained regime of tests/golden/heads_stress.npz (oracle/gen_golden.py::gen_heads_stress) generated here from a seed for
n components: 256 frames, beta = 2.5, sd_eps = 1e-4; a quarter of the frames with every sd at the sd_eps floor, a quarter with
beta * raw either side of the softplus threshold, a quarter with one dominant component (logit spread > 90); every mean 0..3 sds away
from its target.

Bar, as tests/test_gpu_heads.py: |hip - truth| <= max(4 |ref32 - truth|, floor), truth = the float64 oracle, ref32 = the same oracle in
float32.  The floors are that file's with the term count n in place of 10 (its groups of ten become groups of n):
  * floor_ll = 64 u S_f, S_f = 1 + |ll| + max |logit|, u = 2^-24.  The constant holds for every n <= 16: a component's log-density
    is ~12 roundings on quantities <= S_f (rcp, (y - mu) / sd, its square, log sd, logit - lse), the two log-sum-exps add n + 3
    roundings each on weights <= 1 — 18 + 2 n <= 50 < 64 — and the components enter the result as a convex combination, not a sum;
  * floor_g = 64 u S_f (|g| + term size) + 2^-100, term size = the largest entry of the entry's group of n (means | raw sds), for a
    logit the responsibility and the softmax weight it is the difference of;
  * through a fused Linear W: d_par as above, d_dec = d_par W gets floor_par |W| + 64 u (|d_par| |W|) (test_heads_random_linear's rule).
W, bias and the activations lie on grids (2^-6, 2^-14, 2^-8) that make W dec + b exact in float32, so the bars measure the likelihood
and the product with W, not the conditioning of rounded head outputs.
Ten components run through the same cases: they take the kernels they took before the general arm existed and must meet the same bars."""
import pytest
import torch

import blvm_oracle as O
from blvm import _hip, ops

from test_gpu_heads import ABS, SENTINEL, U, check_bar, dev_buf, from_rows, p_, to_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BETA, SD_EPS = 2.5, 1e-4
LIB = None


@pytest.fixture(scope="module", autouse=True)
def _require_hip():
    global LIB
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    LIB = _hip.load()
    assert LIB.blvm_device_ok() == 1, "libblvm_hip: no gfx950 device visible"


def stress_frames(n, seed):
    """heads_stress.npz's Gaussian-mixture frames for n components -> (par [256, 3n] = logits | means | raw sds, y [256])."""
    g = torch.Generator().manual_seed(seed)
    N = 256
    y = torch.rand(N, generator=g) * 2 - 1
    logits = torch.randn(N, n, generator=g) * 2
    logits[192:, 0] = 60.0
    if n > 1:
        logits[192:, 1:] = -40.0 - 20 * torch.rand(64, n - 1, generator=g)
    raw = torch.randn(N, n, generator=g)
    raw[0:64] = -40.0 / BETA
    cross = torch.tensor([19.0, 19.99, 20.0, 20.01, 21.0, 30.0]) / BETA
    raw[64:128] = cross[torch.randint(0, len(cross), (64, n), generator=g)]
    sd = torch.nn.functional.softplus(raw.double(), beta=BETA) + SD_EPS
    mu = (y.double().unsqueeze(1) - torch.randn(N, n, generator=g).double() * 3 * sd).float()
    return torch.cat([logits, mu, raw], 1), y


def gmm_ll(par, y, n):
    sd = torch.nn.functional.softplus(par[:, 2 * n :], beta=BETA) + SD_EPS
    return O.gaussian_mixture_ll(y.unsqueeze(1), par[:, :n], par[:, n : 2 * n].unsqueeze(1), sd.unsqueeze(1), epsilon=0)


def scale_f(par, ll, n):
    return 1 + ll.abs() + par[:, :n].double().abs().max(1).values


def floor_grad(par, ll, g, n):
    S_f = scale_f(par, ll, n).unsqueeze(1)
    gm = torch.zeros_like(g)
    for sl in (slice(n, 2 * n), slice(2 * n, 3 * n)):
        gm[:, sl] = g[:, sl].abs().max(1, keepdim=True).values
    pm = torch.softmax(par[:, :n].double(), 1)
    gm[:, :n] = (pm + g[:, :n]).abs() + pm
    return 64 * U * S_f * (g.abs() + gm) + ABS


def layout_of(Tp, S):
    """B = 3: a full utterance, a ragged one, an EMPTY one; the last S // 2 frames of every row set lie beyond T."""
    T_ = Tp * S - S // 2
    x_sl = torch.tensor([T_, max(1, (2 * T_) // 3 - 1), 0])
    valid = torch.arange(Tp * S).unsqueeze(0) < x_sl.unsqueeze(1)
    return T_, x_sl, valid


def run_abi(n, dec_rows, W, bias, y, x_sl, g_b, layout, B, T_, Tp, S):
    dec = dev_buf(dec_rows, False)
    Wd = W.contiguous().to(DEV) if W is not None else None
    bd = bias.contiguous().to(DEV) if bias is not None else None
    yd, xs, gb = y.contiguous().to(DEV), x_sl.to(DEV, torch.int32), g_b.float().to(DEV)
    lp = torch.zeros(B, device=DEV, dtype=torch.float64)
    ll = torch.full((B, T_), SENTINEL, device=DEV)
    d_dec = torch.full((dec.numel(),), float("nan"), device=DEV)
    d_par = torch.full((dec.numel(),), float("nan"), device=DEV) if W is not None else None
    a = (p_(dec), layout, p_(Wd), p_(bd), p_(yd), p_(xs))
    _hip.check(LIB.blvm_gmm_fwd(*a, B, T_, Tp, S, n, BETA, SD_EPS, p_(lp), p_(ll), _hip.stream_ptr()), "gmm_fwd")
    _hip.check(LIB.blvm_gmm_bwd(*a, p_(gb), B, T_, Tp, S, n, BETA, SD_EPS, p_(d_dec), p_(d_par), _hip.stream_ptr()), "gmm_bwd")
    torch.cuda.synchronize()
    return ll.cpu(), lp.cpu(), d_dec.view(B * Tp, -1), (d_par.view(B * Tp, -1) if d_par is not None else None)


def gmm_case(n, Tp, S, layout, linear, seed):
    B, F = 3, 3 * n
    par, y = stress_frames(n, 4000 + n)
    T_, x_sl, valid = layout_of(Tp, S)
    assert (B * Tp * S) % 256 != 0 and B * Tp * S > 256, "set-up: more than one workgroup, the last one partly filled"
    gen = torch.Generator().manual_seed(1000 + seed)
    idx_all = (torch.arange(B * Tp * S) * 37 + seed) % par.shape[0]
    g_b = torch.randn(B, generator=gen)
    if linear:
        W = torch.eye(F) + torch.randint(-4, 5, (F, F), generator=gen).float() * (1 - torch.eye(F)) / 64
        bias = torch.randint(-256, 257, (F,), generator=gen).float() / 2**14
        dec_f = torch.linalg.solve(W.double(), (par[idx_all].double() - bias.double()).t()).t()
        dec_f = (dec_f.clamp(-63, 63) * 256).round().div(256).float().view(B, Tp * S, F)
    else:
        W = bias = None
        dec_f = par[idx_all].view(B, Tp * S, F).clone()
    # garbage (finite) in every padded frame and target
    pad_fr = torch.randn(B, Tp * S, F, generator=gen) * 8
    dec_in = torch.where(valid.unsqueeze(-1), dec_f, pad_fr)
    y_fr = y[idx_all].view(B, Tp * S)
    yy = torch.where(valid[:, :T_], y_fr[:, :T_], torch.full((B, T_), 5.0))
    bi, ti = valid.nonzero(as_tuple=True)

    def oracle(dt):
        d0 = dec_f.to(dt).clone().requires_grad_(True)
        pp = d0[valid] @ W.to(dt).t() + bias.to(dt) if linear else d0[valid] * 1
        pp.retain_grad()
        ll = gmm_ll(pp, y_fr[valid].to(dt), n)
        lp = torch.zeros(B, dtype=torch.float64).index_add(0, bi, ll.double())
        (lp * g_b.double()).sum().backward()
        return ll.detach().double(), lp.detach(), d0.grad.double()[valid], pp.grad.double(), pp.detach().double()

    r32, tr = oracle(torch.float32), oracle(torch.float64)
    ll, lp, d_dec, d_par = run_abi(n, to_rows(dec_in, B, Tp, S, layout), W, bias, yy, x_sl, g_b, layout, B, T_, Tp, S)
    frame_of = lambda i: f"frame (b={int(bi[i])}, tau={int(ti[i])})"  # noqa: E731
    name = f"gmm n={n} S={S} layout={layout} {'W' if linear else 'W=NULL'}"
    margins = {}
    S_f = scale_f(tr[4], tr[0], n)
    margins["ll"] = check_bar(f"{name} ll", ll[valid[:, :T_]], tr[0], r32[0], 64 * U * S_f, frame_of)
    pad = ~valid[:, :T_]
    assert bool((ll[pad] == SENTINEL).all()), f"{name}: ll_twise written in a padded frame"
    own = (ll.double() * valid[:, :T_]).sum(1)
    assert torch.allclose(lp, own, rtol=1e-12, atol=1e-9), f"{name} lp: per-utterance sums {lp} != sums of ll_twise {own}"
    assert float(lp[2]) == 0.0, f"{name}: the empty utterance's sum is {float(lp[2])}"
    fl_lp = torch.zeros(B, dtype=torch.float64).index_add(0, bi, 64 * U * S_f) + ABS  # (the empty utterance: 0 against 0)
    margins["lp"] = check_bar(f"{name} lp", lp, tr[1], r32[1], fl_lp, lambda i: f"utterance {i}")
    # gradient w.r.t. the head outputs in float64 (per frame, before the upstream factor) for the floors
    p64 = tr[4].clone().requires_grad_(True)
    gmm_ll(p64, y_fr[valid].double(), n).sum().backward()
    gbv = g_b.double()[bi].unsqueeze(1)
    fl_par = floor_grad(tr[4], tr[0], p64.grad, n) * gbv.abs()
    dd = from_rows(d_dec, B, Tp, S, layout, F)
    assert bool((dd[~valid] == 0).all()), f"{name} d_dec: nonzero in a padded frame ({int((dd[~valid] != 0).sum())} entries)"
    entry = lambda i: frame_of(i // F) + f" entry {i % F}"  # noqa: E731
    if linear:
        dp = from_rows(d_par, B, Tp, S, layout, F)
        assert bool((dp[~valid] == 0).all()), f"{name} d_par: nonzero in a padded frame"
        margins["d_par"] = check_bar(f"{name} d_par", dp[valid], tr[3], r32[3], fl_par, entry)
        d_in = fl_par @ W.double().abs() + 64 * U * ((p64.grad * gbv).abs() @ W.double().abs())
        margins["d_dec"] = check_bar(f"{name} d_dec", dd[valid], tr[2], r32[2], d_in, entry)
    else:
        assert d_par is None
        margins["d_dec"] = check_bar(f"{name} d_dec", dd[valid], tr[2], r32[2], fl_par, entry)
    print(f"[{name}] worst err / bar: " + ", ".join(f"{k} {v:.3g}" for k, v in margins.items()))


SHAPES = [(100, 1), (20, 5), (2, 64)]  # (Tp, S): 300, 300 and 384 frames


@pytest.mark.parametrize("linear", [False, True], ids=["nolin", "lin"])
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("Tp,S", SHAPES)
@pytest.mark.parametrize("n", [1, 3, 7, 16])
def test_gmm_any_count_per_frame_vs_float64(n, Tp, S, layout, linear):
    gmm_case(n, Tp, S, layout, linear, seed=7 * n + S + layout)


@pytest.mark.parametrize("linear", [False, True], ids=["nolin", "lin"])
@pytest.mark.parametrize("Tp,S,layout", [(100, 1, 1), (20, 5, 0), (2, 64, 0), (2, 64, 1)])
def test_gmm_ten_components_keep_their_bars(Tp, S, layout, linear):
    """num_mix = 10 through the same cases: the flat kernel at S = 1 and 5, the rows kernel at S = 64, as before the general arm."""
    gmm_case(10, Tp, S, layout, linear, seed=70 + S + layout)


def test_gmm_autograd_any_count_matches_abi():
    """ops.gmm_log_prob at n = 3 with a fused Linear: log_prob, d_dec, dW and db equal what the C ABI's d_par gives (dW = d_par^T dec,
    db = column sums) — the wrapper adds no arithmetic of its own beyond the head Linear's weight-gradient GEMM."""
    n, B, Tp, S, F = 3, 3, 20, 5, 9
    par, y = stress_frames(n, 4003)
    T_, x_sl, valid = layout_of(Tp, S)
    gen = torch.Generator().manual_seed(5)
    W = torch.eye(F) + torch.randint(-4, 5, (F, F), generator=gen).float() * (1 - torch.eye(F)) / 64
    bias = torch.randint(-256, 257, (F,), generator=gen).float() / 2**14
    idx = (torch.arange(B * Tp * S) * 11) % par.shape[0]
    dec = par[idx].view(B * Tp, S * F)
    yy = torch.where(valid[:, :T_], y[idx].view(B, Tp * S)[:, :T_], torch.full((B, T_), 5.0))
    g_b = torch.randn(B, generator=gen)
    ll, lp0, d_dec0, d_par0 = run_abi(n, dec, W, bias, yy, x_sl, g_b, 0, B, T_, Tp, S)
    dd = dec.to(DEV).requires_grad_(True)
    Wd, bd = W.to(DEV).requires_grad_(True), bias.to(DEV).requires_grad_(True)
    lp = ops.gmm_log_prob(dd, Wd, bd, yy.to(DEV), x_sl.to(DEV, torch.int32), 0, B, T_, Tp, S, n, BETA, SD_EPS)
    (lp * g_b.to(DEV).double()).sum().backward()
    assert torch.equal(lp.cpu(), lp0)
    assert torch.equal(dd.grad.cpu(), d_dec0.cpu())
    dp, de = d_par0.cpu().double().view(-1, F), dec.double().view(-1, F)
    torch.testing.assert_close(Wd.grad.cpu().double(), dp.t() @ de, rtol=1e-5, atol=1e-5 * float((dp.abs().t() @ de.abs()).max()))
    torch.testing.assert_close(bd.grad.cpu().double(), dp.sum(0), rtol=1e-5, atol=1e-5 * float(dp.abs().sum(0).max()))


@pytest.mark.parametrize("n", [0, 17])
def test_gmm_count_out_of_range_is_refused_before_any_launch(n):
    B, Tp, S, T_ = 2, 3, 4, 12
    F = 3 * max(n, 1)
    dec = torch.randn(B * Tp, S * F, device=DEV)
    y, xs = torch.zeros(B, T_, device=DEV), torch.full((B,), T_, device=DEV, dtype=torch.int32)
    gb = torch.ones(B, device=DEV)
    lp = torch.full((B,), SENTINEL, device=DEV, dtype=torch.float64)
    ll = torch.full((B, T_), SENTINEL, device=DEV)
    d_dec, d_par = torch.full_like(dec, SENTINEL), torch.full_like(dec, SENTINEL)
    W, b = torch.eye(F, device=DEV), torch.zeros(F, device=DEV)
    a = (p_(dec), 0, p_(W), p_(b), p_(y), p_(xs))
    for rc in (LIB.blvm_gmm_fwd(*a, B, T_, Tp, S, n, BETA, SD_EPS, p_(lp), p_(ll), _hip.stream_ptr()),
               LIB.blvm_gmm_bwd(*a, p_(gb), B, T_, Tp, S, n, BETA, SD_EPS, p_(d_dec), p_(d_par), _hip.stream_ptr())):  # fmt: skip
        assert rc != 0
        msg = LIB.blvm_last_error().decode()
        assert "num_mix" in msg and str(n) in msg, msg
    torch.cuda.synchronize()
    for name, t in (("log_prob", lp), ("ll_twise", ll), ("d_dec", d_dec), ("d_par", d_par)):
        assert bool((t == SENTINEL).all()), f"{name} written by a refused call"
    with pytest.raises(NotImplementedError, match=str(n)):
        ops.gmm_log_prob(dec, None, None, y, xs, 0, B, T_, Tp, S, n, BETA, SD_EPS)
    # the DMoL entry keeps refusing every count but ten
    rc = LIB.blvm_dmol_fwd(*a, B, T_, Tp, S, 3, 256, -7.0, p_(lp), p_(ll), _hip.stream_ptr())
    assert rc != 0 and "num_mix == 10" in LIB.blvm_last_error().decode()
    torch.cuda.synchronize()
    assert bool((lp == SENTINEL).all()) and bool((ll == SENTINEL).all())
