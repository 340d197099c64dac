"""The mixture samplers' test regimes, the rule a draw is judged by and its bars, shared by tests/test_draw_cases_cpu.py,
tests/test_oracle_golden.py and tests/test_gpu_samplers.py (and by oracle/gen_golden.py::gen_samplers, which builds the crafted rows
with `build` and records what the unmodified reference draws and returns on them into tests/golden/samplers.npz).

A regime is a set of packed head outputs par [N, 3K] (logits | locations | raw scales), Gumbel uniforms u [N, K], the component's
own noise v [N] (kind 0: uniform, the logistic's; kind 1: standard normal, stored as n) and the head's constants.  Truth is
blvm_oracle.mix_draw_detail: float64 on the float32 inputs cast up.

The rule (`judge`):
  * structural tie: best and runner-up have bit-equal (p_m, u_m); first maximum decides, and the draw is judged like any other;
  * undecided: otherwise, when the float64 gap between the best and the runner-up score is below
    16 u (2 + |p_a| + |G_a| + |p_b| + |G_b|), u = 2^-24, G the Gumbel term: the fp32 evaluation error of two scores (logf twice
    each, one rounding on each difference).  The sampler may return the value of either of the two components;
  * decided: |x - x64| <= 16 u (|loc| + sd (|log v| + |log(1 - v)|)) after the clamp; kind 1: 16 u (|mu| + sd |n|) + 4 u sd (the
    softplus).  The library is built without fast-math, so logf / expf are the accurate ones and this bar follows from the
    arithmetic: ~6 roundings on terms of those sizes;
  * v = None: the location itself, bit for bit (no arithmetic happens); u = None: the pick compares the fp32 logits themselves, so
    no draw is undecided;
  * where the float64 value before the clamp lies beyond +-(1 + bar), +-inf included, the output is EXACTLY +-1.0f.
Caps on the undecided share of a regime: CAP (0.5 %), and none at all in NO_UNDECIDED regimes."""
import os

import numpy as np
import torch

import blvm_oracle as O

U24 = 2.0**-24
FACTOR = 16.0
CAP = 0.005
NO_UNDECIDED = ("floor", "saturation", "ties")
K0 = 10
LOG_EPS = -7.0
FLOOR_RAWS = (-6.999, -7.0, -7.001, -7.5, -9.0, -30.0, -104.0)
SAT_LOCS = (0.999, 1.0, 1.0001, 1.5, 3.0)
END_U = (np.float32(1e-5), np.float32(1 - 1e-5), np.float32(1e-6), np.float32(1 - 1e-6))
END_V = (np.float32(1e-8), np.float32(1 - 1e-8), np.float32(0.5), np.nextafter(np.float32(0.5), np.float32(1)), np.float32(1 - 2.0**-24))
assert END_V[1] == np.float32(1.0)  # the upper end of the reference's uniform_(1e-8, 1 - 1e-8) in fp32: logit = +inf is a legal input
DMOL_REGIMES = ("floor", "saturation", "dominated", "ties", "ends", "trained")
GMM_REGIMES = ("gmm_sd0", "gmm_beta")
N_LEAD = 704  # rows of `dominated` whose leader is ahead by exactly 8; the rest are the sharp rows of dmol65536_par


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ----------------------------------------------------------------------------------------------------------------------
# the crafted rows (called by oracle/gen_golden.py::gen_samplers only; the tests read the fixture)
# ----------------------------------------------------------------------------------------------------------------------


def build(hs, seed=20261):
    """name -> dict(par [N,30] float32, and u [N,10] / v [N] where the regime crafts its own draws; a missing one means 'as the
    reference draws it').  hs: tests/golden/heads_stress.npz."""
    g = torch.Generator().manual_seed(seed)
    R = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)  # noqa: E731
    Nrm = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    pick = lambda vals, *s: torch.tensor(vals, dtype=torch.float64)[torch.randint(0, len(vals), s, generator=g)]  # noqa: E731
    K, out = K0, {}

    # floor: every component's raw scale from FLOOR_RAWS, |logit v| in [3, 15], locations small so that nothing clamps
    N = 256
    par = torch.cat([Nrm(N, K), R(N, K) * 0.6 - 0.3, pick(FLOOR_RAWS, N, K)], 1)
    lg = (3.0 + 12.0 * R(N)) * torch.where(R(N) < 0.5, -1.0, 1.0)
    out["floor"] = dict(par=par.float(), v=torch.sigmoid(lg).float())

    # saturation: locations at and beyond +-1, scales e^-3 .. e^0
    loc = pick(SAT_LOCS, N, K) * torch.where(R(N, K) < 0.5, -1.0, 1.0)
    out["saturation"] = dict(par=torch.cat([Nrm(N, K), loc, -3.0 * R(N, K)], 1).float())

    # dominated: one logit ahead of nine equal ones by 8 (it loses to Gumbel noise with probability 9 / (9 + e^8) = 0.3 %), and the
    # rows of dmol65536_par whose spread is 95 and more (logits 50 | 48 | -45 .. -105)
    lead = torch.zeros(N_LEAD, K, dtype=torch.float64) + torch.round(64.0 * Nrm(N_LEAD, 1)) / 16  # exact in fp32, so is the lead
    lead[torch.arange(N_LEAD), torch.randint(0, K, (N_LEAD,), generator=g)] += 8.0
    par = torch.cat([lead, R(N_LEAD, K) * 1.6 - 0.8, -7.5 + 5.5 * R(N_LEAD, K)], 1).float()
    out["dominated"] = dict(par=torch.cat([par, _t(hs["dmol65536_par"])[128:192]], 0))

    # ties: all logits equal | two maxima at (3, 7) | at (0, 9); the noisy draws are bit-equal on the tied components
    N = 192
    logits = Nrm(N, K) * 2
    top = logits.max(1).values + 0.5 + 6 * R(N)
    logits[0:64] = (4.0 * Nrm(64, 1)).expand(64, K)
    for rows, pair in ((slice(64, 128), (3, 7)), (slice(128, 192), (0, 9))):
        for m in pair:
            logits[rows, m] = top[rows]
    u = (1e-5 + (1 - 2e-5) * R(N, K)).float()
    u[0:64] = u[0:64, 2:3].clone()
    u[64:128, 7] = u[64:128, 3]
    u[128:192, 9] = u[128:192, 0]
    out["ties"] = dict(par=torch.cat([logits, R(N, K) * 1.8 - 0.9, -7.5 + 5.5 * R(N, K)], 1).float(), u=u)

    # ends: the ends of the reference's uniform ranges on trained and on saturated rows
    N = 240
    par = torch.cat([_t(hs["dmol65536_par"])[:120], out["saturation"]["par"][:120]], 0)
    u = torch.from_numpy(np.array(END_U, dtype=np.float32))[torch.randint(0, len(END_U), (N, K), generator=g)]
    v = torch.from_numpy(np.array(END_V, dtype=np.float32))[torch.arange(N) % len(END_V)]
    out["ends"] = dict(par=par, u=u, v=v)

    out["trained"] = dict(par=_t(hs["dmol65536_par"]).clone())
    # Gaussian mixture: raw IS the sd (the activation in float64, rounded to fp32) | raw is the pre-softplus value
    gp = _t(hs["gmm_par"]).clone()
    sd = O.softplus_beta64(gp[:, 2 * K:], float(hs["gmm_beta"])) + float(hs["gmm_sd_eps"])
    out["gmm_sd0"] = dict(par=torch.cat([gp[:, :2 * K], sd.float()], 1))
    out["gmm_beta"] = dict(par=gp)
    for name, r in out.items():  # standard normals for the kind-1 runs of the DMoL regimes (the GMM regimes record the reference's)
        if name not in GMM_REGIMES:
            r["n"] = Nrm(r["par"].shape[0]).float()
    return out


# ----------------------------------------------------------------------------------------------------------------------
# reading the fixture
# ----------------------------------------------------------------------------------------------------------------------


def load(golden_dir):
    """name -> regime dict(name, par, u, v, n) of float32 tensors; and the raw fixture."""
    fx = {k: v for k, v in np.load(os.path.join(golden_dir, "samplers.npz")).items()}
    regs = {}
    for name in DMOL_REGIMES + GMM_REGIMES:
        regs[name] = dict(name=name, par=_t(fx[f"{name}_par"]), u=_t(fx[f"{name}_u"]), v=_t(fx[f"{name}_v"]) if f"{name}_v" in fx else None,
                          n=_t(fx[f"{name}_n"]))
    return regs, fx


def head_constants(name, kind, fx):
    """(log_eps, sd_beta, sd_eps) a regime runs under.  kind 1 on a DMoL regime: its raw column goes through the softplus."""
    if kind == 0:
        return LOG_EPS, 0.0, 0.0
    if name == "gmm_sd0":
        return LOG_EPS, 0.0, 0.0
    return LOG_EPS, float(fx["gmm_beta"]), float(fx["gmm_sd_eps"])


def noise(reg, kind):
    return reg["v"] if kind == 0 else reg["n"]


def with_K(reg, K):
    """The regime at another component count: K <= 10 keeps the first K components of each group; K = 32 joins the components of rows
    i, i+1, i+2 and the first two of row i+3 (cyclically), so every row keeps distinct components."""
    if K == K0:
        return reg
    par, u = reg["par"], reg["u"]
    groups = [par[:, j * K0:(j + 1) * K0] for j in range(3)] + [u]
    if K < K0:
        groups = [gr[:, :K] for gr in groups]
    else:
        groups = [torch.cat([gr.roll(-j, 0) for j in range((K + K0 - 1) // K0)], 1)[:, :K] for gr in groups]
    return dict(reg, name=f"{reg['name']}/K{K}", par=torch.cat(groups[:3], 1).contiguous(), u=groups[3].contiguous())


def take(reg, idx):
    """Rows idx of a regime."""
    return dict(reg, **{k: reg[k][idx].contiguous() for k in ("par", "u", "v", "n") if reg[k] is not None})


# ----------------------------------------------------------------------------------------------------------------------
# the rule
# ----------------------------------------------------------------------------------------------------------------------


def classify(par, u, v, kind, log_eps=LOG_EPS, sd_beta=0.0, sd_eps=0.0):
    """The float64 truth of every draw with the rule's quantities: dict of mix_draw_detail plus structural, undecided [N] bool and
    bar, bar_runner [N] (bars of the value under the picked component / the runner-up)."""
    d = O.mix_draw_detail(par, u, v, kind, log_eps, sd_beta, sd_eps)
    N, K = par.shape[0], par.shape[1] // 3
    rows = torch.arange(N)
    if u is None:
        same_u = torch.ones(N, dtype=torch.bool)
    else:
        uu = u.reshape(N, K)
        same_u = uu[rows, d["best"]] == uu[rows, d["runner"]]
    same_p = par[rows, d["best"]] == par[rows, d["runner"]]
    d["structural"] = same_u & same_p & (d["best"] != d["runner"])
    tol = FACTOR * U24 * (2 + d["p_best"].abs() + d["g_best"].abs() + d["p_runner"].abs() + d["g_runner"].abs())
    d["undecided"] = (d["s_best"] - d["s_runner"] < tol) & ~d["structural"] & (d["best"] != d["runner"])
    if u is None:  # the mode compares the fp32 logits themselves: nothing is evaluated, nothing is undecided
        d["undecided"] = torch.zeros(N, dtype=torch.bool)

    def bar_of(c):
        loc = par[rows, K + c].double().abs()
        raw = par[rows, 2 * K + c].double()
        if v is None:
            return torch.zeros(N, dtype=torch.float64)
        vv = v.double().reshape(N)
        if kind == 0:
            return FACTOR * U24 * (loc + torch.exp(raw.clamp(min=log_eps)) * (torch.log(vv).abs() + torch.log(1 - vv).abs()))
        sd = (O.softplus_beta64(raw, sd_beta) + sd_eps if sd_beta > 0 else raw).abs()
        return FACTOR * U24 * (loc + sd * vv.abs()) + 4 * U24 * sd

    d["bar"], d["bar_runner"] = bar_of(d["best"]), bar_of(d["runner"])
    return d


def _ratio(got, x, pre, bar):
    """err / bar per draw; where the value before the clamp lies beyond +-(1 + bar) the output must be exactly +-1 (ratio 0 or inf)."""
    err = (got - x).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bar)  # 0 / 0 (v None, exact) counts as met
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    return ratio


def judge(name, got, par, u, v, kind, log_eps=LOG_EPS, sd_beta=0.0, sd_eps=0.0, cap=None, where=None):
    """Hold `got` [N] (float32 samples) to the rule.  Returns dict(n, undecided, share, worst, clamped, detail); raises AssertionError
    naming the worst draw (`where(i)` turns its row into the caller's index) when a draw misses its bar or the regime its cap."""
    got = got.detach().cpu().reshape(-1)
    d = classify(par, u, v, kind, log_eps, sd_beta, sd_eps)
    g64 = got.double()
    clamped = kind == 0 and v is not None
    if clamped:
        exact_hi, exact_lo = d["pre"] > 1 + d["bar"], d["pre"] < -1 - d["bar"]
        exact_hi, exact_lo = exact_hi | (d["pre"] == float("inf")), exact_lo | (d["pre"] == -float("inf"))
    ratio = _ratio(g64, d["x"], d["pre"], d["bar"])
    if clamped:
        one = torch.ones_like(g64)
        ratio = torch.where(exact_hi, torch.where(g64 == one, 0 * one, one * float("inf")), ratio)
        ratio = torch.where(exact_lo, torch.where(g64 == -one, 0 * one, one * float("inf")), ratio)
        assert bool(((g64 >= -1) & (g64 <= 1)).all()), f"{name}: a sample outside [-1, 1] (or not finite)"
    alt = _ratio(g64, d["x_runner"], d["pre_runner"], d["bar_runner"])
    ratio = torch.where(d["undecided"], torch.minimum(ratio, alt), ratio)
    n, und = got.numel(), int(d["undecided"].sum())
    cap = (0.0 if name.split("/")[0] in NO_UNDECIDED else CAP) if cap is None else cap
    i = int(ratio.argmax())
    res = dict(n=n, undecided=und, share=und / n, worst=float(ratio[i]), worst_at=i, detail=d,
               clamped=int(((d["pre"].abs() >= 1)).sum()) if clamped else 0)
    at = where(i) if where is not None else i
    assert res["worst"] <= 1.0, (
        f"{name}: draw {at}: got {float(got[i]):.9g}, float64 {float(d['x'][i]):.9g} (before the clamp {float(d['pre'][i]):.9g}; component "
        f"{int(d['best'][i])}, runner-up {int(d['runner'][i])} would give {float(d['x_runner'][i]):.9g}; score gap {float(d['s_best'][i] - d['s_runner'][i]):.3e}, "
        f"undecided {bool(d['undecided'][i])}); bar {float(d['bar'][i]):.3e}, err/bar {res['worst']:.3g}")
    assert und <= cap * n, f"{name}: {und} of {n} draws undecided, cap {cap * n:.2f}"
    return res


def report(name, res):
    print(f"[samplers] {name}: draws {res['n']}, undecided {res['undecided']} ({100 * res['share']:.3f} %), worst err/bar {res['worst']:.3f}")


def oracle32(par, u, v, kind, log_eps=LOG_EPS, sd_beta=0.0, sd_eps=0.0):
    """The oracle's formulas evaluated in float32 with torch on the CPU (what the float64 bar is compared with when a regime's
    bar is in question; never the kernel under test)."""
    K = par.shape[1] // 3
    logits, locs, raws = par[:, :K], par[:, K:2 * K], par[:, 2 * K:]
    s = logits if u is None else logits - torch.log(-torch.log(u))
    idx = s.argmax(-1, keepdim=True)
    loc, raw = locs.gather(1, idx).squeeze(1), raws.gather(1, idx).squeeze(1)
    if v is None:
        return loc
    if kind == 0:
        return (loc + torch.exp(raw.clamp(min=log_eps)) * (torch.log(v) - torch.log(1 - v))).clamp(-1, 1)
    sd = torch.nn.functional.softplus(raw, beta=sd_beta) + sd_eps if sd_beta > 0 else raw
    return loc + sd * v



# ----------------------------------------------------------------------------------------------------------------------
# the cases the direct tests of blvm_mix_sample run (tests/test_draw_cases_cpu.py asserts the caps for exactly these)
# ----------------------------------------------------------------------------------------------------------------------

K_GENERIC = (1, 3, 5, 32)  # the kernel's any-count arm; K0 = 10 is the unrolled one


def direct_cases(regs, fx):
    """[(id, regime at its K, kind, (log_eps, sd_beta, sd_eps))]: every DMoL regime as kind 0 at every K and as kind 1 (raw through
    the softplus) at K = 10; both Gaussian-mixture regimes at K = 10, 3 and 32."""
    out = []
    for name in DMOL_REGIMES:
        for K in (K0,) + K_GENERIC:
            out.append((f"{name}-kind0-K{K}", with_K(regs[name], K), 0, head_constants(name, 0, fx)))
        out.append((f"{name}-kind1-K{K0}", regs[name], 1, head_constants(name, 1, fx)))
    for name in GMM_REGIMES:
        for K in (K0, 3, 32):
            out.append((f"{name}-kind1-K{K}", with_K(regs[name], K), 1, head_constants(name, 1, fx)))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the in-kernel draw sites: parameter rows a network can be made to emit, and the draws of one launch
# ----------------------------------------------------------------------------------------------------------------------

# The layer in front of the head gets zero weight and a bias a >= 0 (ReLU / LeakyReLU pass it exactly), the head Linear the signed
# diagonal below and zero bias, so position s of the frame stack draws from row s = a[s] * SIGNS whatever was fed back: logits
# >= 0, locations of either sign by component, raw scales <= 0.
SIGNS = torch.cat([torch.ones(K0), torch.tensor([1.0, -1.0] * (K0 // 2)), -torch.ones(K0)])
_BLOCK = {"ties": 64}  # rows whose draws may be exchanged: the tied components sit at the same places within a block
# (entry point, S, B, T) of tests/test_gpu_samplers.py, section b
SITE_SHAPES = (("vrnn_decode", 16, 17, 3), ("vrnn_generate", 8, 5, 3), ("vrnn_generate", 16, 5, 3), ("srnn_generate", 8, 5, 3),
               ("srnn_generate", 16, 5, 3), ("lstm_generate", 1, 5, 3), ("lstm_generate", 24, 5, 3), ("stcn_generate", 8, 3, 3),
               ("wavenet_decode", 1, 19, 24))
# S = 1 (the LSTM at stack 1, WaveNet): one launch per (regime, fixture row)
SINGLE_ROWS = (("floor", 5), ("saturation", 9), ("dominated", 17), ("ties", 70), ("trained", 3), ("trained", 140))


def site_case(reg, S, B, T, first=None):
    """One launch of a draw site on S rows of a DMoL regime: dict(a [S,30] >= 0 (the bias), rows [S,30] = a * SIGNS (the head
    parameters), and the flat regime of its T*B*S draws in the order [t, b, s]: par, u [T*B*S,10], v [T*B*S]).  Row s comes from
    fixture row r_s (spread over the regime, or `first` for S = 1); the draws of (t, b, s) are those of another fixture row of the
    same block, a different one for every (t, b)."""
    name, N = reg["name"], reg["par"].shape[0]
    r = torch.tensor([first]) if first is not None else (torch.arange(S) * (N // S) + (N // S) // 2) % N
    src = reg["par"][r]
    logits = src[:, :K0] - src[:, :K0].min()
    a = torch.cat([logits, src[:, K0:].abs()], 1)
    rows = a * SIGNS
    block = _BLOCK.get(name, N)
    t, b, s = torch.meshgrid(torch.arange(T), torch.arange(B), torch.arange(S), indexing="ij")
    q = (r[s] // block) * block + (r[s] + 7 * (t * B + b) + 3 * s + 1) % block
    q = torch.where(q < N, q, r[s]).reshape(-1)
    flat = dict(name=f"{name}/site", par=rows[s.reshape(-1)].contiguous(), u=reg["u"][q].contiguous(), v=reg["v"][q].contiguous(), n=None)
    return dict(a=a, rows=rows, flat=flat, S=S, B=B, T=T)


def site_index(case, i):
    S, B = case["S"], case["B"]
    return f"(t, b, s) = ({i // (B * S)}, {(i // S) % B}, {i % S})"
