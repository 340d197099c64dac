"""Cases and float64 truth for WaveNet with embedded class input (K10e: `blvm_wavenet_embed_*`, `WaveNet(embedding_dim=E)`): the front
(embedding -> zero left padding -> causal conv with groups = C) restated with torch, its gradients by autograd, the per-element error
bounds, the shapes, and the restatement of window generation the GPU tests compare every class with.
TEST INFRASTRUCTURE: not imported by the product.

Front.  `front_torch` is `causal(pad(embedding(k)))` by `F.embedding` and `F.conv1d(groups=C)`: index -1 is a frame of zeros (the
reference pads AFTER embedding, wavenet.py:182-188).  `front_tables` is the table form the kernels implement,
out[t,b,o] = P_0[k[t,b]][o] + P_1[k[t+1,b]][o] + bias[o] with P_tap[k][o] = sum_j cw[o,j,tap] E[k, o m + j].

Bounds (derived, not measured; u = 2^-24, fp32 round to nearest):
  forward   an output is 2m products, 2m - 2 additions inside the tables, 2 additions outside: at most 2m + 2 roundings on a sum of
            2m + 1 terms, so |err| <= (2m + 2) u sum|terms| to first order, whatever the order.
  backward  a gradient element is a sum of n products, each of one rounding, added in some order in at most n - 1 additions of partial
            sums of the same terms: |err| <= n u sum|terms| for ANY summation order.  n per element: dE[k, e]: the frames of class k in
            either tap + 2 (the two weight products); dcw: every output frame + V (the second stage adds per-class products); db: every
            output frame.  sum|terms| comes from the same autograd with absolute values of the factors.

Generation.  `generate_embed` is `wavenet_cat_cases.generate_cat` with a window of CLASSES and the embedding in front: the zero start
is a window of class 0 (`embedding(zeros)`, wavenet.py:264-266), the drawn class is fed back as a class.  Models are in the trained-like
regime of `wavenet_cat_cases.build_model`.  Tie rule: that file's.  MAX_CDF_ERR32 is the largest |cdf32 - cdf64| of the float32 run of
the same restatement over all cases (re-measured by tests/test_wavenet_embed_cpu.py), MIN_GAP = 16 x that; the draws' seeds are chosen
so that every case has gap >= MIN_GAP, so the GPU tests compare EVERY class."""
import functools
import math

import torch
import torch.nn.functional as F

import blvm_oracle as O
import wavenet_cat_cases as WC

U32 = 2.0**-24

# ---- the front -------------------------------------------------------------------------------------------------------------------------

#               V      C   m  L_in B      (L_in counts the leading padding; both pad_causal settings run on each)
FRONT_SHAPES = [(32, 16, 1, 9, 3), (48, 48, 2, 70, 5), (256, 64, 1, 70, 19), (65536, 32, 1, 40, 4)]
# backward only: L * B = 40 000 frames, 90 % of them in one class (silence)
SKEWED = (256, 64, 1, 2000, 20)


def front_case(V, C, m, L, B, seed=0, skew=None):
    """-> dict(k [L,B] int64 (three leading rows of -1, classes 0 and V - 1 present), emb [V,E], cw [C,m,2], bias [C], d_out for both
    pad_causal settings) in float32.  skew: the share of frames in class V // 3."""
    g = torch.Generator().manual_seed(1000 * seed + V + C + L)
    k = torch.randint(0, V, (L, B), generator=g)
    if skew is not None:
        k = torch.where(torch.rand(L, B, generator=g) < skew, torch.full_like(k, V // 3), k)
    k[:3] = -1
    k[3, 0], k[4, 0], k[L - 1, B - 1], k[L - 2, B - 1] = 0, V - 1, 0, V - 1
    E = C * m
    emb = torch.randn(V, E, generator=g)
    cw = (torch.rand(C, m, 2, generator=g) * 2 - 1) / math.sqrt(2 * m)
    bias = (torch.rand(C, generator=g) * 2 - 1) / math.sqrt(2 * m)
    d_out = {pc: torch.randn(L - 1 - int(pc), B, C, generator=g) for pc in (False, True)}
    return dict(k=k, emb=emb, cw=cw, bias=bias, d_out=d_out, V=V, C=C, m=m, L=L, B=B)


def front_torch(k, emb, cw, bias, pad_causal):
    """causal(pad(embedding(k))) with torch: k [L,B] (-1: a zero frame) -> [L - 1 - pad_causal, B, C], in the dtype of emb."""
    e = F.embedding(k.clamp(min=0), emb) * (k >= 0).unsqueeze(-1).to(emb.dtype)  # [L,B,E]
    h = e.permute(1, 2, 0)  # [B,E,L]
    if pad_causal:
        h = h[..., :-1]
    return F.conv1d(h, cw, bias, groups=cw.shape[0]).permute(2, 0, 1)


def tables(emb, cw):
    """P [2,V+1,C]: P[tap][k][o] = sum_j cw[o,j,tap] emb[k, o m + j]; row V zeros."""
    V = emb.shape[0]
    C, m = cw.shape[0], cw.shape[1]
    P = torch.einsum("kcj,cjt->tkc", emb.view(V, C, m), cw)
    return torch.cat([P, P.new_zeros(2, 1, C)], 1)


def front_tables(k, emb, cw, bias, pad_causal):
    V = emb.shape[0]
    P = tables(emb, cw)
    kk = torch.where(k < 0, torch.full_like(k, V), k)
    Lo = k.shape[0] - 1 - int(pad_causal)
    return P[0][kk[:Lo]] + P[1][kk[1 : Lo + 1]] + bias


@functools.lru_cache(maxsize=None)
def front_reference(shape, pad_causal, skew=None):
    """(case, out64, bound [Lo,B,C]) — computed once, never changed."""
    c = front_case(*shape, skew=skew)
    d = lambda t: t.double()  # noqa: E731
    out = front_torch(c["k"], d(c["emb"]), d(c["cw"]), d(c["bias"]), pad_causal)
    terms = front_torch(c["k"], d(c["emb"]).abs(), d(c["cw"]).abs(), d(c["bias"]).abs(), pad_causal)
    return c, out, (2 * c["m"] + 2) * U32 * terms


def _grads(k, emb, cw, bias, d_out, pad_causal):
    emb, cw, bias = (t.clone().requires_grad_(True) for t in (emb, cw, bias))
    (front_torch(k, emb, cw, bias, pad_causal) * d_out).sum().backward()
    return emb.grad, cw.grad, bias.grad


@functools.lru_cache(maxsize=None)
def grad_reference(shape, pad_causal, skew=None):
    """(case, (dE, dcw, db) in float64 by autograd, their bounds n u sum|terms|, the classes without a frame) — computed once."""
    c = front_case(*shape, skew=skew)
    d = lambda t: t.double()  # noqa: E731
    k, emb, cw, bias, g = c["k"], d(c["emb"]), d(c["cw"]), d(c["bias"]), d(c["d_out"][pad_causal])
    grads = _grads(k, emb, cw, bias, g, pad_causal)
    dE_abs = _grads(k, emb, cw.abs(), bias, g.abs(), pad_causal)[0]
    dcw_abs = _grads(k, emb.abs(), cw, bias, g.abs(), pad_causal)[1]
    Lo, V = g.shape[0], c["V"]
    kk = torch.where(k < 0, torch.full_like(k, V), k)
    counts = torch.bincount(kk[:Lo].reshape(-1), minlength=V + 1)[:V] + torch.bincount(kk[1 : Lo + 1].reshape(-1), minlength=V + 1)[:V]
    frames = Lo * c["B"]
    bounds = ((counts + 2).unsqueeze(-1) * U32 * dE_abs, (frames + V) * U32 * dcw_abs, frames * U32 * g.abs().sum((0, 1)))
    return c, grads, bounds, counts == 0


# ---- generation ------------------------------------------------------------------------------------------------------------------------

# measured by test_min_gap_is_derived_from_the_float32_run: the largest |cdf32 - cdf64| over all cases and prompts is 1.32e-7; recorded
# rounded up, with room for another host's float32 exp and cumsum (the value wavenet_cat_cases records)
MAX_CDF_ERR32 = 2.5e-7
MIN_GAP = 16 * MAX_CDF_ERR32  # 4e-6


class Case(WC.Case):
    def __init__(self, name, B, C, E, layers, stacks, V, n_frames, seed):
        super().__init__(name, B, C, layers, stacks, V, n_frames, seed)
        self.E = E


#                        B   C   E  layers stacks V  n_frames seed    rf    kernel arm
SHAPES = {
    "e16": Case("e16", 3, 16, 16, 4, 2, 32, 24, 8),  # 32   any-width kernel; every ring (d <= 8) wraps
    "e64m2": Case("e64m2", 19, 32, 64, 5, 2, 256, 20, 51),  # 64   <8,32,32>; two embedding columns per channel; a partial 16-row group
    "e64": Case("e64", 2, 64, 64, 6, 2, 1024, 40, 65),  # 128  <8,64,64>
}
# (shape, prompt length); P = 0: the zero start (a past of class 0).  e16: P < rf class-0 pad, P == rf, P > rf trimming; the others one P
# that is no multiple of the larger dilations
STARTS = [("e16", 0), ("e16", 11), ("e16", 32), ("e16", 40), ("e64m2", 0), ("e64m2", 70), ("e64", 0), ("e64", 77)]
# the draws' seed is the case's seed plus this (default 0): the first offset at which the case's gap is >= 1e-5
DRAW_OFFSETS = {("e64m2", 0): 2, ("e64m2", 70): 2, ("e64", 0): 6, ("e64", 77): 5}


def build_model(case):
    """The case's network in the trained-like regime of `wavenet_cat_cases.build_model` (CPU, fp32)."""
    from blvm.models import WaveNet
    from blvm.modules.distributions import CategoricalDense

    torch.manual_seed(case.seed)
    m = WaveNet(likelihood=CategoricalDense(case.C, case.V), embedding_dim=case.E, num_bins=case.V, n_layers=case.layers,
                n_stacks=case.stacks, res_channels=case.C)  # fmt: skip
    assert m.receptive_field == case.rf and list(m.res_stack.dilations) == list(case.dilations)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith("weight") and k.startswith("res_stack.res_blocks"):
                p.mul_(2.0)
            elif k in ("out_transform.linear.weight", "likelihood.logits.weight"):
                p.mul_(3.0)
    return m


def draws(case, P, n_frames=None, offset=0):
    """-> prompt classes [B,P] int64 and n_frames draws u [B] uniform in [0, 1)."""
    g = torch.Generator().manual_seed(case.seed + offset)
    n = case.n_frames if n_frames is None else n_frames
    prompt = torch.randint(0, case.V, (case.B, max(P, 1)), generator=g)
    uni = [torch.rand(case.B, generator=g) for _ in range(n)]
    return prompt[:, :P], uni


def window_of(prompt, rf):
    """The last rf classes of prompt [B,P], class 0 in front of a shorter one -> [B,rf]."""
    w = prompt[:, -rf:]
    return F.pad(w, (rf - w.size(1), 0))


def generate_embed(sd, window, n_frames, n_layers, n_stacks, uniforms, V, base_dilation=2):
    """`wavenet_cat_cases.generate_cat` on a window of classes [B,rf] with the embedding in front, in the dtype of `sd`.
    -> dict(k [B,n] int64, cdf [n,B,V] normalised, gap, mode_share)."""
    dil = O.wavenet_dilations(n_layers, n_stacks, base_dilation)
    cw, emb = sd["causal.conv.weight"], sd["embedding.weight"]
    rf = sum(dil) + 1 + (cw.size(2) - 1)
    assert tuple(window.shape[1:]) == (rf,)
    x = F.embedding(window, emb).transpose(1, 2)  # [B,E,rf]
    scale = math.sqrt(n_layers / n_stacks)
    ks, cdfs, gap, at_mode = [], [], float("inf"), 0
    for t in range(n_frames):
        h = F.conv1d(x, cw, sd["causal.conv.bias"], groups=cw.size(0))
        skips = sum(O.residual_stack_skips(sd, "res_stack", h, dil, 1)) / scale  # [B,C,1]
        o = F.relu(F.linear(F.relu(skips.transpose(1, 2)), sd["out_transform.linear.weight"], sd["out_transform.linear.bias"]))
        l = F.linear(o, sd["likelihood.logits.weight"], sd["likelihood.logits.bias"])[:, 0]  # [B,V]
        top = l.max(-1, keepdim=True).values
        c = (l - top).exp().cumsum(-1)
        cdf = c / c[:, -1:]
        u = uniforms[t].to(cw.dtype)
        hit = c >= (u * c[:, -1]).unsqueeze(-1)
        k = torch.where(hit.any(-1), hit.int().argmax(-1), torch.tensor(V - 1))
        below = torch.where(k > 0, cdf.gather(-1, (k - 1).clamp(min=0).unsqueeze(-1)).squeeze(-1), torch.zeros_like(u))
        above = torch.where(k < V - 1, cdf.gather(-1, k.unsqueeze(-1)).squeeze(-1) - u, torch.full_like(u, float("inf")))
        gap = min(gap, float(torch.minimum(u - below, above).min()))
        at_mode += int((k == l.argmax(-1)).sum())
        ks.append(k)
        cdfs.append(cdf)
        x = torch.cat([x[:, :, 1:], F.embedding(k, emb).unsqueeze(-1)], dim=2)
    k = torch.stack(ks, 1)
    return dict(k=k, cdf=torch.stack(cdfs), gap=gap, mode_share=at_mode / k.numel())


def _run(name, P, dtype):
    case = SHAPES[name]
    m = build_model(case)
    prompt, uni = draws(case, P, offset=DRAW_OFFSETS.get((name, P), 0))
    sd = {k: v.detach().to(dtype) for k, v in m.state_dict().items()}
    return m, prompt, uni, generate_embed(sd, window_of(prompt, case.rf), case.n_frames, case.layers, case.stacks, uni, case.V)


@functools.lru_cache(maxsize=None)
def reference(name, P):
    """(model on the CPU, prompt classes, draws, float64 result of `generate_embed`) of a case — computed once, never changed."""
    return _run(name, P, torch.float64)


@functools.lru_cache(maxsize=None)
def reference32(name, P):
    """The same restatement in float32 (for MIN_GAP only)."""
    return _run(name, P, torch.float32)[3]


# ---- the model against the golden -------------------------------------------------------------------------------------------------------

FIXTURES = {"cat16": ("cat", 16, True), "cat32": ("cat", 32, True), "cat16n": ("cat", 16, False), "dmol16": ("dmol", 16, True)}


def fixture_model(g, tag):
    """This project's model of a fixture of tests/golden/wavenet_embed.npz with the reference's state_dict loaded (CPU)."""
    from blvm.models import WaveNet
    from blvm.modules.distributions import CategoricalDense, DiscretizedLogisticMixtureDense

    head, E, _ = FIXTURES[tag]
    lik = CategoricalDense(16, 32) if head == "cat" else DiscretizedLogisticMixtureDense(16, 1, num_mix=10, num_bins=256)
    m = WaveNet(likelihood=lik, embedding_dim=E, num_bins=32, n_layers=2, n_stacks=2, res_channels=16, kernel_size=2, base_dilation=2)
    m.load_state_dict({k[len(tag) + 4 :]: torch.from_numpy(g[k]) for k in g.files if k.startswith(f"{tag}.sd.")})
    return m


def fixture_ll(g, tag, dtype=torch.float64):
    """The restatement of a categorical fixture's ll [B,T'] in `dtype`: `front_torch`, the oracle's residual stack, log-softmax at y."""
    head, _, pad_rf = FIXTURES[tag]
    assert head == "cat"
    sd = {k[len(tag) + 4 :]: torch.from_numpy(g[k]).to(dtype) for k in g.files if k.startswith(f"{tag}.sd.")}
    k, x_sl, rf = torch.from_numpy(g[f"{tag}.x"]), torch.from_numpy(g[f"{tag}.x_sl"]), int(g[f"{tag}.rf"])
    B, T = k.shape
    kt = k.t()
    if pad_rf:
        kt, skip, sl = torch.cat([torch.full((rf, B), -1), kt]), T, x_sl
    else:
        skip, sl = T - rf, x_sl - rf
    h = front_torch(kt, sd["embedding.weight"], sd["causal.conv.weight"], sd["causal.conv.bias"], True).permute(1, 2, 0)  # [B,C,L]
    out = sum(O.residual_stack_skips(sd, "res_stack", h, O.wavenet_dilations(2, 2), skip)) * math.sqrt(2 / 2)
    o = F.relu(F.linear(F.relu(out.transpose(1, 2)), sd["out_transform.linear.weight"], sd["out_transform.linear.bias"]))
    logp = F.linear(o, sd["likelihood.logits.weight"], sd["likelihood.logits.bias"]).log_softmax(-1)
    y = torch.from_numpy(g[f"{tag}.y"]).long()
    mask = torch.arange(skip).unsqueeze(0) < sl.unsqueeze(1)
    return logp.gather(-1, y.unsqueeze(-1)).squeeze(-1) * mask
