"""Cases and float64 truth for one-launch WaveNet generation with the categorical head (`blvm_wavenet_cat_decode`, K10c): the
shapes, the trained-like models, the draws, and the restatement of window generation the GPU tests compare every class with.
TEST INFRASTRUCTURE: not imported by the product.

Restatement (`generate_cat`): the loop of `blvm_oracle.wavenet_generate` with the initial window as an argument and the categorical
head in place of the DMoL head, in the dtype of the state_dict: logits l = head Linear; e = exp(l - max l); class = the first k whose
prefix sum of e is >= u * S (S the total; V - 1 if none is); the class is fed back as the fp32 `linspace(-1, 1, V)[k]`.

Regime: as tests/test_wavenet_prompt.py — the residual blocks' weights x 2, the output transform's and the head's x 3 (a trained-like
network: the prompt changes the classes drawn and the softmax is not one-hot; `test_cases_have_no_near_ties` asserts that fewer than
half the draws are the arg-max class and that at least 8 distinct classes occur in every case).

Comparison rule: a draw next to a CDF boundary would flip the class and every later sample, so ties are excluded by construction.
Every case records `gap`, the float64 minimum over rows and frames of min(u - cdf[k-1], cdf[k] - u) on the normalised CDF (cdf[-1] = 0;
the cdf[k] side is skipped where k = V - 1, the catch-all class).  MIN_GAP is derived on the CPU from the float32 run of the same
restatement with the same draws: it draws the same classes, and the largest |cdf32 - cdf64| it sees over all cases is MAX_CDF_ERR32;
MIN_GAP = 16 * MAX_CDF_ERR32, the factor covering the other summation orders of the MFMA tiles and of the kernel's prefix sum.
`test_min_gap_is_derived_from_the_float32_run` re-measures the first number and holds the recorded one against it; the seeds are chosen
so that every case has gap >= MIN_GAP (`test_cases_have_no_near_ties`).  With that the GPU tests compare EVERY class."""
import functools
import math

import torch
import torch.nn.functional as F

import blvm_oracle as O

# measured by test_min_gap_is_derived_from_the_float32_run: the largest |cdf32 - cdf64| over all cases and prompts is 1.52e-7 (a little over one
# fp32 ulp of a CDF value next to 1); recorded rounded up, with room for another host's float32 exp and cumsum
MAX_CDF_ERR32 = 2.5e-7
MIN_GAP = 16 * MAX_CDF_ERR32  # 4e-6
MIN_LOGIT_GAP = 1e-3  # the mode tests: the smallest gap between the two largest logits over all rows and frames


class Case:
    def __init__(self, name, B, C, layers, stacks, V, n_frames, seed):
        self.name, self.B, self.C, self.layers, self.stacks = name, B, C, layers, stacks
        self.V, self.n_frames, self.seed = V, n_frames, seed
        self.dilations = O.wavenet_dilations(layers, stacks, 2)
        self.rf = sum(self.dilations) + 2


#                         B   C  layers stacks V  n_frames seed     rf    kernel arm
SHAPES = {
    "c16v32": Case("c16v32", 3, 16, 4, 2, 32, 24, 8),  # 32   any-width kernel; every ring (d <= 8) wraps
    "c32v256": Case("c32v256", 19, 32, 5, 2, 256, 20, 51),  # 64   <8,32,32>; a partial 16-row group (16 + 3)
    "c64v1024": Case("c64v1024", 2, 64, 6, 2, 1024, 40, 65),  # 128  <8,64,64>; the largest logits buffer; the 32-deep rings wrap
    "c128v16": Case("c128v16", 40, 128, 3, 1, 16, 12, 168),  # 9   odd block count; three workgroups, the last partial; widest C; smallest V
    "v2048": Case("v2048", 3, 16, 4, 2, 2048, 10, 8),  # 32    V > 1024: block by block
}
KERNEL_CASES = ["c16v32", "c32v256", "c64v1024", "c128v16"]
# (shape, prompt length); P = 0: the zero start.  c16v32: P < rf zero pad, P == rf exact window, P > rf trimming; the others one P that is
# no multiple of the larger dilations
STARTS = [("c16v32", 0), ("c16v32", 11), ("c16v32", 32), ("c16v32", 40), ("c32v256", 0), ("c32v256", 70), ("c64v1024", 0), ("c64v1024", 77),
          ("c128v16", 0), ("c128v16", 9)]  # fmt: skip
# the draws' seed is the case's seed plus this (default 0): the first offset at which the case's gap is >= 1e-5
DRAW_OFFSETS = {("c16v32", 40): 1, ("c32v256", 0): 1, ("c64v1024", 0): 19, ("c64v1024", 77): 4, ("v2048", 0): 1}


def build_model(case):
    """The case's network in the trained-like regime (CPU, fp32)."""
    from blvm.models import WaveNet
    from blvm.modules.distributions import CategoricalDense

    torch.manual_seed(case.seed)
    m = WaveNet(likelihood=CategoricalDense(case.C, case.V), n_layers=case.layers, n_stacks=case.stacks, res_channels=case.C)
    assert m.receptive_field == case.rf and list(m.res_stack.dilations) == list(case.dilations)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith("weight") and k.startswith("res_stack.res_blocks"):
                p.mul_(2.0)
            elif k in ("out_transform.linear.weight", "likelihood.logits.weight"):
                p.mul_(3.0)
    return m


def draws(case, P, n_frames=None, offset=0):
    """-> prompt [B,P,1] uniform in [-0.8, 0.8] and n_frames draws u [B] uniform in [0, 1)."""
    g = torch.Generator().manual_seed(case.seed + offset)
    n = case.n_frames if n_frames is None else n_frames
    prompt = torch.rand(case.B, max(P, 1), 1, generator=g) * 1.6 - 0.8
    uni = [torch.rand(case.B, generator=g) for _ in range(n)]
    return prompt[:, :P], uni


def window_of(prompt, rf):
    """The last rf samples of prompt [B,P,1], zeros in front of a shorter one -> [B,rf,1]."""
    w = prompt[:, -rf:]
    return F.pad(w, (0, 0, rf - w.size(1), 0))


def generate_cat(sd, window, n_frames, n_layers, n_stacks, uniforms, V, base_dilation=2):
    """Window generation with the categorical head from a given window [B,rf,1], in the dtype of `sd`.  uniforms[t] [B], or None: the
    arg-max class (first maximum) is fed back.  -> dict(k [B,n] int64, x [B,n,1], cdf [n,B,V] normalised, gap, logit_gap, mode_share:
    the share of draws that took the arg-max class)."""
    dil = O.wavenet_dilations(n_layers, n_stacks, base_dilation)
    rf = sum(dil) + 1 + (sd["causal.conv.weight"].size(2) - 1)
    dt = sd["causal.conv.weight"].dtype
    assert tuple(window.shape[1:]) == (rf, 1)
    levels = torch.linspace(-1.0, 1.0, V).to(dt)  # the fp32 table of `CategoricalDense.levels` / `Quantize`
    x = window.to(dt).transpose(1, 2)  # [B,1,rf]
    scale = math.sqrt(n_layers / n_stacks)
    ks, cdfs, gap, logit_gap, at_mode = [], [], float("inf"), float("inf"), 0
    for t in range(n_frames):
        h = F.conv1d(x, sd["causal.conv.weight"], sd["causal.conv.bias"])
        skips = sum(O.residual_stack_skips(sd, "res_stack", h, dil, 1)) / scale  # [B,C,1]
        o = F.relu(F.linear(F.relu(skips.transpose(1, 2)), sd["out_transform.linear.weight"], sd["out_transform.linear.bias"]))
        l = F.linear(o, sd["likelihood.logits.weight"], sd["likelihood.logits.bias"])[:, 0]  # [B,V]
        top = l.topk(2, dim=-1).values
        logit_gap = min(logit_gap, float((top[:, 0] - top[:, 1]).min()))
        first_max = (l == top[:, :1]).int().argmax(-1)
        c = (l - top[:, :1]).exp().cumsum(-1)
        cdf = c / c[:, -1:]
        if uniforms is None:
            k = first_max
        else:
            u = uniforms[t].to(dt)
            hit = c >= (u * c[:, -1]).unsqueeze(-1)
            k = torch.where(hit.any(-1), hit.int().argmax(-1), torch.tensor(V - 1))
            below = torch.where(k > 0, cdf.gather(-1, (k - 1).clamp(min=0).unsqueeze(-1)).squeeze(-1), torch.zeros_like(u))
            above = torch.where(k < V - 1, cdf.gather(-1, k.unsqueeze(-1)).squeeze(-1) - u, torch.full_like(u, float("inf")))
            gap = min(gap, float(torch.minimum(u - below, above).min()))
            at_mode += int((k == first_max).sum())
        ks.append(k)
        cdfs.append(cdf)
        pred = levels[k].reshape(-1, 1, 1)
        x = torch.cat([x[:, :, 1:], pred], dim=2)
    k = torch.stack(ks, 1)
    return dict(k=k, x=levels[k].unsqueeze(-1), cdf=torch.stack(cdfs), gap=gap, logit_gap=logit_gap, mode_share=at_mode / k.numel())


def _run(name, P, dtype, sampled=True):
    case = SHAPES[name]
    m = build_model(case)
    prompt, uni = draws(case, P, offset=DRAW_OFFSETS.get((name, P), 0))
    sd = {k: v.detach().to(dtype) for k, v in m.state_dict().items()}
    out = generate_cat(sd, window_of(prompt, case.rf), case.n_frames, case.layers, case.stacks, uni if sampled else None, case.V)
    return m, prompt, uni, out


@functools.lru_cache(maxsize=None)
def reference(name, P):
    """(model on the CPU, prompt, draws, float64 result of `generate_cat`) of a case — computed once, never changed."""
    return _run(name, P, torch.float64)


@functools.lru_cache(maxsize=None)
def reference32(name, P):
    """The same restatement in float32 (for MIN_GAP only)."""
    return _run(name, P, torch.float32)[3]


@functools.lru_cache(maxsize=None)
def mode_reference(name):
    """The float64 restatement from a zero start with arg-max feedback — computed once, never changed."""
    return _run(name, 0, torch.float64, sampled=False)[3]
