"""CPU: WaveNet with the Gaussian and Gaussian-mixture heads — the restated forward against the reference's values
(tests/golden/wavenet_gauss.npz, tools/gen_golden_wavenet_gauss.py), the preconditions of the generation cases of
tests/wavenet_gauss_cases.py, the one-launch predicate, the argument checks and the two new entry points of the ABI."""
import os
import re

import numpy as np
import pytest
import torch

from blvm import _hip, ops

from conftest import GOLDEN, ROOT
from test_wavenet_prompt import MIN_GAP
import wavenet_gauss_cases as W

GOLDEN_HEADS = {"gauss": ("Gaussian", 1), "gmm3": ("GMM-3", 1), "gmm10": ("GMM-10", 1), "stk": ("GMM-3", 4)}


def T(a):
    return torch.from_numpy(np.asarray(a))


def close(a, b, rtol, atol):
    torch.testing.assert_close(a.detach(), T(b).to(a.dtype), rtol=rtol, atol=atol)


@pytest.mark.parametrize("p,pad_rf", [("s", True), ("n", False)])
@pytest.mark.parametrize("tag", list(GOLDEN_HEADS))
def test_restated_forward_reproduces_the_reference(tag, p, pad_rf):
    """The float32 restatement against the reference, at the tolerances tests/test_oracle_golden.py holds `O.wavenet_forward` to on
    wavenet.npz."""
    g = np.load(os.path.join(GOLDEN, "wavenet_gauss.npz"))
    head, nsf = GOLDEN_HEADS[tag]
    pre = f"{tag}.sd."
    sd = {k[len(pre) :]: T(g[k]).clone().requires_grad_(True) for k in g.files if k.startswith(pre)}
    x = T(g[f"{tag}.x"]).clone().requires_grad_(True)
    out = W.forward_restated(sd, x, T(g[f"{tag}.x_sl"]), 3, 2, head, n_stack_frames=nsf, pad_receptive_field=pad_rf)
    close(out["loss"], g[f"{tag}.{p}_loss"], 1e-6, 0)
    close(out["log_prob"], g[f"{tag}.{p}_log_prob"], 1e-6, 1e-4)
    close(out["log_prob_twise"], g[f"{tag}.{p}_ll_twise"], 1e-5, 1e-5)
    out["loss"].backward()
    close(x.grad, g[f"{tag}.{p}_dx"], 1e-4, 1e-7)
    for k, prm in sd.items():
        ref = T(g[f"{tag}.{p}_grad.{k}"])
        assert (prm.grad - ref).norm() / (ref.norm() + 1e-12) < 2e-5, k
    names = g[f"{tag}.{p}_metric_names"].tolist()
    assert names == ["loss", "ll", "bpd"]
    assert out["bpd"] == pytest.approx(float(g[f"{tag}.{p}_metric_values"][2]), rel=1e-5)


def test_golden_file_holds_only_arrays():
    with np.load(os.path.join(GOLDEN, "wavenet_gauss.npz"), allow_pickle=False) as g:
        for k in g.files:
            assert g[k].dtype.kind in "fiubU", (k, g[k].dtype)
    assert os.path.getsize(os.path.join(GOLDEN, "wavenet_gauss.npz")) < 2**20


@pytest.mark.parametrize("shape,head,P", W.ALL_CASES)
def test_cases_have_no_near_ties(shape, head, P):
    """The precondition of the every-sample comparison on the GPU; the samples are no constant and a prompt moves them."""
    case = W.case_of(shape, head)
    _, prompt, uni, x64, gap = W.reference(shape, head, P)
    assert tuple(x64.shape) == (case.B, case.n_frames, 1) and bool(torch.isfinite(x64).all())
    assert gap >= MIN_GAP, f"{shape} {head} P={P}: perturbed-logit gap {gap:.2e}: pick another seed"
    assert float(x64.std()) > 0.01, f"{shape} {head} P={P}: the samples are (nearly) constant"
    if P:
        assert float((x64 - W.reference(shape, head, 0)[3]).abs().max()) > 0.05, "the prompt does not move the samples"


@pytest.mark.parametrize("shape,head", sorted({(s, h) for s, h, _ in W.ALL_CASES}))
def test_mode_cases_have_no_near_ties(shape, head):
    x64, gap = W.mode_reference(shape, head)
    assert bool(torch.isfinite(x64).all()) and gap >= MIN_GAP, f"{shape} {head}: logit gap {gap:.2e}"


def test_restated_generation_in_float32_follows_float64():
    """The restatement itself is stable in the regime: its float32 run stays within the GPU tests' tolerance of its float64 run."""
    from test_wavenet_prompt import TOL, window_of

    for shape, head, P in [("g16", "GMM-3", 11), ("g16", "Gaussian", 40), ("g16", "GMM-11", 11)]:
        case = W.case_of(shape, head)
        m, prompt, uni, x64, _ = W.reference(shape, head, P)
        sd32 = {k: v.detach() for k, v in m.state_dict().items()}
        x32, _ = W.generate_f64(sd32, window_of(prompt, case.rf), case.n_frames, case.layers, case.stacks, uni, head)
        assert bool(((x32.double() - x64).abs() <= TOL * x64.abs().clamp(min=1)).all())


@pytest.mark.parametrize("n,C,want", [(1, 128, True), (10, 128, True), (11, 128, False), (1, 144, False), (10, 144, False), (11, 144, False),
                                      (0, 128, True), (0, 144, False)])  # fmt: skip
def test_gauss_decode_predicate(n, C, want):
    """n components (0: the plain Gaussian head) at C channels: one launch for 3 n <= 32 head rows at the decode kernel's widths."""
    from blvm.models import WaveNet

    head = W.Head("Gaussian" if n == 0 else f"GMM-{n}")
    m = WaveNet(likelihood=head.module(C), n_layers=2, n_stacks=1, res_channels=C)
    assert m._gauss_decode_kernel_applies() is want
    assert m._decode_kernel_applies() is False and m._cat_decode_kernel_applies() is False
    assert m._decode_widths_fit() is (C == 128)


def test_other_heads_do_not_take_the_gaussian_arm():
    from blvm.models import WaveNet
    from blvm.modules.distributions import CategoricalDense, DiagonalGaussianMixtureDense, DiscretizedLogisticMixtureDense

    for lik in (DiscretizedLogisticMixtureDense(16, 1, num_mix=10), CategoricalDense(16, 32)):
        assert WaveNet(likelihood=lik, n_layers=2, n_stacks=1, res_channels=16)._gauss_decode_kernel_applies() is False
    two = WaveNet(likelihood=DiagonalGaussianMixtureDense(16, 2, num_mix=3), n_layers=2, n_stacks=1, res_channels=16)
    assert two._gauss_decode_kernel_applies() is False  # y_dim = 2


def test_arguments_are_checked_without_a_device():
    m = W.build_model("g16", "GMM-3")
    with pytest.raises(NotImplementedError):
        m.generate(3, 4, cached=False, return_state=True)
    with pytest.raises(ValueError):
        m.generate(3, 4, x=torch.zeros(2, 5, 1), cached=True)
    with pytest.raises(ValueError):
        m.generate(3, 4, x=torch.zeros(3, 5, 1), state=object(), cached=True)
    # an embedded model trains with a Gaussian head and is refused in generate
    from blvm.models import WaveNet

    emb = WaveNet(likelihood=W.Head("GMM-3").module(16), embedding_dim=16, num_bins=32, n_layers=2, n_stacks=1, res_channels=16)
    with pytest.raises(NotImplementedError, match="categorical head"):
        emb.generate(2, 3)
    # the component count of K7b
    dec, y, sl = torch.zeros(4, 3 * 17), torch.zeros(2, 2), torch.zeros(2, dtype=torch.int32)
    for n in (0, 17):
        with pytest.raises(NotImplementedError, match=f"num_mix = {n}"):
            ops.gmm_log_prob(dec, None, None, y, sl, 0, 2, 2, 2, 1, n, 1.0, 1e-4)
        with pytest.raises(NotImplementedError, match=f"num_mix = {n}"):
            ops.gmm_ll_twise(dec, None, None, y, sl, 0, 2, 2, 2, 1, n, 1.0, 1e-4)
    # ops.wavenet_decode: the draws of the Gaussian heads and the head Linear's rows
    parts = m._one_launch_parts()
    gmm = ops.GmmHead(3, 0.69, 1e-4)
    with pytest.raises(ValueError, match="draws"):
        ops.wavenet_decode(parts, gmm, 3, 4, 0.7, 1.0, draws=(torch.zeros(4, 3, 3), torch.zeros(4, 2)))
    with pytest.raises(ValueError, match="draws"):
        ops.wavenet_decode(parts, gmm, 3, 4, 0.7, 1.0, draws=(torch.zeros(4, 3, 10), torch.zeros(4, 3)))
    with pytest.raises(NotImplementedError, match="outputs"):
        ops.wavenet_decode(parts, ops.GmmHead(10, 0.69, 1e-4), 3, 4, 0.7, 1.0)
    with pytest.raises(NotImplementedError, match="outputs"):
        ops.wavenet_decode(parts, ops.GaussHead(0.69, 1e-4), 3, 4, 0.7, 1.0)
    with pytest.raises(ValueError, match="sd_beta"):
        ops.wavenet_decode(parts, ops.GmmHead(3, 0.0, 1e-4), 3, 4, 0.7, 1.0)
    g = W.build_model("g16", "Gaussian")
    with pytest.raises(ValueError, match="draws"):
        ops.wavenet_decode(g._one_launch_parts(), ops.GaussHead(0.69, 1e-4), 3, 4, 0.7, 1.0, draws=torch.zeros(4, 3, 1))
    # the entry point refuses a head_kind it does not know before it looks at anything else
    lib = _hip.load()
    for kind in (0, 3):
        assert lib.blvm_wavenet_gauss_decode(None, None, 1, 1, 16, 16, 16, kind, 3, 1, 1.0, 1.0, 1.0, 0.0, None, None, None, None, None) != 0
        assert f"got {kind}" in lib.blvm_last_error().decode()


def test_the_abi_declares_the_two_new_entry_points_once():
    header = open(os.path.join(ROOT, "include", "blvm_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    for name, n_args in (("blvm_wavenet_gauss_decode", 19), ("blvm_wavenet_gauss_decode_resume", 22)):
        assert len(re.findall(rf"\b{name}\s*\(", code)) == 1, name
        res, args = _hip.SIGNATURES[name]
        assert len(args) == n_args, name
        assert len(getattr(_hip.load(), name).argtypes) == n_args
