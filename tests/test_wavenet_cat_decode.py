"""CPU: the preconditions of tests/test_gpu_wavenet_cat_decode.py (one-launch WaveNet generation with the categorical head) and the
host-side logic around it.  The cases, the float64 restatement and the comparison rule are in tests/wavenet_cat_cases.py."""
import os

import numpy as np
import pytest
import torch

import wavenet_cat_cases as W

from conftest import GOLDEN

ALL_STARTS = W.STARTS + [("v2048", 0)]


def test_min_gap_is_derived_from_the_float32_run():
    """The float32 run of the restatement draws the same classes as the float64 run in every case; the largest |cdf32 - cdf64| it sees
    is what MAX_CDF_ERR32 records (rounded up, by less than a factor 4), and MIN_GAP is 16 times that."""
    worst = 0.0
    for name, P in ALL_STARTS:
        r64, r32 = W.reference(name, P)[3], W.reference32(name, P)
        assert torch.equal(r64["k"], r32["k"]), f"{name} P={P}: the float32 restatement draws other classes"
        worst = max(worst, float((r32["cdf"].double() - r64["cdf"]).abs().max()))
    print(f"largest |cdf32 - cdf64| {worst:.3e}; recorded {W.MAX_CDF_ERR32:.3e}; MIN_GAP {W.MIN_GAP:.3e}")
    assert worst <= W.MAX_CDF_ERR32 <= 4 * worst
    assert W.MIN_GAP == 16 * W.MAX_CDF_ERR32


@pytest.mark.parametrize("name,P", ALL_STARTS)
def test_cases_have_no_near_ties(name, P):
    """The precondition of the every-class comparison, and that the regime is what the header says."""
    case = W.SHAPES[name]
    _, prompt, uni, r = W.reference(name, P)
    assert tuple(r["k"].shape) == (case.B, case.n_frames) and tuple(r["x"].shape) == (case.B, case.n_frames, 1)
    assert int(r["k"].min()) >= 0 and int(r["k"].max()) < case.V
    print(f"{name} P={P}: gap {r['gap']:.3e}, arg-max share {r['mode_share']:.2f}, distinct classes {len(r['k'].unique())}")
    assert r["gap"] >= W.MIN_GAP, f"{name} P={P}: CDF gap {r['gap']:.2e}: pick another seed"
    assert r["mode_share"] < 0.5, "more than half the draws are the arg-max class: the softmax is nearly one-hot"
    assert len(r["k"].unique()) >= 8, "fewer than 8 distinct classes"
    if P:  # the prompt matters
        assert not torch.equal(r["k"], W.reference(name, 0)[3]["k"])


@pytest.mark.parametrize("name", W.KERNEL_CASES)
def test_mode_cases_have_separated_logits(name):
    """The precondition of the arg-max test: the two largest logits are >= 1e-3 apart in every row and frame."""
    r = W.mode_reference(name)
    print(f"{name}: smallest gap between the two largest logits {r['logit_gap']:.3e}")
    assert r["logit_gap"] >= W.MIN_LOGIT_GAP


def test_existing_categorical_generation_test_meets_min_gap():
    """tests/test_gpu_categorical.py::test_generate_window_cached_prompt_and_state_agree (C = 16, V = 32, the golden model) now runs
    through the one-launch kernel and compares classes across paths: its draws (seed 11; the zero start over 14 frames, then the first
    five samples as a prompt for 8 frames) keep MIN_GAP from every CDF boundary in the float64 restatement."""
    g = np.load(os.path.join(GOLDEN, "categorical.npz"))
    tag = "wn1.sd."
    sd = {k[len(tag) :]: torch.from_numpy(g[k]).double() for k in g.files if k.startswith(tag)}
    B, n, V, rf = 3, 14, 32, int(g["wn1.rf"])
    gen = torch.Generator().manual_seed(11)
    uni = [torch.rand(B, generator=gen) for _ in range(n)]
    zero = W.generate_cat(sd, torch.zeros(B, rf, 1), n, 2, 2, uni, V)
    primed = W.generate_cat(sd, W.window_of(zero["x"][:, :5].float(), rf), 8, 2, 2, uni[:8], V)
    print(f"zero start: gap {zero['gap']:.3e}; prompt of 5: gap {primed['gap']:.3e}; MIN_GAP {W.MIN_GAP:.3e}")
    assert zero["gap"] >= W.MIN_GAP and primed["gap"] >= W.MIN_GAP


def _model(likelihood, C=16, **kw):
    from blvm.models import WaveNet

    return WaveNet(likelihood=likelihood, n_layers=2, n_stacks=1, res_channels=C, **kw)


def test_predicate_truth_table():
    from blvm.modules.distributions import CategoricalDense, DiscretizedLogisticMixtureDense

    for V, want in ((8, False), (16, True), (24, False), (256, True), (1024, True), (1040, False), (2048, False), (65536, False)):
        m = _model(CategoricalDense(16, V))
        assert m._cat_decode_kernel_applies() is want, V
        assert m._decode_kernel_applies() is False
    assert _model(CategoricalDense(128, 256), C=128)._cat_decode_kernel_applies() is True
    assert _model(CategoricalDense(144, 256), C=144)._cat_decode_kernel_applies() is False
    dmol = _model(DiscretizedLogisticMixtureDense(16, 1, num_mix=10, num_bins=2**16))
    assert dmol._cat_decode_kernel_applies() is False and dmol._decode_kernel_applies() is True


def test_arguments_are_checked_without_a_device():
    m = W.build_model(W.SHAPES["c16v32"])
    assert m._cat_decode_kernel_applies()
    with pytest.raises(NotImplementedError):
        m.generate(3, 4, cached=False, return_state=True)
    with pytest.raises(ValueError, match="prompt of 2 rows"):
        m.generate(3, 4, x=torch.zeros(2, 5, 1), cached=True)
    with pytest.raises(ValueError, match="a state already contains its past"):
        m.generate(3, 4, x=torch.zeros(3, 5, 1), state=object(), cached=True)


def test_new_entry_points_are_declared_once():
    from blvm import _hip

    i, p, f = _hip.ctypes.c_int, _hip.ctypes.c_void_p, _hip.ctypes.c_float
    sig = _hip.SIGNATURES
    assert sig["blvm_wavenet_cat_decode_pack_floats"] == (_hip.ctypes.c_size_t, [i] * 5)
    assert sig["blvm_wavenet_cat_decode"] == (i, [p, p] + [i] * 7 + [f, f] + [p] * 6)
    assert sig["blvm_wavenet_cat_decode_resume"] == (i, [p, p] + [i] * 8 + [f, f] + [p] * 8)
    lib = _hip.load()
    assert lib.blvm_version() >= 201
    # the DMoL image with its head padded to 32 rows, the categorical one unpadded
    assert lib.blvm_wavenet_cat_decode_pack_floats(32, 32, 32, 4, 32) == lib.blvm_wavenet_decode_pack_floats(32, 32, 32, 4)
    assert lib.blvm_wavenet_cat_decode_pack_floats(32, 32, 32, 4, 256) - lib.blvm_wavenet_decode_pack_floats(32, 32, 32, 4) == 224 * 33


def test_one_packer_builds_the_image_of_either_head():
    """`ops._wavenet_decode_pack` on the smallest model (C = 16, two blocks): the size the library states for the head, and element
    for element the image built part by part, whose tail is the DMoL head padded with zeros to 32 rows or the categorical head as it
    stands.  Exact: the image is a copy of the parameters."""
    from blvm import _hip, ops
    from blvm.modules.distributions import CategoricalDense, DiscretizedLogisticMixtureDense

    lib = _hip.load()
    torch.manual_seed(5)
    dmol, cat = _model(DiscretizedLogisticMixtureDense(16, 1, num_mix=10, num_bins=2**16)), _model(CategoricalDense(16, 48))
    for m, head, lin, want in (
        (dmol, ops.DmolHead(10, dmol.likelihood.log_epsilon), dmol.likelihood.params, lib.blvm_wavenet_decode_pack_floats(16, 16, 16, 2)),
        (cat, ops.CategoricalHead(cat.likelihood.levels), cat.likelihood.logits, lib.blvm_wavenet_cat_decode_pack_floats(16, 16, 16, 2, 48)),
    ):
        rs, hw, hb = m.res_stack, lin.weight, lin.bias
        assert len(rs.res_blocks) == 2 and m.res_channels == 16
        parts = [m.causal.conv.weight, m.causal.conv.bias, rs.in_transform.weight, rs.in_transform.bias]
        for b in rs.res_blocks:
            parts += list(b.kernel_params())
        parts += [m.out_transform.linear.weight, m.out_transform.linear.bias]
        if isinstance(head, ops.DmolHead):
            assert tuple(hw.shape) == (30, 16)
            parts += [hw, hw.new_zeros(2, 16), hb, hb.new_zeros(2)]
        else:
            parts += [hw, hb]
        image = torch.cat([p.detach().float().reshape(-1) for p in parts])
        with torch.no_grad():
            packed = ops._wavenet_decode_pack(m._one_launch_parts(), head)[5]
        assert packed.dtype == torch.float32 and packed.numel() == want == image.numel()
        assert torch.equal(packed, image)
