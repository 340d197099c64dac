"""CPU: the preconditions of tests/test_gpu_wavenet_embed.py (WaveNet with embedded class input, K10e) and the host-side logic around
it.  The cases, the float64 restatements, the bounds and the tie rule are in tests/wavenet_embed_cases.py."""
import os
import sys

import numpy as np
import pytest
import torch

import wavenet_embed_cases as W

from conftest import GOLDEN


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "wavenet_embed.npz"))


# ---- restatements -------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("tag", ["cat16", "cat32", "cat16n"])
def test_restatement_equals_the_reference_golden(g, tag):
    """The float64 restatement of the embedded model (`front_torch` in front of the oracle's residual stack) gives the ll the
    unmodified reference's modules gave in float32: the tolerances of the GPU test's ll."""
    ll = W.fixture_ll(g, tag)
    want = torch.from_numpy(g[f"{tag}.ll"])
    assert tuple(ll.shape) == tuple(want.shape)
    torch.testing.assert_close(ll.float(), want, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(ll.sum(1).float(), torch.from_numpy(g[f"{tag}.log_prob"]), rtol=1e-5, atol=1e-3)


def test_fixtures_hold_the_edge_classes_and_float_targets(g):
    for tag, (head, E, pad_rf) in W.FIXTURES.items():
        k = torch.from_numpy(g[f"{tag}.x"])
        assert tuple(k.shape) == (3, 37) and int(k.min()) == 0 and int(k.max()) == 31 and g[f"{tag}.x_sl"].tolist() == [37, 22, 9]
        assert bool(g[f"{tag}.pad_rf"]) is pad_rf and tuple(g[f"{tag}.sd.embedding.weight"].shape) == (32, E)
        y = torch.from_numpy(g[f"{tag}.y"])
        want = k if head == "cat" else torch.linspace(-1.0, 1.0, 32)[k]
        assert torch.equal(y, want if pad_rf else want[:, int(g[f"{tag}.rf"]) :])
        assert g[f"{tag}.grad.embedding.weight"].shape == (32, E) and np.abs(g[f"{tag}.grad.embedding.weight"]).max() > 0


@pytest.mark.parametrize("shape", W.FRONT_SHAPES)
@pytest.mark.parametrize("pad_causal", [False, True])
def test_table_form_equals_embedding_and_grouped_conv_in_float64(shape, pad_causal):
    c = W.front_case(*shape)
    emb, cw, bias = c["emb"].double(), c["cw"].double(), c["bias"].double()
    a, b = W.front_torch(c["k"], emb, cw, bias, pad_causal), W.front_tables(c["k"], emb, cw, bias, pad_causal)
    assert tuple(a.shape) == (shape[3] - 1 - int(pad_causal), shape[4], shape[1])
    err = float((a - b).abs().max())
    print(f"V={shape[0]} C={shape[1]} m={shape[2]}: largest |table form - embedding + conv| {err:.2e}")
    assert err <= 4e-15 * float(a.abs().max())
    k = c["k"]
    assert bool((k[:3] == -1).all()) and bool((k == 0).any()) and bool((k == shape[0] - 1).any())
    assert bool((W.tables(emb, cw)[:, shape[0]] == 0).all())


def test_skewed_regime_is_what_the_header_says():
    V, C, m, L, B = W.SKEWED
    k = W.front_case(*W.SKEWED, skew=0.9)["k"]
    assert L * B == 40000 and C == 64
    share = float((k == V // 3).float().mean())
    assert 0.88 < share < 0.92, share
    c, grads, bounds, empty = W.grad_reference(W.FRONT_SHAPES[3], True)
    assert int(empty.sum()) > 60000  # the V = 65536 case is sparse: most classes have no frame
    assert bool((grads[0][empty] == 0).all())


# ---- the model's construction -------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("tag", list(W.FIXTURES))
def test_state_dict_keys_and_shapes_are_the_reference_s(g, tag):
    m = W.fixture_model(g, tag)
    want = {k[len(tag) + 4 :]: tuple(g[k].shape) for k in g.files if k.startswith(f"{tag}.sd.")}
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    E = W.FIXTURES[tag][1]
    assert want["embedding.weight"] == (32, E) and want["causal.conv.weight"] == (16, E // 16, 2) and want["causal.conv.bias"] == (16,)
    assert m.receptive_field == int(g[f"{tag}.rf"])
    assert [k for k, _ in m.named_parameters()] == [k[len(tag) + 6 :] for k in g.files if k.startswith(f"{tag}.grad.")]


def test_the_reference_s_two_value_errors_and_the_other_refusals():
    from blvm.models import WaveNet
    from blvm.models.wavenet import CausalConv1d
    from blvm.modules.distributions import CategoricalDense, DiscretizedLogisticMixtureDense

    kw = dict(likelihood=CategoricalDense(16, 32), n_layers=2, n_stacks=2, res_channels=16, num_bins=32)
    with pytest.raises(ValueError, match="Cannot stack frames"):
        WaveNet(embedding_dim=16, n_stack_frames=2, **kw)
    with pytest.raises(ValueError, match="more than 1 input_channel"):
        WaveNet(embedding_dim=16, in_channels=2, **kw)
    with pytest.raises(NotImplementedError, match="embedding"):
        WaveNet(embedding_dim=24, **kw)
    for bad in (dict(groups=2), dict(groups=16, kernel_size=1)):
        with pytest.raises(NotImplementedError):
            CausalConv1d(16, 16, **{"kernel_size": 2, **bad})
    conv = CausalConv1d(32, 16, kernel_size=2, groups=16)
    assert tuple(conv.conv.weight.shape) == (16, 2, 2)
    with pytest.raises(NotImplementedError, match="fused with the embedding"):
        conv.forward_tm(torch.zeros(4, 1, 32))
    m = WaveNet(embedding_dim=16, **kw)
    assert m._cat_decode_kernel_applies() is True and m._decode_kernel_applies() is False
    # the classes are targets only for a head of as many classes; generation needs the categorical head
    other = WaveNet(likelihood=CategoricalDense(16, 48), embedding_dim=16, num_bins=32, n_layers=2, n_stacks=2, res_channels=16)
    with pytest.raises(ValueError, match="give y"):
        other(torch.zeros(1, 20, dtype=torch.long), torch.tensor([20]))
    with pytest.raises(ValueError, match="cannot feed an embedding"):
        other.generate(1, 2)
    dmol = WaveNet(likelihood=DiscretizedLogisticMixtureDense(16, 1, num_mix=10, num_bins=256), embedding_dim=16, num_bins=32, n_layers=2,
                   n_stacks=2, res_channels=16)  # fmt: skip
    for cached in (False, True):
        with pytest.raises(NotImplementedError, match="categorical head"):
            dmol.generate(1, 2, cached=cached)


def test_float_input_is_quantised_by_the_categorical_target_s_rule():
    """`_classes` on the edge values of tests/golden/categorical.npz (`q.*`: +-1, 0, every boundary, every boundary +- 1 ulp)."""
    from blvm.models import WaveNet
    from blvm.modules.distributions import CategoricalDense

    q = np.load(os.path.join(GOLDEN, "categorical.npz"))
    for bits in (8, 4):
        V = 2**bits
        m = WaveNet(likelihood=CategoricalDense(16, V), embedding_dim=16, num_bins=V, n_layers=2, n_stacks=1, res_channels=16)
        x, k = torch.from_numpy(q[f"q.{bits}.x"]), torch.from_numpy(q[f"q.{bits}.k"])
        assert torch.equal(m._classes(x.unsqueeze(0)), k.clamp(max=V - 1).unsqueeze(0))
        assert torch.equal(m._classes(k.clamp(max=V - 1).unsqueeze(0).int()), k.clamp(max=V - 1).unsqueeze(0))
        assert torch.equal(m._classes(m.levels.unsqueeze(0)), torch.arange(V).unsqueeze(0))


def test_the_experiment_flag_reaches_the_constructor(monkeypatch):
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "experiments")
    monkeypatch.syspath_prepend(here)
    monkeypatch.delitem(sys.modules, "experiment_wavenet_audio", raising=False)
    import experiment_wavenet_audio as E

    args = E.parser.parse_args(["--likelihood", "Categorical", "--num_bits", "8", "--input_embedding_dim", "64", "--n_layers", "2", "--n_stacks", "1"])
    m = E.build_model(args)
    assert m.embedding_dim == 64 and m.num_bins == 256 and tuple(m.embedding.weight.shape) == (256, 64)
    assert tuple(m.causal.conv.weight.shape) == (64, 1, 2) and m.causal.groups == 64 and m.likelihood.y_dim == 256
    args = E.parser.parse_args(["--likelihood", "Categorical", "--num_bits", "8", "--n_layers", "2", "--n_stacks", "1"])
    m = E.build_model(args)
    assert m.embedding is None and m.embedding_dim is None and tuple(m.causal.conv.weight.shape) == (64, 1, 2) and m.causal.groups == 1


def test_new_entry_points_are_declared():
    from blvm import _hip

    i, p, f, z = _hip.ctypes.c_int, _hip.ctypes.c_void_p, _hip.ctypes.c_float, _hip.ctypes.c_size_t
    sig = _hip.SIGNATURES
    assert sig["blvm_wavenet_embed_tables"] == (i, [p, p, i, i, i, p, p])
    assert sig["blvm_wavenet_embed_fwd"] == (i, [p, p, p] + [i] * 5 + [p, p])
    assert sig["blvm_wavenet_embed_bwd_workspace_floats"] == (z, [i] * 4)
    assert sig["blvm_wavenet_embed_bwd"] == (i, [p] * 4 + [i] * 5 + [p] * 8)
    assert sig["blvm_wavenet_embed_cat_decode"] == (i, [p, p, p] + [i] * 7 + [f, f] + [p] * 6)
    assert sig["blvm_wavenet_embed_cat_decode_resume"] == (i, [p, p, p] + [i] * 8 + [f, f] + [p] * 8)
    lib = _hip.load()
    assert lib.blvm_version() >= 203
    assert lib.blvm_wavenet_embed_bwd_workspace_floats(0, 32, 16, 1) == 0
    # 300 sorted frames: three chunks of 128, each two partial rows of two taps and one bias row; 32 classes: one dcw partial
    assert lib.blvm_wavenet_embed_bwd_workspace_floats(300, 32, 16, 2) == 3 * 4 * 16 + 3 * 16 + 2 * 32


def test_the_packer_takes_the_tables_in_the_causal_weights_place():
    """`ops._wavenet_decode_pack` on an embedded model's parts with CPU tensors: the image has the float model's layout with zeros where
    the causal weights were, and the tables come back beside it."""
    from blvm import ops

    case = W.SHAPES["e16"]
    m = W.build_model(case)
    tabs = W.tables(m.embedding.weight.detach(), m.causal.conv.weight.detach())
    rs, t_in = m.res_stack, m.res_stack.in_transform
    weights = ((tabs, m.causal.conv.bias), (t_in.weight.view(t_in.out_channels, -1), t_in.bias), [b.kernel_params() for b in rs.res_blocks],
               rs.dilations, (m.out_transform.linear.weight, m.out_transform.linear.bias), (m.likelihood.logits.weight, m.likelihood.logits.bias))  # fmt: skip
    with torch.no_grad():
        out = ops._wavenet_decode_pack(weights, ops.CategoricalHead(m.likelihood.levels))
    packed, got_tabs = out[5], out[7]
    assert torch.equal(got_tabs, tabs) and bool((packed[: 2 * case.C] == 0).all())
    assert torch.equal(packed[2 * case.C : 3 * case.C], m.causal.conv.bias.detach())


# ---- the tie rule ---------------------------------------------------------------------------------------------------------------------------


def test_min_gap_is_derived_from_the_float32_run():
    """As tests/test_wavenet_cat_decode.py: the float32 run of the restatement draws the same classes as the float64 run in every
    case; the largest |cdf32 - cdf64| it sees is what MAX_CDF_ERR32 records (rounded up, by less than a factor 4); MIN_GAP is 16 x."""
    worst = 0.0
    for name, P in W.STARTS:
        r64, r32 = W.reference(name, P)[3], W.reference32(name, P)
        assert torch.equal(r64["k"], r32["k"]), f"{name} P={P}: the float32 restatement draws other classes"
        worst = max(worst, float((r32["cdf"].double() - r64["cdf"]).abs().max()))
    print(f"largest |cdf32 - cdf64| {worst:.3e}; recorded {W.MAX_CDF_ERR32:.3e}; MIN_GAP {W.MIN_GAP:.3e}")
    assert worst <= W.MAX_CDF_ERR32 <= 4 * worst
    assert W.MIN_GAP == 16 * W.MAX_CDF_ERR32


@pytest.mark.parametrize("name,P", W.STARTS)
def test_cases_have_no_near_ties(name, P):
    case = W.SHAPES[name]
    _, prompt, uni, r = W.reference(name, P)
    assert tuple(r["k"].shape) == (case.B, case.n_frames) and tuple(prompt.shape) == (case.B, P)
    assert int(r["k"].min()) >= 0 and int(r["k"].max()) < case.V
    print(f"{name} P={P}: gap {r['gap']:.3e}, arg-max share {r['mode_share']:.2f}, distinct classes {len(r['k'].unique())}")
    assert r["gap"] >= W.MIN_GAP, f"{name} P={P}: CDF gap {r['gap']:.2e}: pick another seed"
    assert r["mode_share"] < 0.5 and len(r["k"].unique()) >= 8
    if P:  # the prompt matters
        assert not torch.equal(r["k"], W.reference(name, 0)[3]["k"])
