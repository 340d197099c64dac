"""CPU: what the categorical head (K7d) rests on that needs no GPU — the fixture tests/golden/categorical.npz (the reference's float32
`CategoricalDense` + `categorical_ll(reduce_dim=None)`, `Quantize`, a tiny reference WaveNet) against the float64 truth and the float32
composition of tests/cat_cases.py, `Quantize` / `CategoricalDense.dequantize`, the state_dict layout and the refusals."""
import os

import numpy as np
import pytest
import torch

import cat_cases as CC
from conftest import GOLDEN


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "categorical.npz"))


def T_(a):
    return torch.from_numpy(np.asarray(a))


@pytest.mark.parametrize("shape", CC.SHAPES, ids=lambda s: "B{}_T{}_S{}_C{}_V{}".format(*s))
def test_reference_values_against_the_float64_truth(g, shape):
    """The reference's float32 values (all of ll and log_prob, gradients at the sampled frames and classes) are the float32
    composition of cat_cases — to the last few bits, since both are `nn.Linear`, `logsumexp`, `gather` in float32 — and lie within
    the float32 bound of the float64 truth: the fixture, the truth and the GPU tests' `ref32` describe the same function."""
    for regime in CC.REGIMES:
        case = CC.make_case(shape, regime)
        t64, t32, fl = CC.compose(case, torch.float64), CC.compose(case, torch.float32), None
        fl = CC.floors(case, t64)
        fr, cl = CC.sampled(case)
        tag = "op." + CC.case_id(shape, regime)
        C = case["C"]
        picks = {"ll": lambda t: t["ll"], "log_prob": lambda t: t["log_prob"], "d_x": lambda t: t["d_x"].reshape(-1, C)[fr],
                 "dW": lambda t: t["dW"][cl], "db": lambda t: t["db"][cl]}  # fmt: skip
        floors = {"ll": fl["ll"], "log_prob": fl["ll"].sum(1), "d_x": fl["d_x"].reshape(-1, C)[fr], "dW": fl["dW"][cl], "db": fl["db"][cl]}
        for name, pick in picks.items():
            ref, truth, mine = T_(g[f"{tag}.{name}"]).double(), pick(t64).double(), pick(t32).double()
            assert ref.shape == truth.shape, (tag, name)
            # a float32 evaluation may err by a few times the any-order bound (its own sums are not the kernel's)
            assert ((ref - truth).abs() <= 8 * floors[name] + 1e-30).all(), (tag, name, float((ref - truth).abs().max()))
            assert ((ref - mine).abs() <= 8 * floors[name] + 1e-30).all(), (tag, name, float((ref - mine).abs().max()))
        if regime == "equal":
            assert torch.allclose(T_(g[f"{tag}.ll"])[case["valid"][:, : case["T"]]].double(), torch.tensor(-np.log(case["V"])), atol=1e-5)


def test_cases_exercise_what_they_claim():
    for shape in CC.SHAPES:
        c = CC.make_case(shape, "peaked")
        t = CC.compose(c, torch.float64)
        rng = (t["logits"].max(-1).values - t["logits"].min(-1).values)[c["valid"]]
        assert 60 < float(rng.mean()) < 100
        c = CC.make_case(shape, "garbage_padding")
        assert torch.isnan(c["X_in"][~c["valid"]]).all() and not torch.isnan(c["X"]).any()
        bad = c["y_in"][~c["valid"][:, : c["T"]]]
        assert ((bad == -7) | (bad == c["V"] + 5)).all() and (~c["valid"]).any()
        c = CC.make_case(shape, "empty_utterance")
        assert int(c["x_sl"][-1]) == 0
        c = CC.make_case(shape, "last_class")
        assert (CC.compose(c, torch.float64)["logits"].argmax(-1)[c["valid"]] == c["V"] - 1).all()
    assert float(CC.compose(CC.make_case(CC.SHAPES[3], "peaked"), torch.float64)["ll"].min()) < -60


@pytest.mark.parametrize("bits", [8, 4])
def test_quantize_matches_the_reference_on_edge_values(g, bits):
    from blvm.data.transforms import Quantize
    from blvm.modules.distributions import CategoricalDense

    x, k = T_(g[f"q.{bits}.x"]), T_(g[f"q.{bits}.k"])
    q = Quantize(bits=bits)
    got = q(x)
    assert got.dtype == k.dtype and torch.equal(got, k)
    assert torch.equal(Quantize(bits=None, bins=2**bits)(x), k)
    assert Quantize(bits=bits, force_out_int64=False)(x).dtype == torch.int32
    # round trip: dequantize(k) quantises back to k, for every class; rescale=True returns those values
    V = 2**bits
    lik = CategoricalDense(16, V) if V >= 2 else None
    classes = torch.arange(V)
    values = lik.dequantize(classes)
    assert torch.equal(values, torch.linspace(-1, 1, V)) and torch.equal(q(values), classes)
    assert torch.equal(Quantize(bits=bits, rescale=True)(x), values[k.clamp(max=V - 1)])
    with pytest.raises(AssertionError):
        Quantize(bits=8, bins=256)


def test_categorical_dense_has_the_reference_state_dict_and_init(g):
    from blvm.models import WaveNet
    from blvm.modules.distributions import CategoricalDense

    torch.manual_seed(3)
    lik = CategoricalDense(16, 32)
    torch.manual_seed(3)
    lin = torch.nn.Linear(16, 32)
    assert list(lik.state_dict()) == ["logits.weight", "logits.bias"]
    assert torch.equal(lik.logits.weight, lin.weight) and torch.equal(lik.logits.bias, lin.bias)
    for nsf in (1, 2):
        m = WaveNet(likelihood=CategoricalDense(16, 32), n_layers=2, n_stacks=2, res_channels=16, n_stack_frames=nsf)
        tag = f"wn{nsf}.sd."
        sd = {k[len(tag) :]: T_(g[k]) for k in g.files if k.startswith(tag)}
        assert sorted(sd) == sorted(m.state_dict())
        m.load_state_dict(sd)
        assert m.receptive_field == int(g[f"wn{nsf}.rf"])
    # per-frame log_prob on materialised logits: the reference's values
    case = CC.make_case(CC.SHAPES[0], "random")
    lik = CategoricalDense(case["C"], case["V"])
    logits = torch.nn.functional.linear(case["X"], case["W"], case["b"])[:, : case["T"]]
    ll = lik.log_prob(case["y"], logits) * case["valid"][:, : case["T"]]
    torch.testing.assert_close(ll, T_(g["op." + CC.case_id(CC.SHAPES[0], "random") + ".ll"]), rtol=1e-6, atol=1e-6)


def test_fixture_wavenet_targets_are_the_quantised_input(g):
    from blvm.data.transforms import Quantize

    for nsf in (1, 2):
        x, y = T_(g[f"wn{nsf}.x"]), T_(g[f"wn{nsf}.y"])
        assert torch.equal(Quantize(bits=None, bins=32)(x).clamp(max=31), y) and int(y.max()) == 31 and int(y.min()) == 0


def test_refusals():
    from blvm import ops
    from blvm.models import WaveNet
    from blvm.modules.distributions import CategoricalDense

    with pytest.raises(NotImplementedError, match="C = 24"):
        CategoricalDense(24, 10)
    with pytest.raises(NotImplementedError, match="V = 1"):
        CategoricalDense(16, 1)
    for C, V in ((24, 10), (16, 1), (528, 4), (16, 65537)):
        with pytest.raises(NotImplementedError):  # before any device work: CPU tensors get this far
            ops.categorical_log_prob(torch.zeros(4, C), torch.zeros(V, C), torch.zeros(V), torch.zeros(2, 2, dtype=torch.int64), None, 2, 2, 2, 1)
    with pytest.raises(NotImplementedError, match="embedding"):
        WaveNet(likelihood=CategoricalDense(16, 32), embedding_dim=8, n_layers=2, n_stacks=2, res_channels=16)
    m = WaveNet(likelihood=CategoricalDense(16, 32), n_layers=2, n_stacks=2, res_channels=16)
    with pytest.raises(TypeError, match="integer"):
        m(torch.zeros(1, 20), torch.tensor([20]), y=torch.zeros(1, 20))
    assert not m._decode_kernel_applies()


def test_sampler_draw_check_accepts_the_exact_inverse_cdf_and_rejects_a_neighbour():
    """The draw check itself: the float64 inverse CDF passes; a class two bins away fails."""
    logits, u = CC.sampler_case(256, "random")
    e = (logits.double() - logits.double().max(-1, keepdim=True).values).exp()
    c = e.cumsum(-1)
    k = (c >= (u.double() * c[:, -1]).unsqueeze(-1)).int().argmax(-1)
    assert CC.check_draws(logits, u, k) <= 1.0
    with pytest.raises(AssertionError):
        CC.check_draws(logits, u, (k + 2).clamp(max=255))
