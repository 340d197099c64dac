"""GPU: VRNN and SRNN roll-outs with the GMM and Gaussian heads in one launch (`blvm_vrnn_generate_head`, `blvm_srnn_generate_head`,
`blvm_vrnn_decode_head`), against the float64 restatement (gauss_rollout_reference.py) over EVERY element, against the step-by-step
path on the same draws, and the engine's properties for the new kinds.

The bar of every comparison is 16 * e_ref absolute, e_ref = the largest difference between the unmodified reference's fp32 samples
and the restatement on the fixture's draws (tests/golden/generate_gauss.npz: 3.0e-7, so the bar is 4.8e-6): seven steps feed rounding
back through a GRU, and the 16-wide fma tiles sum in another order than the CPU's BLAS.  No pick of any case is closer than 1e-3
(test_gauss_rollout_cpu.py), so no element is left out.  Each test prints its figures before it asserts."""
import contextlib
import os

import numpy as np
import pytest
import torch

import gauss_rollout_cases as C
import gauss_rollout_reference as G
from blvm import _hip, ops
from blvm.models import SRNNAudio, VRNNAudio
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = lambda a: torch.from_numpy(np.asarray(a))  # noqa: E731


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "generate_gauss.npz"))


@pytest.fixture(scope="module")
def bar(fixture):
    return 16.0 * float(fixture["e_ref"])


def _dev(t):
    return None if t is None else t.to(DEV)


def err(a, ref):
    return float((a.detach().double().cpu() - ref.double()).abs().max())


def run_vrnn(m, d, fused, use_mode=False, **kw):
    """-> x [B,T,S] (the leading start frame checked and cut off)."""
    B, S = d.x0.shape
    (x, x_sl), _ = m.generate(n_samples=B, max_timesteps=d.eps.shape[0], x=_dev(d.x0).reshape(B, S, 1), h0=_dev(d.h0), eps=_dev(d.eps),
                              uniforms=(_dev(d.u), _dev(d.n)), use_mode=use_mode, fused=fused, **kw)  # fmt: skip
    assert tuple(x.shape) == (B, d.eps.shape[0] + 1, S) and x_sl.tolist() == [d.eps.shape[0] + 1] * B
    assert torch.equal(x[:, 0].cpu(), d.x0)
    return x[:, 1:]


def run_srnn(m, d, fused, use_mode=False):
    """-> (x [B,T,S], h_p [B,R+Z])."""
    B, S = d.x0.shape
    (x, x_sl), out = m.generate(n_samples=B, max_timesteps=d.eps.shape[0], x=_dev(d.x0).reshape(B, 1, S), d_0=_dev(d.h0), z_0=_dev(d.z0), eps=_dev(d.eps),
                                uniforms=(_dev(d.u), _dev(d.n)), use_mode=use_mode, fused=fused)  # fmt: skip
    assert tuple(x.shape) == (B, d.eps.shape[0], S, 1) and x_sl.tolist() == [d.eps.shape[0]] * B
    return x.squeeze(-1), out.h_p.reshape(B, -1)


# ---- 1. the reference fixture -------------------------------------------------------------------------------------------------


def test_fixture_gmm_vrnn_both_paths_against_the_restatement(fixture, bar):
    g = fixture
    m = VRNNAudio(likelihood="GMM", input_size=16, hidden_size=32, latent_size=16, residual_posterior=True, num_mix=10, num_bins=2**16)
    sd = {k[6:]: T(g[k]) for k in g.files if k.startswith("vr_sd.")}
    m.load_state_dict(sd)
    m = m.to(DEV)
    d = C.Draws(T(g["vr_x0"]).reshape(5, 16), T(g["vr_eps"]), T(g["vr_u"]), T(g["vr_n"]), None, None)
    ref = G.vrnn_generate(sd, G.GMM, d.x0, d.eps, d.u, d.n)
    e = {fused: err(run_vrnn(m, d, fused), ref["x"]) for fused in (True, False)}
    e_golden = err(run_vrnn(m, d, True), T(g["vr_x"])[:, 1:])
    print(f"vrnn fixture: one launch {e[True]:.3e}, step by step {e[False]:.3e}, one launch vs the reference's samples {e_golden:.3e}, bar {bar:.3e}")
    _hip.check_async()
    assert e[True] <= bar and e[False] <= bar and e_golden <= bar + float(g["e_ref"])


def test_fixture_gmm_srnn_both_paths_against_the_restatement(fixture, bar):
    g = fixture
    m = SRNNAudio(likelihood="GMM", input_size=16, hidden_size=32, latent_size=16, residual_posterior=True, smoothing=True)
    sd = {k[6:]: T(g[k]) for k in g.files if k.startswith("sr_sd.")}
    m.load_state_dict(sd)
    m = m.to(DEV)
    d = C.Draws(torch.zeros(5, 16), T(g["sr_eps"]), T(g["sr_u"]), T(g["sr_n"]), None, None)
    ref = G.srnn_generate(sd, G.GMM, d.x0, d.eps, d.u, d.n)
    e = {}
    for fused in (True, False):
        x, h_p = run_srnn(m, d, fused)
        e[fused] = (err(x, ref["x"]), err(h_p, ref["h_p"]))
    print(f"srnn fixture: one launch x {e[True][0]:.3e} h_p {e[True][1]:.3e}, step by step x {e[False][0]:.3e} h_p {e[False][1]:.3e}, bar {bar:.3e}")
    _hip.check_async()
    assert max(e[True]) <= bar and max(e[False]) <= bar
    assert g["sr_x_sl"].tolist() == [7] * 5


# ---- 2. edge shapes -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", C.ALL_CASES, ids=lambda c: c.id)
def test_edge_shapes_one_launch_step_by_step_and_restatement(case, bar):
    sd, d, ref = C.prepared(case)
    m = C.make_model(case)
    m.load_state_dict(sd)
    m = m.to(DEV)
    if case.model == "vrnn":
        a, b = run_vrnn(m, d, True, case.use_mode), run_vrnn(m, d, False, case.use_mode)
        e = dict(one=err(a, ref["x"]), step=err(b, ref["x"]), paths=err(a, b.cpu()))
    else:
        (a, ha), (b, hb) = run_srnn(m, d, True, case.use_mode), run_srnn(m, d, False, case.use_mode)
        e = dict(one=err(a, ref["x"]), step=err(b, ref["x"]), paths=err(a, b.cpu()), h_p_one=err(ha, ref["h_p"]), h_p_step=err(hb, ref["h_p"]))
    print(f"{case.id}: " + ", ".join(f"{k} {v:.3e}" for k, v in e.items()) + f", bar {bar:.3e}")
    _hip.check_async()
    assert torch.isfinite(a).all() and max(e.values()) <= bar, e


# ---- 3. the per-CU form -------------------------------------------------------------------------------------------------------


def _vrnn_ops(m, d, head, **kw):
    """ops.vrnn_decode as `VRNN._generate_gauss` calls it -> (x [B,T,S], h_n)."""
    v = m.vrnn
    S, enc_lin, dec_lin, lik = v._plan()
    c = v.vrnn_cell
    return ops.vrnn_decode(enc_lin, c.kernel_params(), dec_lin, lik.params, _dev(d.x0), _dev(d.h0), _dev(d.eps), _dev(d.u), _dev(d.n), S, c.h_dim, c.z_dim,
                           c.r_dim, getattr(head, "num_mix", 0), c.prior[6].epsilon, 0.01, 0.0, head=head, **kw)  # fmt: skip


def test_per_cu_form_gmm_above_the_batch_limit(bar):
    from blvm.modules.distributions import gauss_rollout_head

    nb = ops.load().blvm_pchain_max_batch()
    case = C.Case("vrnn", "GMM", 16, nb + 1)
    m = C.make_model(case, seed=0)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    seed = C.find_seed(case, sd)  # (by the restatement alone; a batch the cases' table cannot know)
    d = C.make_draws(case, seed)
    ref = C.restate(case, sd, d)
    m = m.to(DEV)
    head = gauss_rollout_head(m.vrnn.likelihood)
    x_cu, h_cu = _vrnn_ops(m, d, head, whole_chip=False)
    first = C.Draws(d.x0[:nb], d.eps[:, :nb], d.u[:, :nb], d.n[:, :nb], None, None)
    x_wc, h_wc = _vrnn_ops(m, first, head, whole_chip=True)
    e = dict(restatement=err(x_cu, ref["x"]), h_n=err(h_cu, ref["h_n"]), whole_chip=err(x_cu[:nb], x_wc.cpu()), whole_chip_h=err(h_cu[:nb], h_wc.cpu()))
    print(f"per-CU GMM B {nb + 1} seed {seed}: " + ", ".join(f"{k} {v:.3e}" for k, v in e.items()) + f", bar {bar:.3e}")
    _hip.check_async()
    assert max(e.values()) <= bar, e
    # the default dispatch takes this form above the limit (S % 16 == 0) ...
    assert err(run_vrnn(m, d, None), ref["x"]) <= bar
    # ... and the Gaussian head is refused there with the library's message
    gm = C.make_model(C.Case("vrnn", "Gaussian", 16, 3), seed=0).to(DEV)
    dg = C.make_draws(C.Case("vrnn", "Gaussian", 16, 3), 0)
    with pytest.raises(_hip.BlvmHipError, match=r"not the Gaussian head \(kind 2\)"):
        _vrnn_ops(gm, dg, gauss_rollout_head(gm.vrnn.likelihood), whole_chip=False)


# ---- 4. engine properties -----------------------------------------------------------------------------------------------------


@contextlib.contextmanager
def counting(monkeypatch, name):
    """Counts the library calls named `name` that blvm.ops checks."""
    seen, real = [], ops.check
    with monkeypatch.context() as mp:
        mp.setattr(ops, "check", lambda rc, what: (seen.append(what) if what == name else None, real(rc, what))[1])
        yield seen


class Fill:
    """Stand-in for `torch` inside blvm.ops: `empty` returns its float32 buffer filled with one 32-bit word."""

    def __init__(self, word):
        self.word, self.buffers = word, []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *a, **k):
        t = torch.empty(*a, **k)
        if t.numel() and t.dtype == torch.float32:
            t.view(torch.int32).fill_(self.word)
            self.buffers.append(t)
        return t


def _srnn_ops(m, d, head, **kw):
    s = m.srnn
    S, enc_lin, dec_lin, lik = s._plan()
    return ops.srnn_generate(enc_lin, s.d_forward_recurrent, s._chain_params(), dec_lin, lik.params, _dev(d.x0), _dev(d.h0), _dev(d.z0), _dev(d.eps), _dev(d.u),
                             _dev(d.n), S, s.h_dim, s.z_dim, s.r_dim, getattr(head, "num_mix", 0), s.prior[6].epsilon, 0.01, 0.0, head=head, **kw)  # fmt: skip


ENGINE = [C.Case("vrnn", "GMM", 6, 17), C.Case("srnn", "Gaussian", 24, 3), C.Case("srnn", "GMM", 16, 3), C.Case("vrnn", "Gaussian", 1, 17)]


@pytest.mark.parametrize("case", ENGINE, ids=lambda c: c.id)
def test_chunked_repeated_and_poisoned_launches_are_bit_identical(case, monkeypatch):
    """(a) chunked under max_scratch_floats (one step per launch: three launches) == one launch, final states included; (b) a second
    identical call == the first; (c) scratch and outputs filled with NaN words and with the hand-off sentinel before the call: the same."""
    from blvm.modules.distributions import gauss_rollout_head

    sd, d, _ = C.prepared(case)
    m = C.make_model(case)
    m.load_state_dict(sd)
    m = m.to(DEV)
    lib = ops.load()
    if case.model == "vrnn":
        head = gauss_rollout_head(m.vrnn.likelihood)
        call, name = (lambda **kw: _vrnn_ops(m, d, head, whole_chip=True, **kw)), "blvm_vrnn_generate_head"
        one_step = lib.blvm_vrnn_generate_scratch_floats_head(1, case.B, case.S, C.H, C.Z, C.R, ops._head_scalars(head)[0])
    else:
        head = gauss_rollout_head(m.srnn.likelihood)
        call, name = (lambda **kw: _srnn_ops(m, d, head, **kw)), "blvm_srnn_generate_head"
        one_step = lib.blvm_srnn_generate_scratch_floats_head(1, case.B, case.S, C.H, C.Z, C.R, ops._head_scalars(head)[0])
    with counting(monkeypatch, name) as seen:
        single = call()
    assert len(seen) == 1 and one_step > 0
    with counting(monkeypatch, name) as seen:
        chunked = call(max_scratch_floats=one_step)
    assert len(seen) == C.T == 3
    again = call()
    for a, b, c in zip(single, chunked, again):
        assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(a, c)
    for word in (0x7FC00000, -1):
        with monkeypatch.context() as mp:
            h = Fill(word)
            mp.setattr(ops, "torch", h)
            got = call()
        assert len(h.buffers) >= 3
        for a, b in zip(single, got):
            assert torch.equal(a, b), f"results depend on what the buffers held (word {word:#x})"
    torch.cuda.synchronize()
    _hip.check_async()


@pytest.mark.parametrize("model", ["vrnn", "srnn"])
def test_refused_head_leaves_planted_buffers_untouched(model, monkeypatch):
    case = C.Case(model, "GMM", 6, 3)
    m = C.make_model(case, seed=0).to(DEV)
    d = C.make_draws(case, 0)
    for head, message in ((ops.GmmHead(5, 0.69, 1e-4), "10 components"), (ops.GmmHead(10, -1.0, 1e-4), "must not be negative")):
        with monkeypatch.context() as mp:
            h = Fill(0x40E80000)  # 7.25
            mp.setattr(ops, "torch", h)
            with pytest.raises(_hip.BlvmHipError, match=message):
                (_vrnn_ops(m, d, head, whole_chip=True) if model == "vrnn" else _srnn_ops(m, d, head))
        torch.cuda.synchronize()
        assert len(h.buffers) >= 3 and all(bool((b == 7.25).all()) for b in h.buffers)


def test_dmol_rollouts_are_bit_equal_through_old_and_new_entry_points(monkeypatch):
    """generate16.npz's draws: fused=True through blvm_vrnn_generate / blvm_srnn_generate == the same call with an explicit DMoL
    `head=` through the *_head entry points."""
    g = np.load(os.path.join(GOLDEN, "generate16.npz"))
    v = VRNNAudio(likelihood="DMoL", input_size=16, hidden_size=32, latent_size=16, residual_posterior=True, num_mix=10, num_bins=2**16)
    v.load_state_dict({k[6:]: T(g[k]) for k in g.files if k.startswith("vr_sd.")})
    s = SRNNAudio(likelihood="DMoL", input_size=16, hidden_size=32, latent_size=16, residual_posterior=True, smoothing=True)
    s.load_state_dict({k[6:]: T(g[k]) for k in g.files if k.startswith("sr_sd.")})
    v, s = v.to(DEV), s.to(DEV)

    def both():
        (xv, _), _ = v.generate(n_samples=5, max_timesteps=7, x=T(g["vr_x0"]).to(DEV), eps=T(g["vr_eps"]).to(DEV),
                                uniforms=(T(g["vr_u"]).to(DEV), T(g["vr_u2"]).to(DEV)), fused=True)  # fmt: skip
        uni = [(u.to(DEV), u2.to(DEV)) for u, u2 in zip(T(g["sr_u"]), T(g["sr_u2"]))]
        (xs, _), out = s.srnn.generate(x=torch.zeros(5, 1, 16, device=DEV), n_samples=5, max_timesteps=7, eps=T(g["sr_eps"]).to(DEV), uniforms=uni, fused=True)
        return xv, xs, out.h_p

    with counting(monkeypatch, "blvm_vrnn_generate") as a, counting(monkeypatch, "blvm_srnn_generate") as b:
        old = both()
    assert len(a) == len(b) == 1
    rv, rs = ops.vrnn_decode, ops.srnn_generate
    monkeypatch.setattr(ops, "vrnn_decode", lambda *p, **k: rv(*p, head=ops.DmolHead(10, -7.0), **k))
    monkeypatch.setattr(ops, "srnn_generate", lambda *p, **k: rs(*p, head=ops.DmolHead(10, -7.0), **k))
    with counting(monkeypatch, "blvm_vrnn_generate_head") as a, counting(monkeypatch, "blvm_srnn_generate_head") as b:
        new = both()
    assert len(a) == len(b) == 1
    for x, y in zip(old, new):
        assert torch.isfinite(x).all() and torch.equal(x, y)
    _hip.check_async()


# ---- 5. dispatch --------------------------------------------------------------------------------------------------------------


@contextlib.contextmanager
def counting_ops(monkeypatch, name):
    seen, real = [], getattr(ops, name)
    with monkeypatch.context() as mp:
        mp.setattr(ops, name, lambda *a, **k: (seen.append(k.get("head")), real(*a, **k))[1])
        yield seen


@pytest.mark.parametrize("model,head", [(m, h) for m in ("vrnn", "srnn") for h in ("GMM", "Gaussian")])
def test_default_dispatch_takes_the_one_launch_path_and_falls_back_without_noise(model, head, monkeypatch, bar):
    name = "vrnn_decode" if model == "vrnn" else "srnn_generate"
    case = C.Case(model, head, 6, 3)
    m = C.make_model(case, seed=0).to(DEV)

    def seeded(fused, mm=m, **kw):
        torch.manual_seed(11)
        (x, _), _ = mm.generate(n_samples=3, max_timesteps=4, fused=fused, **kw)
        return x

    with counting_ops(monkeypatch, name) as seen:
        auto = seeded(None)
    assert len(seen) == 1 and type(seen[0]).__name__ == ("GmmHead" if head == "GMM" else "GaussHead")
    assert torch.isfinite(auto).all() and torch.equal(auto, seeded(True))
    # the same seed on the step-by-step path replays the same draws: equal to the bar's accuracy (T = 4)
    e = err(auto, seeded(False).cpu())
    print(f"{model} {head}: seeded one launch vs seeded step by step {e:.3e}, bar {bar:.3e}")
    assert e <= bar
    # a call the one-launch kernels do not take — a batch above the persistent path's limit with a stack the per-CU form does not
    # take either (S = 6; the Gaussian head has no per-CU form at all): the default falls back before it draws anything
    nb = ops.load().blvm_pchain_max_batch() + 1

    def seeded_big(fused):
        torch.manual_seed(13)
        (x, _), _ = m.generate(n_samples=nb, max_timesteps=2, fused=fused)
        return x

    with counting_ops(monkeypatch, name) as seen:
        x_auto = seeded_big(None)
    assert seen == [] and torch.isfinite(x_auto).all() and torch.equal(x_auto, seeded_big(False))
    with pytest.raises(_hip.BlvmHipError):
        seeded_big(True)
    _hip.check_async()


@pytest.mark.parametrize("model", ["vrnn", "srnn"])
def test_five_components_are_refused_when_fused_is_asked_for(model):
    torch.manual_seed(0)
    cls = VRNNAudio if model == "vrnn" else SRNNAudio
    m = cls(likelihood="GMM", input_size=6, hidden_size=32, latent_size=16, num_mix=5).to(DEV)
    with pytest.raises(_hip.BlvmHipError, match="10 components"):
        m.generate(n_samples=3, max_timesteps=2, fused=True)
    (x, _), _ = m.generate(n_samples=3, max_timesteps=2)  # the default serves it step by step
    assert torch.isfinite(x).all()
