"""GPU (MI355X): `represent()` of the four latent-variable models, K8r (`ops.particle_mean`), the `LatentRepresentation` front end
and the resampling CTC probe.

Models and fixtures are the small ones of the parity tests (tests/golden/vrnn_small.npz, srnn.npz, stcn.npz, cwvae.npz); the
tolerance against the reference's own z is the one each model's parity test applies to `out.z`:
  vrnn (a, b), srnn (sm, ns): rtol 1e-4, atol 1e-5;   stcn (s8, s1), cwvae (pw, rs): rtol 1e-4, atol 1e-4.
Against `forward` with the same noise the comparison is bit for bit: the same kernels run on the same shapes."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from blvm import _hip, ops
from blvm.data.token_map import TokenMap
from blvm.data.transforms import LatentRepresentation
from blvm.models import CWVAEAudio, SimpleLSTMASR, SRNNAudio, STCN, VRNNAudio

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CW_SMALL = dict(z_size=[32, 16, 16], h_size=16, strides=[4, 2, 2], num_level_layers=2, stride_per_layer=2, likelihood="DMoL",
                num_mix=10, num_bins=2**16)  # fmt: skip
ST_SMALL = dict(likelihood="DMoL", n_layers=3, latent_size=[16, 16, 32], res_channels=16)
CASES = [("vrnn", "a"), ("vrnn", "b"), ("srnn", "sm"), ("srnn", "ns"), ("stcn", "s8"), ("stcn", "s1"), ("cwvae", "pw"), ("cwvae", "rs")]
TOL = dict(vrnn=(1e-4, 1e-5), srnn=(1e-4, 1e-5), stcn=(1e-4, 1e-4), cwvae=(1e-4, 1e-4))
IDS = [f"{n}-{t}" for n, t in CASES]
K = 4


@pytest.fixture(scope="module", autouse=True)
def _require_hip():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert _hip.load().blvm_device_ok() == 1


def T(a):
    return torch.from_numpy(np.asarray(a))


_CASES = {}


def case(name, tag):
    """(model on the device in eval(), x on the device, x_sl, eps in `forward`'s shapes on the device, the reference's z per level
    [B,T,Z]) of a golden fixture; built once."""
    if (name, tag) in _CASES:
        return _CASES[name, tag]
    g = np.load(os.path.join(GOLDEN, {"vrnn": "vrnn_small.npz", "srnn": "srnn.npz", "stcn": "stcn.npz", "cwvae": "cwvae.npz"}[name]))
    sd = lambda pre: {k[len(pre):]: T(g[k]) for k in g.files if k.startswith(pre)}  # noqa: E731
    if name == "vrnn":
        m = VRNNAudio(likelihood="DMoL", input_size=8, hidden_size=32, latent_size=16, residual_posterior=True, num_mix=10, num_bins=2**16)
        m.load_state_dict(sd("sd."))
        x, x_sl, eps, gold = T(g["x"]), T(g["x_sl"]), T(g[f"{tag}_eps"]).to(DEV), [T(g[f"{tag}_z"])]
    elif name == "srnn":
        m = SRNNAudio(likelihood="DMoL", input_size=8, hidden_size=32, latent_size=16, residual_posterior=True, smoothing=tag == "sm")
        m.load_state_dict(sd(f"{tag}_sd."))
        x, x_sl, eps, gold = T(g["x"]), T(g["x_sl"]), T(g[f"{tag}_eps"]).to(DEV), [T(g[f"{tag}_z"])]
    elif name == "stcn":
        m = STCN(**ST_SMALL, n_stack_frames=8 if tag == "s8" else 1)
        m.load_state_dict(sd(f"{tag}_sd."))
        x, x_sl = T(g[f"{tag}_x"]), T(g[f"{tag}_x_sl"])
        eps = [T(g[f"{tag}_eps{l}"]).transpose(0, 1).contiguous().to(DEV) for l in range(3)]  # the reference draws [B,T',z]
        gold = [T(g[f"{tag}_z{l}"]) for l in range(3)]
    else:
        m = CWVAEAudio(**CW_SMALL, **(dict(precision_posterior=True) if tag == "pw" else dict(residual_posterior=True)))
        m.load_state_dict(sd(f"{tag}_sd."))
        x, x_sl = T(g["x"]), T(g["x_sl"])
        eps = [T(g[f"{tag}_eps{l}"]).to(DEV) for l in range(3)]
        gold = [T(g[f"{tag}_z{l}"]) for l in range(3)]
    _CASES[name, tag] = (m.to(DEV).eval(), x.to(DEV), x_sl, eps, gold)
    return _CASES[name, tag]


def as_levels(z, z_sl):
    return ([z], [z_sl]) if torch.is_tensor(z) else (list(z), list(z_sl))


def live_mask(z_sl, T_):
    return torch.arange(T_).unsqueeze(0) < torch.as_tensor(z_sl).to(torch.int64).unsqueeze(1)  # [B,T]


def forward_z(m, x, x_sl, **kw):
    with torch.no_grad():
        out = m(x, x_sl, **kw)[2]
    return as_levels(out.z, out.z_sl)


def check_dead_frames_zero(z, z_sl):
    """z [T,B,Z] time-major: every frame at or beyond z_sl[b] is exactly zero."""
    dead = ~live_mask(z_sl, z.shape[0]).t()  # [T,B]
    assert float(z.cpu()[dead].abs().sum()) == 0.0 and not bool(torch.isnan(z).any())


# ---- 1. against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tag", CASES, ids=IDS)
def test_represent_matches_the_reference_z(name, tag):
    m, x, x_sl, eps, gold = case(name, tag)
    rtol, atol = TOL[name]
    z, z_sl = m.represent(x, x_sl, eps=eps)
    zs, sls = as_levels(z, z_sl)
    _, f_sl = forward_z(m, x, x_sl, eps=eps)
    assert len(zs) == len(gold) == len(sls) == len(f_sl)
    assert torch.is_tensor(z) == (name in ("vrnn", "srnn"))
    for l, (zl, sl, gl) in enumerate(zip(zs, sls, gold)):
        assert zl.dtype == torch.float32 and zl.is_contiguous() and zl.shape[1:] == (x.shape[0], gl.shape[2])  # time-major [T_l,B,Z_l]
        assert torch.equal(torch.as_tensor(sl).to(torch.int64), torch.as_tensor(f_sl[l]).to(torch.int64))
        Tg = min(zl.shape[0], gl.shape[1])
        assert int(torch.as_tensor(sl).max()) <= Tg
        live = live_mask(sl, Tg)
        got = zl.permute(1, 0, 2).cpu()[:, :Tg][live]
        err = float((got - gl[:, :Tg][live]).abs().max())
        print(f"{name}-{tag} level {l}: {int(live.sum())} live frames, max |z - reference| {err:.3e}")
        torch.testing.assert_close(got, gl[:, :Tg][live], rtol=rtol, atol=atol)
        check_dead_frames_zero(zl, sl)
        # the one-level form: the same tensor and lengths
        z1, sl1 = m.represent(x, x_sl, level=l, eps=eps)
        assert torch.is_tensor(z1) and torch.equal(z1, zl) and torch.equal(torch.as_tensor(sl1), torch.as_tensor(sl))
    if name == "cwvae":
        g = np.load(os.path.join(GOLDEN, "cwvae.npz"))
        for l in range(3):
            assert torch.equal(sls[l].to(torch.int64), T(g[f"{tag}_z_sl{l}"]).to(torch.int64))


# ---- 2. against forward, bit for bit ----------------------------------------------------------------------------------------------
def assert_live_equal(zl, fz, sl, what):
    """represent's z [T,B,Z] and forward's [B,T,Z] are the same bits on the live frames."""
    live = live_mask(sl, zl.shape[0])
    a, b = zl.permute(1, 0, 2).cpu()[live], fz.cpu()[:, : zl.shape[0]][live]
    assert torch.equal(a, b), (what, float((a - b).abs().max()))


@pytest.mark.parametrize("name,tag", [c for c in CASES if c[0] != "vrnn"], ids=[i for i in IDS if not i.startswith("vrnn")])
@pytest.mark.parametrize("seeded", [False, True], ids=["eps", "seed"])
def test_represent_equals_forward_bit_for_bit(name, tag, seeded):
    m, x, x_sl, eps, _ = case(name, tag)
    variants = [False, True] if name == "cwvae" else [False]
    for resets in variants:
        if name == "cwvae":
            m.cwvae.with_resets = resets
        try:
            if seeded:
                torch.manual_seed(5)
                fz, _ = forward_z(m, x, x_sl)
                torch.manual_seed(5)
                z, z_sl = m.represent(x, x_sl)
            else:
                fz, _ = forward_z(m, x, x_sl, eps=eps)
                z, z_sl = m.represent(x, x_sl, eps=eps)
        finally:
            if name == "cwvae":
                m.cwvae.with_resets = False
        for l, (zl, sl) in enumerate(zip(*as_levels(z, z_sl))):
            assert_live_equal(zl, fz[l], sl, (name, tag, l, resets, seeded))
            check_dead_frames_zero(zl, sl)


def folding_vrnn():
    """A VRNN whose decoder `forward` folds into the cell's launch (Z == H, DH == H, S * F a multiple of 16)."""
    torch.manual_seed(21)
    m = VRNNAudio(likelihood="DMoL", input_size=16, hidden_size=32, latent_size=32, residual_posterior=True).to(DEV).eval()
    gen = torch.Generator().manual_seed(4)
    x = (torch.rand(3, 16 * 6 - 5, generator=gen) * 2 - 1).to(DEV)
    return m, x, torch.tensor([16 * 6 - 5, 60, 17]), torch.randn(6, 3, 32, generator=gen).to(DEV)


@pytest.mark.parametrize("which", ["a", "b", "folding"])
def test_vrnn_represent_equals_forward(which):
    lib = _hip.load()
    m, x, x_sl, eps = folding_vrnn() if which == "folding" else case("vrnn", which)[:4]
    prev = lib.blvm_vrnn_dec_fold(0)  # both routes build the same launch
    try:
        fz, _ = forward_z(m, x, x_sl, eps=eps)
        z, z_sl = m.represent(x, x_sl, eps=eps)
        assert_live_equal(z, fz[0], z_sl, (which, "eps"))
        torch.manual_seed(8)
        fz, _ = forward_z(m, x, x_sl)
        torch.manual_seed(8)
        z2, _ = m.represent(x, x_sl)
        assert_live_equal(z2, fz[0], z_sl, (which, "seed"))
    finally:
        lib.blvm_vrnn_dec_fold(prev)
    # with the fold as the process has it: the golden tolerance, and whether it was bit-identical all the same
    folds0 = lib.blvm_vrnn_dec_fold(-2)
    fz, _ = forward_z(m, x, x_sl, eps=eps)
    folded = lib.blvm_vrnn_dec_fold(-2) - folds0
    live = live_mask(z_sl, z.shape[0])
    a, b = z.permute(1, 0, 2).cpu()[live], fz[0].cpu()[live]
    print(f"vrnn-{which}: forward folded its decoder: {bool(folded)}; represent vs forward bit-identical: {torch.equal(a, b)}, "
          f"max |diff| {float((a - b).abs().max()):.3e}")  # fmt: skip
    torch.testing.assert_close(a, b, rtol=TOL["vrnn"][0], atol=TOL["vrnn"][1])
    check_dead_frames_zero(z, z_sl)


# ---- 3. pruning, counted ----------------------------------------------------------------------------------------------------------
def counters():
    lib = _hip.load()
    g, n, s = (torch.zeros(17, dtype=torch.int64), torch.zeros(12, dtype=torch.int64), torch.zeros(6, dtype=torch.int64))
    for fn, t in ((lib.blvm_gemm_arm_counts, g), (lib.blvm_rnn_path_counts, n), (lib.blvm_rssm_path_counts, s)):
        fn(ctypes.c_void_p(t.data_ptr()))
    return dict(gemm=int(g.sum()), gru_fwd=int(n[6:9].sum()), rssm_fwd=int(s[0:2].sum()))


def delta(fn):
    c0 = counters()
    fn()
    c1 = counters()
    return {k: c1[k] - c0[k] for k in c0}


@pytest.mark.parametrize("name,tag", [("vrnn", "a"), ("srnn", "sm"), ("stcn", "s8"), ("cwvae", "pw")])
def test_represent_launches_less_than_forward(name, tag):
    m, x, x_sl, eps, _ = case(name, tag)
    fwd = delta(lambda: forward_z(m, x, x_sl, eps=eps))
    rep = delta(lambda: m.represent(x, x_sl, eps=eps))
    print(f"{name}: forward {fwd}, represent {rep}")
    assert 0 < rep["gemm"] < fwd["gemm"], (fwd, rep)
    if name == "srnn":
        assert rep["gru_fwd"] == 2 and fwd["gru_fwd"] == 2
    if name == "stcn":
        top = delta(lambda: m.represent(x, x_sl, level=2, eps=eps))
        mid = delta(lambda: m.represent(x, x_sl, level=1, eps=eps))
        low = delta(lambda: m.represent(x, x_sl, level=0, eps=eps))
        print(f"stcn: level 2 {top}, level 1 {mid}, level 0 {low}")
        assert top["gemm"] < mid["gemm"] < low["gemm"] == rep["gemm"]
    if name == "cwvae":
        assert fwd["rssm_fwd"] == 3 and rep["rssm_fwd"] == 3
        per_level = {l: delta(lambda l=l: m.represent(x, x_sl, level=l, eps=eps)) for l in (2, 1, 0)}
        print(f"cwvae: per level {per_level}")
        assert [per_level[l]["rssm_fwd"] for l in (2, 1, 0)] == [1, 2, 3]
        assert per_level[2]["gemm"] < per_level[1]["gemm"] < per_level[0]["gemm"] == rep["gemm"]


def test_stcn_bottom_up_prunes_from_below():
    torch.manual_seed(2)
    m = STCN(**ST_SMALL, n_stack_frames=8, top_down=False).to(DEV).eval()
    _, x, x_sl, eps, _ = case("stcn", "s8")
    fz, _ = forward_z(m, x, x_sl, eps=eps)
    low = delta(lambda: m.represent(x, x_sl, level=0, eps=eps))
    top = delta(lambda: m.represent(x, x_sl, level=2, eps=eps))
    assert low["gemm"] < top["gemm"], (low, top)
    for l in range(3):
        z, z_sl = m.represent(x, x_sl, level=l, eps=eps)
        assert_live_equal(z, fz[l], z_sl, ("bottom-up", l))
    torch.manual_seed(6)
    fz, _ = forward_z(m, x, x_sl)
    torch.manual_seed(6)
    z, z_sl = m.represent(x, x_sl, level=1)  # draws levels 0 and 1, in forward's order
    assert_live_equal(z, fz[1], z_sl, "bottom-up seeded")


# ---- 4. K8r directly --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Z", [16, 48])
def test_particle_mean_kernel(Z):
    T_, B = 3, 3
    gen = torch.Generator().manual_seed(Z)
    z = torch.randn(T_, 3 * B, Z, generator=gen)
    z[2, 1] = float("nan")  # a dead frame of particle 0 (row 1: lens 1): padding noise must not leave the call
    z[1, B + 2] = float("inf")  # row 2 is empty
    lens = torch.tensor([3, 1, 0], dtype=torch.int32)
    live = (torch.arange(T_).unsqueeze(1) < lens.unsqueeze(0)).unsqueeze(-1)  # [T,B,1]
    zk = z.view(T_, 3, B, Z)
    third = torch.tensor(1 / 3, dtype=torch.float32)
    want3 = torch.where(live, ((zk[:, 0] + zk[:, 1]) + zk[:, 2]) * third, torch.zeros(()))
    want1 = torch.where(live, zk[:, 0], torch.zeros(()))
    zd, ld = z.to(DEV), lens.to(DEV)
    nan_out = lambda: torch.full((T_, B, Z), float("nan"), device=DEV)  # noqa: E731

    one = ops.particle_mean(zd, ld, B, out=nan_out(), scale=1 / 3)  # c = 3 in one pass
    assert torch.equal(one.cpu(), want3)
    assert torch.equal(ops.particle_mean(zd, ld, B, scale=1 / 3).cpu(), want3)  # allocates its own output
    assert torch.equal(ops.particle_mean(zd, ld, B, out=nan_out(), scale=1 / 3), one)  # repeats bit for bit

    first = zd[:, :B].contiguous()
    k1 = ops.particle_mean(first, ld, B, out=nan_out())  # c = 1, scale 1: z with its dead frames zeroed
    assert torch.equal(k1.cpu(), want1)

    two = nan_out()
    ops.particle_mean(zd[:, : 2 * B].contiguous(), ld, B, out=two, first=True, last=False)
    mid = two.clone()
    ops.particle_mean(zd[:, 2 * B :].contiguous(), ld, B, out=two, first=False, last=True, scale=1 / 3)
    assert torch.equal(two, one)  # two passes (2 + 1 particles) are the single pass, bit for bit
    # an unfinished pass holds the plain sums, dead frames included (they are masked by the last pass only)
    assert torch.equal(mid.cpu()[live.expand_as(mid)], (zk[:, 0] + zk[:, 1])[live.expand_as(mid)])

    three = nan_out()
    for k in range(3):
        ops.particle_mean(zd[:, k * B : (k + 1) * B].contiguous(), ld, B, out=three, first=k == 0, last=k == 2, scale=1 / 3)
    assert torch.equal(three, one)


def test_particle_mean_many_blocks_and_errors():
    """More items than one grid pass (4096 blocks x 256 threads) so the grid-stride loop wraps, against the torch expression."""
    T_, B, Z, c = 70, 64, 1024, 2
    gen = torch.Generator().manual_seed(1)
    z = torch.randn(T_, c * B, Z, generator=gen).to(DEV)
    lens = torch.randint(0, T_ + 1, (B,), generator=gen).to(torch.int32)
    assert T_ * B * Z // 4 > 4096 * 256
    got = ops.particle_mean(z, lens.to(DEV), B, scale=0.5)
    live = (torch.arange(T_).unsqueeze(1) < lens.unsqueeze(0)).unsqueeze(-1).to(DEV)
    want = torch.where(live, (z[:, :B] + z[:, B:]) * 0.5, torch.zeros((), device=DEV))
    assert torch.equal(got, want)
    with pytest.raises(_hip.BlvmHipError, match="multiple of 4"):
        ops.particle_mean(torch.zeros(2, 3, 6, device=DEV), lens[:3].to(DEV), 3)
    with pytest.raises(_hip.BlvmHipError, match="first"):
        ops.particle_mean(torch.zeros(2, 3, 8, device=DEV), lens[:3].to(DEV), 3, first=False)


# ---- 5. particles in the models ---------------------------------------------------------------------------------------------------
def particle_eps(eps, seed):
    """K particles' noise with the particle axis in front; particle 0 is the fixture's."""
    gen = torch.Generator().manual_seed(seed)
    more = lambda e: torch.cat([e.cpu().unsqueeze(0), torch.randn(K - 1, *e.shape, generator=gen)]).to(DEV)  # noqa: E731
    return [more(e) for e in eps] if isinstance(eps, list) else more(eps)


@pytest.mark.parametrize("name,tag", [("vrnn", "a"), ("srnn", "sm"), ("stcn", "s8"), ("cwvae", "pw")])
def test_particles_agree_across_pass_splits_and_with_single_draws(name, tag):
    m, x, x_sl, eps, _ = case(name, tag)
    B = x.shape[0]
    rtol, atol = TOL[name]
    ek = particle_eps(eps, 31)
    runs = {rows: as_levels(*m.represent(x, x_sl, num_samples=K, eps=ek, max_rows=rows)) for rows in (B, 3 * B, 4 * B, None)}
    singles = [as_levels(*m.represent(x, x_sl, eps=[e[k] for e in ek] if isinstance(ek, list) else ek[k]))[0] for k in range(K)]
    quarter = torch.tensor(0.25, dtype=torch.float32, device=DEV)
    for l in range(len(runs[None][0])):
        ref, sl = runs[None][0][l], runs[None][1][l]
        for rows in (B, 3 * B, 4 * B):
            got = runs[rows][0][l]
            print(f"{name} level {l}: max_rows {rows} vs default bit-identical: {torch.equal(got, ref)}, max |diff| {float((got - ref).abs().max()):.3e}")
            torch.testing.assert_close(got, ref, rtol=rtol, atol=atol)
        mean = (((singles[0][l] + singles[1][l]) + singles[2][l]) + singles[3][l]) * quarter
        torch.testing.assert_close(ref, mean, rtol=rtol, atol=atol)
        check_dead_frames_zero(ref, sl)
        assert torch.equal(torch.as_tensor(sl), torch.as_tensor(as_levels(*m.represent(x, x_sl, eps=eps))[1][l]))
    # K particles drawn on the device run too, and differ from one draw
    torch.manual_seed(1)
    zk = as_levels(*m.represent(x, x_sl, num_samples=K))[0]
    assert all(bool(torch.isfinite(t).all()) for t in zk) and not torch.equal(zk[-1], runs[None][0][-1])


@pytest.mark.parametrize("name,tag", [("vrnn", "a"), ("srnn", "sm"), ("stcn", "s8"), ("cwvae", "pw")])
def test_deterministic_front_runs_once_whatever_k(name, tag):
    """At max_rows = B every particle is a pass of its own: with E the GEMM launches of the deterministic front alone,
    gemm(K) = E + K * per_pass (the counter arithmetic of test_gpu_iw_models.py::test_deterministic_part_runs_once)."""
    m, x, x_sl, eps, _ = case(name, tag)
    B = x.shape[0]
    ek = particle_eps(eps, 32)
    with torch.no_grad():
        if name == "vrnn":
            S, enc_lin, _, _ = m.vrnn._plan()
            det = delta(lambda: m.vrnn._encode(x, x_sl, S, enc_lin))
        elif name == "srnn":
            S, enc_lin, _, _ = m.srnn._plan()
            det = delta(lambda: m.srnn._deterministic(x, x_sl, None, None, S, enc_lin))
        elif name == "stcn":
            det = delta(lambda: m._front(x, x_sl, None, True))
        else:
            det = delta(lambda: m.cwvae._front(x, x_sl, None, False, True))
    d1 = delta(lambda: m.represent(x, x_sl, num_samples=1, eps=eps, max_rows=B))
    d4 = delta(lambda: m.represent(x, x_sl, num_samples=K, eps=ek, max_rows=B))
    print(f"{name}: deterministic front {det}, represent K=1 {d1}, K={K} {d4}")
    per_pass = d1["gemm"] - det["gemm"]
    assert per_pass >= 0 and d4["gemm"] == det["gemm"] + K * per_pass, (det, d1, d4)
    if name != "stcn":
        assert det["gemm"] > 0
    if name == "srnn":
        assert det["gru_fwd"] == 2 and d1["gru_fwd"] == 2 and d4["gru_fwd"] == 2
    if name == "cwvae":
        assert det["rssm_fwd"] == 0 and d1["rssm_fwd"] == 3 and d4["rssm_fwd"] == 3 * K


def test_represent_follows_the_process_operand_mode_and_model_state():
    m, x, x_sl, eps, _ = case("vrnn", "a")
    z32, _ = m.represent(x, x_sl, eps=eps)
    m.train()
    try:
        zt, _ = m.represent(x, x_sl, eps=eps)  # evaluation-only: the same in either `training` state
    finally:
        m.eval()
    assert torch.equal(zt, z32)
    # bf16 operands: represent does not force fp32 (iw_bound does), so it is `forward` under that mode, bit for bit (fold off: the
    # same launch on both routes), and the mode is left as it was
    lib = _hip.load()
    _hip.set_operand_dtype("bf16")
    prev = lib.blvm_vrnn_dec_fold(0)
    try:
        z16, z_sl = m.represent(x, x_sl, eps=eps)
        assert _hip.get_operand_dtype() == "bf16"
        fz, _ = forward_z(m, x, x_sl, eps=eps)
    finally:
        lib.blvm_vrnn_dec_fold(prev)
        _hip.set_operand_dtype("f32")
    assert_live_equal(z16, fz[0], z_sl, "bf16")
    check_dead_frames_zero(z16, z_sl)
    print(f"bf16 vs fp32 operands: max |diff| {float((z16 - z32).abs().max()):.3e}")
    assert not any(p.grad is not None for p in m.parameters())


# ---- 6. the probe step ------------------------------------------------------------------------------------------------------------
def _experiments():
    sys.path.insert(0, os.path.join(ROOT, "experiments"))
    try:
        import _asr
    finally:
        sys.path.pop(0)
    return _asr


def probe_step(kind, level, seed=3):
    """The front end on a synthetic model plus one forward / backward step of the probe -> what the test looks at."""
    asr = _experiments()
    rep, frame_samples = asr.synthetic_model(kind, seed)
    rep = rep.to(DEV).train()
    frozen = {k: v.clone() for k, v in rep.state_dict().items()}
    fe = LatentRepresentation(rep, level=level, num_samples=1)
    (x, x_sl), (y, y_sl) = next(iter(asr.SyntheticWaveforms(1, 4, 6, 36, frame_samples[level], seed, pad_to=max(frame_samples))))
    torch.manual_seed(seed)
    feats, lens = fe(x.to(DEV), x_sl)
    assert torch.equal(torch.as_tensor(lens).to(torch.int64), x_sl // frame_samples[level]) and bool((lens >= 2 * y_sl).all())
    probe = SimpleLSTMASR(TokenMap([f"t{i}" for i in range(6)], add_blank=True), input_size=feats.size(1), hidden_size=128).to(DEV).train()
    seen = []
    hook = probe.lstm.register_forward_pre_hook(lambda mod, args: seen.append(args[0]))
    loss, metrics, out = probe(feats, lens, y.to(DEV), y_sl)
    hook.remove()
    loss.backward()
    torch.cuda.synchronize()
    return rep, frozen, fe, feats, probe, seen, loss


def test_probe_step_on_resampled_vrnn_latents():
    rep, frozen, fe, feats, probe, seen, loss = probe_step("vrnn", 0)
    assert not rep.training and all(not p.requires_grad for p in rep.parameters())
    assert math.isfinite(float(loss.detach()))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in probe.parameters())
    assert all(p.grad is None for p in rep.parameters())
    assert all(torch.equal(v, frozen[k]) for k, v in rep.state_dict().items())
    # the hand-off copies nothing: the tensor the LSTM block receives is represent's output
    assert tuple(feats.shape) == (4, 16, seen[0].shape[0]) and not feats.is_contiguous()
    assert len(seen) == 1 and seen[0].is_contiguous() and seen[0].data_ptr() == feats.data_ptr()
    assert tuple(seen[0].shape) == (feats.shape[2], 4, 16)
    # every call draws afresh
    torch.manual_seed(99)
    again, _ = fe(torch.zeros(4, 64, device=DEV), torch.tensor([64, 64, 48, 32]))
    other, _ = fe(torch.zeros(4, 64, device=DEV), torch.tensor([64, 64, 48, 32]))
    assert not torch.equal(again, other)


# ---- 7. the script ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,level", [("srnn", 0), ("stcn", 2), ("cwvae", 1)])
def test_front_end_and_one_probe_step_on_the_other_synthetic_models(kind, level):
    rep, frozen, fe, feats, probe, seen, loss = probe_step(kind, level)
    assert math.isfinite(float(loss.detach()))
    assert all(p.grad is not None for p in probe.parameters()) and all(p.grad is None for p in rep.parameters())
    assert all(torch.equal(v, frozen[k]) for k, v in rep.state_dict().items())
    assert seen[0].data_ptr() == feats.data_ptr()


def test_resampling_script_runs_one_synthetic_epoch():
    cmd = [sys.executable, os.path.join(ROOT, "experiments", "experiment_asr_ctc_resampling.py"), "--dataset", "synthetic",
           "--synthetic_model", "vrnn", "--epochs", "1", "--batch_size", "4", "--synthetic_utterances", "16", "--synthetic_frames", "36",
           "--hidden_size", "128", "--seed", "1", "--device", "0"]  # fmt: skip
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    train = [ln for ln in lines if ln.startswith("epoch") and "frames/s" in ln]
    test = [ln for ln in lines if ln.strip().startswith("test ")]
    assert len(train) == 1 and len(test) == 1, r.stdout[-2000:]
    for ln in train + test:
        words = ln.replace("|", " ").replace(",", " ").split()
        pairs = dict(zip(words, words[1:]))  # every word with the one after it: "loss" -> its value
        for key in ("loss", "wer", "cer"):
            assert key in pairs and math.isfinite(float(pairs[key])), ln
    assert "skipped" not in train[0], train[0]
