"""CPU: what the GMM / Gaussian roll-out tests stand on — the reference fixture `generate_gauss.npz` against the float64 restatement
(gauss_rollout_reference.py), the pick margins of the fixture and of every case of gauss_rollout_cases.py, the host plans of the two
heads (tests/host/gauss_rollout_plan_test.hip, also under the address and undefined-behaviour sanitizers), the scratch sizes and the
refusals of the *_head entry points (all host arithmetic: nothing is launched), and `DiagonalGaussianDense.sample(noise=)`."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import gauss_rollout_cases as C
import gauss_rollout_reference as G
from blvm import _hip, ops
from conftest import GOLDEN, ROOT

T = lambda a: torch.from_numpy(np.asarray(a))  # noqa: E731


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "generate_gauss.npz"))


def _sd(g, prefix):
    return {k[len(prefix):]: T(g[k]) for k in g.files if k.startswith(prefix)}


def test_fixture_leaves_no_pick_to_chance_and_the_restatement_reproduces_the_reference(fixture):
    """Every component pick of the fixture has a margin >= 1e-3 (recomputed here), and the float64 restatement on the fixture's draws
    gives the reference's fp32 samples to the stored `e_ref`, which is what an fp32 evaluation of seven steps leaves: below 1e-6."""
    g = fixture
    B, S = 5, 16
    rv = G.vrnn_generate(_sd(g, "vr_sd."), G.GMM, T(g["vr_x0"]).reshape(B, S), T(g["vr_eps"]), T(g["vr_u"]), T(g["vr_n"]))
    rs = G.srnn_generate(_sd(g, "sr_sd."), G.GMM, torch.zeros(B, S), T(g["sr_eps"]), T(g["sr_u"]), T(g["sr_n"]))
    assert float(rv["margins"].min()) >= 1e-3 and float(rs["margins"].min()) >= 1e-3
    assert float(rv["margins"].min()) == pytest.approx(float(g["vr_min_margin"])) and float(rs["margins"].min()) == pytest.approx(float(g["sr_min_margin"]))
    assert tuple(g["vr_x"].shape) == (B, 8, S) and tuple(g["sr_x"].shape) == (B, 7, S, 1)
    e_vr = float((T(g["vr_x"])[:, 1:].double() - rv["x"]).abs().max())
    e_sr = float((T(g["sr_x"]).squeeze(-1).double() - rs["x"]).abs().max())
    e_hp = float((T(g["sr_h_p"]).reshape(B, -1).double() - rs["h_p"]).abs().max())
    assert max(e_vr, e_sr) == pytest.approx(float(g["e_ref"]), rel=1e-6) and e_hp == pytest.approx(float(g["e_ref_h_p"]), rel=1e-6)
    assert 0 < float(g["e_ref"]) < 1e-6
    assert np.array_equal(g["vr_x"][:, 0], g["vr_x0"].reshape(B, S))  # the leading start frame


@pytest.mark.parametrize("case", [c for c in C.ALL_CASES if c.head == "GMM"], ids=lambda c: c.id)
def test_every_gmm_case_has_its_first_seed_with_clear_picks(case):
    sd, d, ref = C.prepared(case)
    assert float(ref["margins"].min()) >= C.MIN_MARGIN
    assert C.find_seed(case, sd) == C.SEEDS[case.id]
    assert torch.isfinite(ref["x"]).all() and tuple(ref["x"].shape) == (case.B, C.T, case.S)


def test_cases_cover_the_edge_shapes_of_the_tile():
    shapes = {(c.S, c.B) for c in C.EDGE_CASES}
    assert shapes == {(S, B) for S in (1, 6, 16, 24) for B in (3, 17)}
    for model in ("vrnn", "srnn"):
        for head in ("GMM", "Gaussian"):
            assert sum(c.model == model and c.head == head for c in C.EDGE_CASES) == 8
            assert any(c.model == model and c.head == head and c.use_mode for c in C.ALL_CASES)
    assert {c.model for c in C.START_CASES} == {"vrnn", "srnn"} and set(C.SEEDS) == {c.id for c in C.ALL_CASES}


def _hipcc(src, exe, *extra):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'benchmarking-lvms_amd', 'csrc')}"]
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", *extra, *inc, src, "-o", str(exe)], check=True, timeout=900)
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)


def test_host_plans_of_the_gmm_and_gaussian_heads(tmp_path):
    """tests/host/gauss_rollout_plan_test.hip: Np, Sp, the u / v strides, the tile's LDS floats, the reads of the dec slab, the replay of
    the GMM programs, kind 0 field for field — and the scratch sizes it prints against the library's *_scratch_floats_head."""
    out = _hipcc(os.path.join(ROOT, "tests", "host", "gauss_rollout_plan_test.hip"), tmp_path / "gauss_rollout_plan_test")
    assert out.returncode == 0 and "40 cases, 0 errors" in out.stdout, out.stdout + out.stderr
    lib = _hip.load()
    lines = re.findall(r"^scratch (\w+) (\d) (\d+) (\d+) (\d+) (\d+)$", out.stdout, flags=re.M)
    assert len(lines) == 32
    for model, kind, T_, B, S, floats in lines:
        fn = lib.blvm_vrnn_generate_scratch_floats_head if model == "vrnn" else lib.blvm_srnn_generate_scratch_floats_head
        assert fn(int(T_), int(B), int(S), 48, 16, 32, int(kind)) == int(floats), (model, kind, B, S)


def test_host_plans_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same plan-building host code as a stand-alone program of its own, with the sanitizers on the host side of the compile."""
    out = _hipcc(os.path.join(ROOT, "tests", "host", "gauss_rollout_plan_test.hip"), tmp_path / "gauss_rollout_plan_test_san", "-g", "-Xarch_host",
                 "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined")  # fmt: skip
    assert out.returncode == 0 and "40 cases, 0 errors" in out.stdout and "runtime error" not in out.stderr, out.stdout + out.stderr


def test_dmol_step_programs_are_the_ones_built_before_the_heads(tmp_path):
    """tools/dump_rollout_program.hip without arguments prints every DMoL program of its grid (VRNN, SRNN, LSTM: header, strides, every
    descriptor field, pointers as offsets, scratch sizes): the digest of that text as the plan printed it before the draw tile had head
    kinds.  Kind 0 is field for field the program built then; `--heads` adds the GMM and Gaussian programs behind it."""
    import hashlib

    out = _hipcc(os.path.join(ROOT, "tools", "dump_rollout_program.hip"), tmp_path / "dump_rollout_program")
    assert out.returncode == 0 and out.stdout.count("\n== ") + 1 == 6 * 4 * 2 * 7
    assert hashlib.sha256(out.stdout.encode()).hexdigest() == "45988e03b89026b94ccf26e569c2a5c990ad7c33384d9cca8ba8ec0a18e11104"
    heads = subprocess.run([str(tmp_path / "dump_rollout_program"), "--heads"], capture_output=True, text=True, timeout=300).stdout
    assert heads.startswith(out.stdout) and heads.count(" head 1\n") == heads.count(" head 2\n") == 16


def test_scratch_sizes_follow_the_head():
    lib = _hip.load()
    args = (7, 5, 6, 32, 16, 64)
    for old, new in ((lib.blvm_vrnn_generate_scratch_floats, lib.blvm_vrnn_generate_scratch_floats_head),
                     (lib.blvm_srnn_generate_scratch_floats, lib.blvm_srnn_generate_scratch_floats_head)):  # fmt: skip
        assert new(*args, 0) == new(*args, 1) == old(*args) > 0
        assert 0 < new(*args, 2) < new(*args, 0)  # F = 2: the last layer and its slabs are narrower
        assert new(*args, 3) == new(*args, -1) == 0 and new(0, *args[1:], 1) == 0
        # S = 6: Np = 16 ceil(6 F / 16): 192 against 16 — the weight copy [Np,H] twice (pack + stage), the bias stage and T slabs [B,Np]
        assert new(*args, 0) - new(*args, 2) == (192 - 16) * (2 * 32 + 1 + 7 * 5)
    assert lib.blvm_vrnn_decode_applies(16, 32, 16, 64) == 1 and lib.blvm_vrnn_decode_applies(64, 256, 256, 512) == 1
    assert lib.blvm_vrnn_decode_applies(6, 32, 16, 64) == 0 and lib.blvm_vrnn_decode_applies(16, 32, 16, 4096) == 0 and lib.blvm_vrnn_decode_applies(160, 32, 16, 64) == 0


REFUSALS = [
    (dict(kind=3), "unknown head kind"),
    (dict(kind=-1), "unknown head kind"),
    (dict(kind=0, num_mix=5), "10 components"),
    (dict(kind=1, num_mix=5), "10 components"),
    (dict(kind=1, sd_beta=-1.0), "must not be negative"),
    (dict(kind=2, sd_beta=-0.5), "must not be negative"),
    (dict(kind=2, u=True), "takes no u"),
    (dict(kind=1, u=True, v=False), "given together"),
]


@pytest.mark.parametrize("entry", ["vrnn_generate", "srnn_generate", "vrnn_decode"])
@pytest.mark.parametrize("how,message", REFUSALS, ids=[m + str(i) for i, (_, m) in enumerate(REFUSALS)])
def test_head_entry_points_refuse_before_they_touch_a_buffer(entry, how, message):
    """Every refusal of the *_head entry points is host arithmetic in front of the first launch or write: it can be shown without a
    device, with host arrays in the place of the buffers, which keep their planted values.  Kind 2 on the per-CU form is refused too."""
    lib = _hip.load()
    H, Z, R, S, B, T_ = 32, 16, 64, 16, 3, 2
    if entry == "vrnn_decode" and message == "takes no u":
        message = "not the Gaussian head"  # (refused there as a kind, in front of the check of its streams)
    planted = np.full(4096, 7.25, dtype=np.float32)
    bufs = {k: planted.copy() for k in ("x0", "eps", "u", "v", "x_out", "s_out", "z_out", "scratch")}
    p = lambda k: bufs[k].ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    scratch = ctypes.c_void_p((bufs["scratch"].ctypes.data + 15) & ~15)
    u = p("u") if how.get("u", how.get("kind") != 2) else None
    v = p("v") if how.get("v", True) else None
    head = (how["kind"], how.get("num_mix", 10), -7.0, how.get("sd_beta", 0.69), 1e-4)
    if entry == "srnn_generate":
        w, cw = _hip.SrnnDecodeWeights(), _hip.SrnnWeights()
        w.chain = ctypes.pointer(cw)
        rc = lib.blvm_srnn_generate_head(ctypes.byref(w), p("x0"), None, None, p("eps"), u, v, T_, B, S, H, Z, R, *head, 1e-6, 0.01, p("x_out"), p("s_out"),
                                         p("z_out"), scratch, None)  # fmt: skip
    else:
        w, cw = _hip.VrnnDecodeWeights(), _hip.VrnnWeights()
        w.cell = ctypes.pointer(cw)
        fn = lib.blvm_vrnn_generate_head if entry == "vrnn_generate" else lib.blvm_vrnn_decode_head
        rc = fn(ctypes.byref(w), p("x0"), None, p("eps"), u, v, T_, B, S, H, Z, R, *head, 1e-6, 0.01, p("x_out"), p("s_out"), scratch, None)
    assert rc == _hip.CONSTANTS["BLVM_EINVAL"]
    assert message in lib.blvm_last_error().decode(), lib.blvm_last_error().decode()
    assert all(np.array_equal(b, planted) for b in bufs.values())


def test_per_cu_form_refuses_the_gaussian_head():
    lib = _hip.load()
    w, cw = _hip.VrnnDecodeWeights(), _hip.VrnnWeights()
    w.cell = ctypes.pointer(cw)
    a = np.zeros(64, dtype=np.float32)
    q = a.ctypes.data_as(ctypes.c_void_p)
    s = ctypes.c_void_p((a.ctypes.data + 15) & ~15)
    assert lib.blvm_vrnn_decode_head(ctypes.byref(w), q, None, q, None, q, 2, 3, 16, 32, 16, 64, 2, 0, 0.0, 0.69, 1e-4, 1e-6, 0.01, q, q, s, None) == _hip.CONSTANTS["BLVM_EINVAL"]
    assert "not the Gaussian head (kind 2)" in lib.blvm_last_error().decode()


def test_head_value_types_map_to_the_five_scalars():
    assert ops._head_scalars(ops.DmolHead(10, -7.0)) == (0, 10, -7.0, 0.0, 0.0)
    assert ops._head_scalars(ops.GmmHead(10, 0.5, 1e-4)) == (1, 10, 0.0, 0.5, 1e-4)
    assert ops._head_scalars(ops.GaussHead(0.5, 1e-4)) == (2, 0, 0.0, 0.5, 1e-4)
    with pytest.raises(TypeError):
        ops._head_scalars((1, 10))


def test_gaussian_head_sample_takes_given_noise_and_is_unchanged_without():
    from blvm.modules.distributions import DiagonalGaussianDense, DiagonalGaussianMixtureDense, gauss_rollout_head

    lik = DiagonalGaussianDense(x_dim=2, y_dim=1, epsilon=1e-4)
    g = torch.Generator().manual_seed(0)
    mu, sd, n = torch.randn(3, 6, 1, generator=g), torch.rand(3, 6, 1, generator=g) + 0.1, torch.randn(3, 6, 1, generator=g)
    assert torch.equal(lik.sample((mu, sd), noise=n), mu + sd * n) and torch.equal(lik.sample((mu, sd), noise=n.reshape(3, 6)), mu + sd * n)
    torch.manual_seed(3)
    a = lik.sample((mu, sd))
    torch.manual_seed(3)
    assert torch.equal(a, mu + sd * torch.randn_like(mu))  # today's call: the same draw from the same RNG state
    assert gauss_rollout_head(lik) == ops.GaussHead(lik.softplus_beta, 1e-4)
    gm = DiagonalGaussianMixtureDense(x_dim=30, y_dim=1, num_mix=10, initial_sd=1, epsilon=1e-4)
    assert gauss_rollout_head(gm) == ops.GmmHead(10, gm.softplus_beta, 1e-4) and gauss_rollout_head(torch.nn.Linear(2, 2)) is None
    assert (gm.softplus_beta, lik.softplus_beta) == (G.head_constants(G.GMM)[0], G.head_constants(G.GAUSS)[0])
