"""GPU (MI355X): `iw_bound` of the four latent-variable models (K-sample importance-weighted bound, K8m).

Shapes: the smallest the existing model tests use with every width a multiple of 16, B = 3 utterances of unequal lengths, a few
latent steps, K = 4 particles with the noise given.

log_w[k] against a float64 recomputation with the CPU oracle (oracle/blvm_oracle.py), to the tolerance the model's existing parity
test applies to `elbo`:
  vrnn            oracle route: `vrnn_audio_forward` (log_prob) + `vrnn_cell_step` (moments, z), log-ratio in float64 here;
                  tests/test_gpu_parity.py::test_vrnn_vs_oracle_ragged_with_initial_state, rtol 1e-5, atol 1e-3
  stcn_bottom_up  oracle route: `stcn_forward(top_down=False)`, whose KL IS the Monte-Carlo log-ratio at the drawn z;
                  tests/test_gpu_stcn.py::test_stcn_small_matches_reference, rtol 1e-4
  srnn            fallback (the oracle does not hand out the moments): tests/test_gpu_parity.py::test_srnn_small_vs_reference_golden,
                  rtol 1e-5, atol 1e-3
  stcn            fallback (top-down: the oracle has the analytic KL only): test_stcn_small_matches_reference, rtol 1e-4
  cwvae, cwvae_resets  fallback: tests/test_gpu_cwvae.py::test_cwvae_small_matches_reference, rtol 1e-4
Fallback route: log p(x | z_k) = log_w[k] + sum of the log-ratio sums the model used is compared with `forward(eps=eps[k]).log_prob`
at that tolerance, and the log-ratio part is pinned on the tensors the model handed to `ops.gauss_log_ratio_sums` (a recording
wrapper): each recorded sum against the formula in float64 on those tensors within K8's bar (64 u sum |r|), the recorded z equal
to mu_q + sd_q eps, and the recorded noise equal to the given eps in particle-major rows.  Every model takes these checks, the
oracle-route ones too."""
import math

import numpy as np
import pytest
import torch

import blvm_oracle as O
from blvm import _hip, ops
from blvm.models import CWVAEAudio, SRNNAudio, STCN, VRNNAudio

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0**-24
K, B = 4, 3
CW_SMALL = dict(z_size=[32, 16, 16], h_size=16, strides=[4, 2, 2], num_level_layers=2, stride_per_layer=2, likelihood="DMoL",
                num_mix=10, num_bins=2**16, precision_posterior=True)  # fmt: skip
ST_SMALL = dict(likelihood="DMoL", n_layers=3, latent_size=[16, 16, 32], res_channels=16, n_stack_frames=8)
NAMES = ["vrnn", "srnn", "stcn", "stcn_bottom_up", "cwvae", "cwvae_resets"]
TOL = dict(vrnn=(1e-5, 1e-3), srnn=(1e-5, 1e-3), stcn=(1e-4, 0.0), stcn_bottom_up=(1e-4, 0.0), cwvae=(1e-4, 0.0), cwvae_resets=(1e-4, 0.0))


@pytest.fixture(scope="module", autouse=True)
def _require_hip():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert _hip.load().blvm_device_ok() == 1


def T(a):
    return torch.from_numpy(np.asarray(a))


def noise(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def build(name):
    """(model on the CPU, x [B,T], x_sl, eps with the particle axis in front)."""
    torch.manual_seed(11)
    if name == "vrnn":
        m = VRNNAudio(likelihood="DMoL", input_size=16, hidden_size=48, latent_size=32, residual_posterior=True)
        x, x_sl = O.synth_batch(B, 16 * 5 - 3, seed=9, ragged=True)
        return m, x, x_sl, noise((K, 5, B, 32), 1)
    if name == "srnn":
        m = SRNNAudio(likelihood="DMoL", input_size=16, hidden_size=32, latent_size=16, residual_posterior=True)
        x, x_sl = O.synth_batch(B, 16 * 5 - 3, seed=9, ragged=True)
        return m, x, x_sl, noise((K, 5, B, 16), 2)
    if name.startswith("stcn"):
        m = STCN(**ST_SMALL, top_down=name == "stcn")
        if name == "stcn":
            g = np.load(f"{GOLDEN}/stcn.npz")
            m.load_state_dict({k[len("s8_sd."):]: T(g[k]) for k in g.files if k.startswith("s8_sd.")})
        x, x_sl = O.synth_batch(B, 8 * 6, seed=5, ragged=True)
        return m, x, x_sl, [noise((K, 6, B, z), 10 + l) for l, z in enumerate(ST_SMALL["latent_size"])]
    m = CWVAEAudio(**CW_SMALL)
    g = np.load(f"{GOLDEN}/cwvae.npz")
    m.load_state_dict({k[len("pw_sd."):]: T(g[k]) for k in g.files if k.startswith("pw_sd.")})
    m.cwvae.with_resets = name == "cwvae_resets"
    x, x_sl = O.synth_batch(B, 64, seed=7, ragged=True)
    return m, x, x_sl, [noise((K, 64 // s, B, z), 20 + l) for l, (s, z) in enumerate(zip((4, 8, 16), CW_SMALL["z_size"]))]


def particle(eps, k):
    return [e[k] for e in eps] if isinstance(eps, list) else eps[k]


def to_dev(e):
    return [t.to(DEV) for t in e] if isinstance(e, list) else e.to(DEV)


_RUNS = {}


def run(name):
    """One iw_bound(K = 4, eps given, default max_rows: one pass of K * B rows) per model, shared by the tests; the arguments and
    results of every `ops.gauss_log_ratio_sums` call it made are recorded."""
    if name in _RUNS:
        return _RUNS[name]
    m, x, x_sl, eps = build(name)
    assert len(set(x_sl.tolist())) == B, x_sl
    sd64 = {k: v.double().clone() for k, v in m.state_dict().items()}
    m = m.to(DEV).eval()
    calls, real = [], ops.gauss_log_ratio_sums

    def recording(*a):
        out = real(*a)
        calls.append((a, out))
        return out

    ops.gauss_log_ratio_sums = recording
    try:
        bound, metrics, out = m.iw_bound(x.to(DEV), x_sl, K, eps=to_dev(eps))
    finally:
        ops.gauss_log_ratio_sums = real
    _RUNS[name] = dict(m=m, x=x, x_sl=x_sl, eps=eps, sd64=sd64, bound=bound, metrics=metrics, out=out, calls=calls)
    return _RUNS[name]


def ratio64(sd_q, mu_p, sd_p, z, e):
    return sd_p.log() - sd_q.log() - 0.5 * e * e + 0.5 * ((z - mu_p) / sd_p) ** 2


def oracle_log_w(name, r, k):
    """log_w[k] recomputed in float64 by the CPU oracle, or None where the oracle does not hand out what it takes."""
    x, x_sl, sd64 = r["x"].double(), r["x_sl"], r["sd64"]
    if name == "vrnn":
        e = r["eps"][k].double()
        o = O.vrnn_audio_forward(sd64, x, x_sl, e, stack=16)
        Tp = e.shape[0]
        stride = math.ceil(x.shape[1] / Tp)
        h, ratio = torch.zeros(B, 96, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
        for t in range(Tp):
            h, c = O.vrnn_cell_step(sd64, o["enc"][:, t], h, e[t], True)
            ratio += ratio64(c["sd_q"], c["mu_p"], c["sd_p"], c["z"], e[t]).sum(-1) * (t * stride < x_sl)
        return o["log_prob"] - ratio
    if name == "stcn_bottom_up":
        o = O.stcn_forward(sd64, x, x_sl, [e[k].transpose(0, 1).double() for e in r["eps"]], n_layers=3, latent_size=ST_SMALL["latent_size"],
                           n_stack_frames=8, top_down=False)  # fmt: skip
        return o["log_prob"] - o["kld"]
    return None


@pytest.mark.parametrize("name", NAMES)
def test_log_w_vs_float64_recomputation(name):
    r = run(name)
    log_w, (rtol, atol) = r["out"].log_w, TOL[name]
    assert log_w.dtype == torch.float64 and log_w.shape == (K, B) and bool(torch.isfinite(log_w).all())
    for k in range(K):
        truth = oracle_log_w(name, r, k)
        if truth is not None:
            print(f"{name} particle {k}: log_w {log_w[k].tolist()} oracle {truth.tolist()}")
            torch.testing.assert_close(log_w[k].cpu(), truth.detach(), rtol=rtol, atol=atol)
    # the log-ratio part on the tensors the model passed (every model: it is the fallback's pin and costs the others nothing)
    calls = r["calls"]
    assert calls, "iw_bound did not go through ops.gauss_log_ratio_sums"
    total = torch.zeros(K * B, dtype=torch.float64)
    for (mu_q, sd_q, mu_p, sd_p, z, e, sl, layout, n, Tp, Z, stride), got in calls:
        assert layout == ops.LAYOUT_TIME_MAJOR and got.shape == (n,)
        sq, mp, sp, zz, ee, mq = (t.detach().double().cpu().reshape(Tp, n, Z) for t in (sd_q, mu_p, sd_p, z, e, mu_q))
        torch.testing.assert_close(zz, mq + sq * ee, rtol=1e-6, atol=1e-6)  # z is the draw from (mu_q, sd_q) with this noise
        live = (torch.arange(Tp).unsqueeze(1) * stride < sl.cpu().unsqueeze(0)).double().unsqueeze(-1)
        el = ratio64(sq, mp, sp, zz, ee) * live
        truth, bar = el.sum((0, 2)), 64 * U * el.abs().sum((0, 2))
        assert bool(((got.cpu() - truth).abs() <= bar).all()), (name, (got.cpu() - truth).abs().tolist(), bar.tolist())
        if n == K * B:
            total += got.cpu()
        else:  # CW-VAE with resets: rows are (segment, particle, utterance); the model folds the segments
            total += got.cpu().view(-1, K * B).sum(0)
    if name in ("vrnn", "srnn"):  # the recorded noise is the given eps, rows particle-major
        e_given = r["eps"].permute(1, 0, 2, 3).reshape(r["eps"].shape[1], K * B, -1)
        assert torch.equal(calls[0][0][5].cpu().reshape(e_given.shape), e_given)
    # log p(x | z_k) = log_w + the log-ratio sums, against forward on the same noise
    log_prob_iw = log_w.cpu() + total.view(K, B)
    with torch.no_grad():
        for k in range(K):
            _, _, fo = r["m"](r["x"].to(DEV), r["x_sl"], eps=to_dev(particle(r["eps"], k)))
            torch.testing.assert_close(log_prob_iw[k], fo.log_prob.double().cpu(), rtol=rtol, atol=atol)


@pytest.mark.parametrize("name", NAMES)
def test_bound_reduction_metrics(name):
    r = run(name)
    out, bound = r["out"], r["bound"]
    b2, e2 = ops.iw_reduce(out.log_w)
    assert torch.equal(bound.view(torch.int64), b2.view(torch.int64)) and torch.equal(out.ess.view(torch.int64), e2.view(torch.int64))
    assert bound.dtype == torch.float64 and bound.shape == (B,)
    assert bool((bound >= out.elbo_mc - 1e-9 * out.elbo_mc.abs()).all()), (bound, out.elbo_mc)  # Jensen
    torch.testing.assert_close(out.elbo_mc, out.log_w.mean(0), rtol=1e-15, atol=0)
    assert bool((out.ess >= 1 - 1e-12).all()) and bool((out.ess <= K + 1e-9).all())
    vals = {mm.name: mm.value for mm in r["metrics"]}
    n_frames = float(r["x_sl"].sum())
    assert set(vals) == {f"iw-{K} (nats)", f"iw-{K} (bpt)", f"iw-{K} ess"}
    assert vals[f"iw-{K} (nats)"] == pytest.approx(float(bound.sum()) / B, rel=1e-12)
    assert vals[f"iw-{K} (bpt)"] == pytest.approx(-float(bound.sum()) / math.log(2) / n_frames, rel=1e-12)
    assert vals[f"iw-{K} ess"] == pytest.approx(float(out.ess.mean()), rel=1e-12)


@pytest.mark.parametrize("name", NAMES)
def test_chunking_agrees(name):
    r = run(name)
    rtol, atol = TOL[name]
    m, x, x_sl, eps = r["m"], r["x"].to(DEV), r["x_sl"], to_dev(r["eps"])
    one = m.iw_bound(x, x_sl, K, eps=eps, max_rows=B)[2].log_w  # one particle per pass
    all_ = m.iw_bound(x, x_sl, K, eps=eps, max_rows=K * B)[2].log_w  # one pass
    mid = m.iw_bound(x, x_sl, K, eps=eps, max_rows=3 * B)[2].log_w  # passes of 3 and 1 particles
    print(f"{name}: chunked vs one pass bit-identical: {torch.equal(one, all_)}, max |diff| {float((one - all_).abs().max()):.3e}")
    torch.testing.assert_close(one, all_, rtol=rtol, atol=atol)
    torch.testing.assert_close(mid, all_, rtol=rtol, atol=atol)
    assert torch.equal(all_, r["out"].log_w)  # the default max_rows is one pass here, and calls repeat bit for bit


def counters():
    lib = _hip.load()
    g, n, s = (torch.zeros(17, dtype=torch.int64), torch.zeros(12, dtype=torch.int64), torch.zeros(6, dtype=torch.int64))
    import ctypes

    for fn, t in ((lib.blvm_gemm_arm_counts, g), (lib.blvm_rnn_path_counts, n), (lib.blvm_rssm_path_counts, s)):
        fn(ctypes.c_void_p(t.data_ptr()))
    return dict(gemm=int(g.sum()), gru_fwd=int(n[6:9].sum()), rssm_fwd=int(s[0:2].sum()))


def delta(fn):
    c0 = counters()
    fn()
    c1 = counters()
    return {k: c1[k] - c0[k] for k in c0}


@pytest.mark.parametrize("name", NAMES)
def test_deterministic_part_runs_once(name):
    """At max_rows = B every particle is a pass of its own: whatever a pass launches is launched K times, the deterministic part
    once.  With E the GEMM launches of the deterministic part alone, gemm(K) = E + K * per_pass."""
    r = run(name)
    m, x, x_sl, eps = r["m"], r["x"].to(DEV), r["x_sl"], to_dev(r["eps"])
    first = lambda e: [t[:1] for t in e] if isinstance(e, list) else e[:1]  # noqa: E731
    with torch.no_grad():
        if name == "vrnn":
            S, enc_lin, _, _ = m.vrnn._plan()
            det = delta(lambda: m.vrnn._encode(x, x_sl, S, enc_lin))
        elif name == "srnn":
            S, enc_lin, _, _ = m.srnn._plan()
            det = delta(lambda: m.srnn._deterministic(x, x_sl, None, None, S, enc_lin))
        elif name.startswith("stcn"):
            det = delta(lambda: m._front(x, x_sl, None, True))
        else:
            det = delta(lambda: m.cwvae._front(x, x_sl, None, False, True))
    d1 = delta(lambda: m.iw_bound(x, x_sl, 1, eps=first(eps), max_rows=B))
    d4 = delta(lambda: m.iw_bound(x, x_sl, K, eps=eps, max_rows=B))
    print(f"{name}: deterministic part {det}, iw_bound K=1 {d1}, K={K} {d4}")
    per_pass = d1["gemm"] - det["gemm"]
    assert per_pass >= 0 and d4["gemm"] == det["gemm"] + K * per_pass, (det, d1, d4)
    if name in ("vrnn", "srnn", "cwvae", "cwvae_resets"):
        assert det["gemm"] > 0  # the encoder's launches are counted, and they are not repeated
    if name == "srnn":  # the two GRU sequences (d, a): once per call
        assert det["gru_fwd"] == 2 and d1["gru_fwd"] == 2 and d4["gru_fwd"] == 2, (det, d1, d4)
    if name.startswith("cwvae"):  # one cell sequence per level and pass
        assert det["rssm_fwd"] == 0 and d1["rssm_fwd"] == 3 and d4["rssm_fwd"] == 3 * K, (det, d1, d4)


@pytest.mark.parametrize("name", ["vrnn", "srnn", "stcn", "cwvae"])
def test_cpu_tensors_are_refused(name):
    m, x, x_sl, eps = build(name)
    with pytest.raises(_hip.BlvmHipError):
        m.iw_bound(x, x_sl, 2, eps=first2(eps))
    with pytest.raises(ValueError):
        run(name)["m"].iw_bound(x.to(DEV), x_sl, 0)


def first2(e):
    return [t[:2] for t in e] if isinstance(e, list) else e[:2]


def test_noise_drawn_on_the_device_and_operand_dtype_restored():
    r = run("vrnn")
    _hip.set_operand_dtype("bf16")
    try:
        torch.manual_seed(3)
        bound, _, out = r["m"].iw_bound(r["x"].to(DEV), r["x_sl"], K)
        assert _hip.get_operand_dtype() == "bf16"
    finally:
        _hip.set_operand_dtype("f32")
    assert bool(torch.isfinite(bound).all()) and out.log_w.shape == (K, B)
    # fp32 operands inside: the same seed under the fp32 mode draws the same noise and gives the same bits
    torch.manual_seed(3)
    bound2, _, _ = r["m"].iw_bound(r["x"].to(DEV), r["x_sl"], K)
    assert torch.equal(bound, bound2)
