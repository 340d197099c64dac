"""CPU: the oracle (oracle/blvm_oracle.py) against golden vectors produced by the imported reference
(oracle/gen_golden.py) and against the reference's own known-answer tests."""
import os

import numpy as np
import pytest
import torch

import blvm_oracle as O

from conftest import GOLDEN


def T(a):
    return torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def fn():
    return np.load(os.path.join(GOLDEN, "functions.npz"))


def close(a, b, rtol=1e-6, atol=1e-6):
    torch.testing.assert_close(a, T(b) if not isinstance(b, torch.Tensor) else b, rtol=rtol, atol=atol)


def test_dmol_ll(fn):
    y, lg, lc, ls = T(fn["dmol_y"]), T(fn["dmol_logits"]), T(fn["dmol_locs"]), T(fn["dmol_ls"])
    close(O.dmol_ll(y, lg, lc, ls, 2**16), fn["dmol_ll_65536"], 1e-6, 1e-6)
    close(O.dmol_ll(y, lg, lc, ls, 256), fn["dmol_ll_256"], 1e-6, 1e-6)


def test_dmol_head(fn):
    lg, lc, ls = O.dmol_head(T(fn["dmolhead_x"]), T(fn["dmolhead_w"]), T(fn["dmolhead_b"]))
    close(lg, fn["dmolhead_logits"])
    close(lc, fn["dmolhead_locs"])
    close(ls, fn["dmolhead_ls"])
    assert float(ls.min()) >= -7.0
    close(O.dmol_mode(lg, lc), fn["dmolhead_mode"])


def test_gaussian_head(fn):
    mu, sd = O.gaussian_head(T(fn["ghead_x"]), T(fn["ghead_w"]), T(fn["ghead_b"]))
    close(mu, fn["ghead_mu"])
    close(sd, fn["ghead_sd"])


def test_gaussian_lls(fn):
    close(O.gaussian_ll(T(fn["gll_y"]), T(fn["gll_mu"]), T(fn["gll_sd"]), epsilon=0), fn["gll_eps0"])
    close(O.gaussian_mixture_ll(T(fn["gmm_y"]), T(fn["gmm_logits"]), T(fn["gmm_mu"]), T(fn["gmm_sd"]), 1e-4), fn["gmm_ll"], 1e-5, 1e-5)


def test_kl_freenats_precision(fn):
    mq, sq, mp, sp = (T(fn[k]) for k in ("kl_mq", "kl_sq", "kl_mp", "kl_sp"))
    kl = O.kl_gaussian(mq, sq, mp, sp)
    close(kl, fn["kl_out"], 1e-6, 1e-5)
    close(O.discount_free_nats(T(fn["kl_out"]), 2.0), fn["kl_fn2"])
    close(O.discount_free_nats(T(fn["kl_out"]), 0), fn["kl_fn0"])
    mu, sd = O.precision_weighted_gaussian(mq, sq, mp, sp)
    close(mu, fn["pw_mu"], 1e-6, 1e-6)
    close(sd, fn["pw_sd"], 1e-6, 1e-6)


def test_stack_mask_reverse(fn):
    st, pad = O.stack_tensor(T(fn["stack_x"]), 8)
    close(st, fn["stack_out"], 0, 0)
    assert pad == int(fn["stack_pad"])
    sl = T(fn["mask_sl"])
    assert torch.equal(O.sequence_mask(sl), T(fn["mask_bool"]))
    assert torch.equal(O.sequence_mask(sl, dtype=torch.float64), T(fn["mask_f64"]))
    close(O.reverse_sequences(T(fn["rev_x"]), sl), fn["rev_out"], 0, 0)


def test_reverse_sequences_reference_known_answer():
    """Known-answer vectors of the reference's tests/utils/test_operations.py:7-48 (lengths 10,7,5,2)."""
    x_sl = torch.tensor([10, 7, 5, 2])
    x = torch.zeros(10, 4)
    for b, n in enumerate(x_sl.tolist()):
        x[:n, b] = torch.arange(1, n + 1, dtype=torch.float32)
    out = O.reverse_sequences(x, x_sl)
    for b, n in enumerate(x_sl.tolist()):
        assert out[:n, b].tolist() == list(range(n, 0, -1))
        assert out[n:, b].abs().sum() == 0


def test_mulaw_and_annealer(fn):
    u = T(fn["mulaw_u"])
    close(O.mu_law_encode(u, 16), fn["mulaw_16"])
    close(O.mu_law_encode(u, 8), fn["mulaw_8"])
    np.testing.assert_allclose(O.cosine_anneal_trace(15, 10, 0, 0.0, 1.0), fn["anneal_beta"], rtol=0, atol=1e-15)
    np.testing.assert_allclose(O.cosine_anneal_trace(15, 7, 5, 2.0, 0.0), fn["anneal_fn"], rtol=0, atol=1e-15)


@pytest.mark.parametrize("tag,beta,fn_", [("a", 1.0, 2.0), ("b", 0.3, 0.0)])
def test_vrnn_small_forward_backward(tag, beta, fn_):
    g = np.load(os.path.join(GOLDEN, "vrnn_small.npz"))
    sd = {k[3:]: T(g[k]).clone().requires_grad_(True) for k in g.files if k.startswith("sd.")}
    x, x_sl, eps = T(g["x"]), T(g["x_sl"]), T(g[f"{tag}_eps"])
    out = O.vrnn_audio_forward(sd, x, x_sl, eps, beta=beta, free_nats=fn_, stack=8)
    assert out["loss"].dtype == torch.float64
    close(out["z"], g[f"{tag}_z"], 1e-5, 1e-6)
    close(out["loss"], g[f"{tag}_loss"], 1e-7, 0)
    close(out["elbo"], g[f"{tag}_elbo"], 1e-7, 0)
    close(out["log_prob"], g[f"{tag}_log_prob"], 1e-7, 0)
    close(out["kl"], g[f"{tag}_kl"], 1e-6, 1e-6)
    close(out["h_n"], g[f"{tag}_h_n"], 1e-5, 1e-6)
    m = O.vrnn_metrics(out, x_sl, beta, fn_)
    for name, val in zip(g[f"{tag}_metric_names"].tolist(), g[f"{tag}_metric_values"].tolist()):
        assert m[name] == pytest.approx(val, rel=1e-6, abs=1e-9), name
    out["loss"].backward()
    for k, p in sd.items():
        ref = T(g[f"{tag}_grad.{k}"])
        err = (p.grad - ref).norm() / (ref.norm() + 1e-12)
        assert err < 2e-5, (k, float(err))


def test_lstm_small_forward_backward():
    g = np.load(os.path.join(GOLDEN, "lstm.npz"))
    sd = {k[5:]: T(g[k]).clone().requires_grad_(True) for k in g.files if k.startswith("s_sd.")}
    x, x_sl = T(g["s_x"]), T(g["s_x_sl"])
    out = O.lstm_audio_forward(sd, x, x_sl, stack=8, num_bins=2**16)
    assert out["loss"].dtype == torch.float32  # fp32 sums for LSTM
    close(out["loss"], g["s_loss"], 1e-6, 0)
    close(out["ll"], g["s_ll"], 1e-6, 1e-4)
    close(out["z"], g["s_z"], 1e-5, 1e-6)
    close(out["h_n"], g["s_hn"][0], 1e-5, 1e-6)
    close(out["c_n"], g["s_cn"][0], 1e-5, 1e-6)
    out["loss"].backward()
    for k, p in sd.items():
        ref = T(g[f"s_grad.{k}"])
        assert (p.grad - ref).norm() / (ref.norm() + 1e-12) < 2e-5, k


@pytest.mark.parametrize("tag,smoothing,beta,fn_", [("sm", True, 1.0, 2.0), ("ns", False, 0.5, 0.0)])
def test_srnn_small_forward_backward(tag, smoothing, beta, fn_):
    g = np.load(os.path.join(GOLDEN, "srnn.npz"))
    pre = f"{tag}_sd."
    sd = {k[len(pre):]: T(g[k]).clone().requires_grad_(True) for k in g.files if k.startswith(pre)}
    x, x_sl, eps = T(g["x"]), T(g["x_sl"]), T(g[f"{tag}_eps"])
    out = O.srnn_audio_forward(sd, x, x_sl, eps, beta=beta, free_nats=fn_, stack=8, smoothing=smoothing)
    close(out["z"], g[f"{tag}_z"], 1e-5, 1e-6)
    close(out["loss"], g[f"{tag}_loss"], 1e-7, 0)
    close(out["elbo"], g[f"{tag}_elbo"], 1e-7, 0)
    close(out["kl"], g[f"{tag}_kl"], 1e-6, 1e-6)  # raw KL
    close(out["d_n"], g[f"{tag}_d_n"][0], 1e-5, 1e-6)
    close(out["z_n"], g[f"{tag}_z_n"], 1e-5, 1e-6)
    if smoothing:
        close(out["a_n"], g[f"{tag}_a_n"][0], 1e-5, 1e-6)
    out["loss"].backward()
    for k, p in sd.items():
        ref = T(g[f"{tag}_grad.{k}"])
        assert (p.grad - ref).norm() / (ref.norm() + 1e-12) < 2e-5, k
    if smoothing:  # carried states of a second split
        sd2 = {k: v.detach() for k, v in sd.items()}
        out2 = O.srnn_audio_forward(sd2, x, x_sl, T(g["c_eps"]), beta=beta, free_nats=fn_, stack=8, d_0=out["d_n"].detach(),
                                    a_0=out["a_n"].detach(), z_0=out["z_n"].detach())
        close(out2["loss"], g["c_loss"], 1e-6, 0)
        close(out2["z"], g["c_z"], 1e-5, 1e-6)


@pytest.mark.parametrize("tag,pad_rf", [("s", True), ("n", False)])
def test_wavenet_small_forward_backward(tag, pad_rf):
    g = np.load(os.path.join(GOLDEN, "wavenet.npz"))
    sd = {k[5:]: T(g[k]).clone().requires_grad_(True) for k in g.files if k.startswith("s_sd.")}
    x = T(g["s_x"]).clone().requires_grad_(True)
    out = O.wavenet_forward(sd, x, T(g["s_x_sl"]), n_layers=3, n_stacks=2, pad_receptive_field=pad_rf)
    close(out["loss"], g[f"{tag}_loss"], 1e-6, 0)
    close(out["log_prob"], g[f"{tag}_log_prob"], 1e-6, 1e-4)
    close(out["log_prob_twise"], g[f"{tag}_ll_twise"], 1e-5, 1e-5)
    out["loss"].backward()
    close(x.grad, g[f"{tag}_dx"], 1e-4, 1e-7)
    for k, p in sd.items():
        ref = T(g[f"{tag}_grad.{k}"])
        assert (p.grad - ref).norm() / (ref.norm() + 1e-12) < 2e-5, k


@pytest.mark.parametrize("tag,kw,c_dim", [("plain", {}, 48), ("res", dict(residual_posterior=True), 48),
                                          ("prec", dict(precision_posterior=True), 48), ("top", dict(precision_posterior=True), 0)])
def test_rssm_cell_sequence(tag, kw, c_dim):
    g = np.load(os.path.join(GOLDEN, "rssm.npz"))
    pre = f"{tag}_sd."
    sd = {k[len(pre):]: T(g[k]).clone().requires_grad_(True) for k in g.files if k.startswith(pre)}
    enc, ctx = T(g["enc"]).clone().requires_grad_(True), T(g["ctx"])[..., :c_dim].clone().requires_grad_(True)
    z0, h0 = T(g["z0"]).clone().requires_grad_(True), T(g["h0"]).clone().requires_grad_(True)
    zs, hs, d = O.rssm_sequence(sd, enc, ctx, (z0, h0), T(g[f"{tag}_eps"]), **kw)
    close(zs, g[f"{tag}_zs"], 1e-5, 1e-6)
    close(hs, g[f"{tag}_hs"], 1e-5, 1e-6)
    kl = O.kl_gaussian(d["enc_mu"], d["enc_sd"], d["prior_mu"], d["prior_sd"])
    loss = (zs * T(g["wz"])).sum() + (hs * T(g["wh"])).sum() + 0.7 * kl.sum()
    close(loss, g[f"{tag}_loss"], 1e-5, 1e-4)
    loss.backward()
    close(enc.grad, g[f"{tag}_d_enc"], 1e-4, 1e-6)
    close(z0.grad, g[f"{tag}_d_z0"], 1e-4, 1e-6)
    close(h0.grad, g[f"{tag}_d_h0"], 1e-4, 1e-6)
    for k, p in sd.items():
        ref = T(g[f"{tag}_grad.{k}"])
        assert (p.grad - ref).norm() / (ref.norm() + 1e-12) < 2e-5, k


CW_SMALL = dict(strides=[4, 2, 2], num_level_layers=2, stride_per_layer=2, num_bins=2**16)


def test_cwvae_with_resets_forward_backward():
    """The oracle's with_resets branch (clockwork_vae.py:273-275) pinned by the reference's outputs (cwvae_resets.npz): latents,
    carried states, loss / ELBO / KL in fp32, and in float64 the gradients within the reference's own fp32 noise."""
    g = np.load(os.path.join(GOLDEN, "cwvae_resets.npz"))
    sd = {k[3:]: T(g[k]).clone() for k in g.files if k.startswith("sd.")}
    x, x_sl = T(g["x"]), T(g["x_sl"])
    eps = [T(g[f"eps{l}"]) for l in range(3)]
    kw = dict(beta=1.0, free_nats=0.5, precision_posterior=True, with_resets=True, **CW_SMALL)
    out = O.cwvae_audio_forward(sd, x, x_sl, eps, **kw)
    for l in range(3):
        close(out["z"][l].transpose(0, 1), g[f"z{l}"], 1e-5, 1e-6)
        close(out["state_n"][l][0], g[f"state_z{l}"], 1e-5, 1e-6)
        close(out["state_n"][l][1], g[f"state_h{l}"], 1e-5, 1e-6)
    close(out["loss"], g["loss"], 2e-5, 0)
    close(out["elbo"], g["elbo"], 2e-5, 0)
    close(out["kld"], g["kld"], 1e-5, 1e-6)
    plain = O.cwvae_audio_forward(sd, x, x_sl, eps, **{**kw, "with_resets": False})
    assert abs(float(plain["loss"]) - float(g["loss"])) > 1e-3  # the flag changes the result
    sd64 = {k: v.detach().double().requires_grad_(True) for k, v in sd.items()}
    out64 = O.cwvae_audio_forward(sd64, x.double(), x_sl, [e.double() for e in eps], **kw)
    out64["loss"].backward()
    for k in sd:
        if k.startswith("cwvae.likelihood."):
            continue
        ref, truth = T(g[f"grad.{k}"]).double(), sd64[k].grad
        assert (ref - truth).norm() / (truth.norm() + 1e-12) < 1e-2, k


@pytest.mark.parametrize("tag,kw,beta,fn_", [("pw", dict(precision_posterior=True), 1.0, 0.5), ("rs", dict(residual_posterior=True), 0.7, 0.0)])
def test_cwvae_small_forward_backward(tag, kw, beta, fn_):
    g = np.load(os.path.join(GOLDEN, "cwvae.npz"))
    pre = f"{tag}_sd."
    sd = {k[len(pre):]: T(g[k]).clone().requires_grad_(True) for k in g.files if k.startswith(pre)}
    x, x_sl = T(g["x"]), T(g["x_sl"])
    eps = [T(g[f"{tag}_eps{l}"]) for l in range(3)]
    out = O.cwvae_audio_forward(sd, x, x_sl, eps, beta=beta, free_nats=fn_, **CW_SMALL, **kw)
    for l in range(3):
        close(out["z"][l].transpose(0, 1), g[f"{tag}_z{l}"], 1e-5, 1e-6)
        close(out["mus"][l][0].transpose(0, 1), g[f"{tag}_enc_mu{l}"], 1e-5, 1e-6)
        close(out["mus"][l][1].transpose(0, 1), g[f"{tag}_prior_mu{l}"], 1e-5, 1e-6)
        close(out["state_n"][l][0], g[f"{tag}_state_z{l}"], 1e-5, 1e-6)
        close(out["state_n"][l][1], g[f"{tag}_state_h{l}"], 1e-5, 1e-6)
    # fp32 reductions in a different order than the reference's ([T,B,Z] vs [B,T,Z]): a few ulp of the sums
    close(out["loss"], g[f"{tag}_loss"], 2e-5, 0)
    close(out["elbo"], g[f"{tag}_elbo"], 2e-5, 0)
    close(out["log_prob"], g[f"{tag}_log_prob"], 2e-5, 0)
    close(out["kld"], g[f"{tag}_kld"], 1e-5, 1e-6)
    # Gradients: the reference evaluates the DMoL bin mass as a difference of two fp32 sigmoids 2^-16 apart; that
    # cancellation alone moves ITS OWN gradients up to ~6e-3 (relative L2) away from a float64 evaluation on this small
    # batch, and everything upstream inherits it.  So the restatement is pinned in float64: it must sit as close to the
    # reference's fp32 gradients as that noise allows (a wrong formula shows up as >> 1e-2).
    sd64 = {k: v.detach().double().requires_grad_(True) for k, v in sd.items()}
    out64 = O.cwvae_audio_forward(sd64, x.double(), x_sl, [e.double() for e in eps], beta=beta, free_nats=fn_, **CW_SMALL, **kw)
    close(out64["loss"].float(), g[f"{tag}_loss"], 2e-6, 0)
    out64["loss"].backward()
    out["loss"].backward()
    for k, p in sd.items():
        if k.startswith("cwvae.likelihood."):  # alias of `likelihood.*` (the head is registered twice, clockwork_vae.py:458,488)
            continue
        ref, truth = T(g[f"{tag}_grad.{k}"]).double(), sd64[k].grad
        assert (ref - truth).norm() / (truth.norm() + 1e-12) < 1e-2, k
        assert (p.grad.double() - truth).norm() / (truth.norm() + 1e-12) < 1e-2, k
    if tag == "pw":  # carried per-level (z, h) state of a second call
        sd2 = {k: v.detach() for k, v in sd.items()}
        st0 = [(z.detach(), h.detach()) for z, h in out["state_n"]]
        out2 = O.cwvae_audio_forward(sd2, x, x_sl, [T(g[f"c_eps{l}"]) for l in range(3)], beta=beta, free_nats=fn_, state0=st0,
                                     **CW_SMALL, **kw)
        close(out2["loss"], g["c_loss"], 2e-5, 0)
        for l in range(3):
            close(out2["z"][l].transpose(0, 1), g[f"c_z{l}"], 1e-5, 1e-6)


@pytest.mark.parametrize("tag,S,beta,fn_", [("s8", 8, 1.0, 1.5), ("s1", 1, 0.6, 0.0)])
def test_stcn_small_forward_backward(tag, S, beta, fn_):
    g = np.load(os.path.join(GOLDEN, "stcn.npz"))
    pre = f"{tag}_sd."
    sd = {k[len(pre):]: T(g[k]).clone().requires_grad_(True) for k in g.files if k.startswith(pre)}
    x, x_sl = T(g[f"{tag}_x"]), T(g[f"{tag}_x_sl"])
    eps = [T(g[f"{tag}_eps{l}"]) for l in range(3)]
    out = O.stcn_forward(sd, x, x_sl, eps, n_layers=3, latent_size=[16, 16, 32], n_stack_frames=S, beta=beta, free_nats=fn_)
    for l in range(3):
        close(out["z"][l], g[f"{tag}_z{l}"], 1e-5, 1e-6)
        close(out["mu_q"][l], g[f"{tag}_enc_mu{l}"], 1e-5, 1e-6)
        close(out["mu_p"][l], g[f"{tag}_prior_mu{l}"], 1e-5, 1e-6)
        close(out["klds"][l], g[f"{tag}_kld{l}"], 2e-5, 1e-5)
    close(out["loss"], g[f"{tag}_loss"], 2e-5, 0)
    close(out["elbo"], g[f"{tag}_elbo"], 2e-5, 0)
    close(out["log_prob"], g[f"{tag}_log_prob"], 2e-5, 0)
    # gradients pinned in float64 (the DMoL bin-mass cancellation makes fp32 gradients of two correct evaluations differ
    # by up to ~1e-2 on small batches, see test_cwvae_small_forward_backward)
    sd64 = {k: v.detach().double().requires_grad_(True) for k, v in sd.items()}
    out64 = O.stcn_forward(sd64, x.double(), x_sl, [e.double() for e in eps], n_layers=3, latent_size=[16, 16, 32],
                           n_stack_frames=S, beta=beta, free_nats=fn_)
    out64["loss"].backward()
    nograd = set(g[f"{tag}_nograd"])
    for k, p in sd64.items():
        if k in nograd:  # skip halves of blocks whose skip connection STCN does not read: never reached by backward
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        ref = T(g[f"{tag}_grad.{k}"]).double()
        assert (ref - p.grad).norm() / (p.grad.norm() + 1e-12) < 1e-2, k


def test_stcn_bottom_up_forward_backward():
    """The oracle's bottom-up branch (each latent conditions on the one below, Monte-Carlo KL: stcn.py:165-170, 284-287, 310-316)
    pinned by the reference's outputs (stcn_bottom_up.npz)."""
    g = np.load(os.path.join(GOLDEN, "stcn_bottom_up.npz"))
    sd = {k[3:]: T(g[k]).clone() for k in g.files if k.startswith("sd.")}
    x, x_sl = T(g["x"]), T(g["x_sl"])
    eps = [T(g[f"eps{l}"]) for l in range(3)]
    kw = dict(n_layers=3, latent_size=[16, 16, 32], n_stack_frames=8, beta=0.8, free_nats=1.5, top_down=False)
    out = O.stcn_forward(sd, x, x_sl, eps, **kw)
    for l in range(3):
        close(out["z"][l], g[f"z{l}"], 1e-5, 1e-6)
        close(out["mu_q"][l], g[f"enc_mu{l}"], 1e-5, 1e-6)
        close(out["mu_p"][l], g[f"prior_mu{l}"], 1e-5, 1e-6)
        close(out["klds"][l], g[f"kld{l}"], 2e-5, 1e-4)
    close(out["loss"], g["loss"], 2e-5, 0)
    close(out["elbo"], g["elbo"], 2e-5, 0)
    sd64 = {k: v.detach().double().requires_grad_(True) for k, v in sd.items()}
    out64 = O.stcn_forward(sd64, x.double(), x_sl, [e.double() for e in eps], **kw)
    out64["loss"].backward()
    nograd = set(g["nograd"])
    for k, p in sd64.items():
        if k in nograd:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        ref = T(g[f"grad.{k}"]).double()
        assert (ref - p.grad).norm() / (p.grad.norm() + 1e-12) < 1e-2, k


def test_cwvae_generate_matches_reference():
    g = np.load(os.path.join(GOLDEN, "generate.npz"))
    sd = {k[6:]: T(g[k]) for k in g.files if k.startswith("cw_sd.")}
    eps = [T(g[f"cw_eps{l}"]) for l in range(3)]
    out = O.cwvae_audio_generate(sd, eps, 2, int(g["cw_T"][0]), [4, 2, 2], 2, 2)
    close(out["mode"], g["cw_x_mode"], 1e-5, 1e-6)


def test_vrnn_generate_matches_reference():
    g = np.load(os.path.join(GOLDEN, "generate.npz"))
    sd = {k[6:]: T(g[k]) for k in g.files if k.startswith("vr_sd.")}
    x = O.vrnn_audio_generate(sd, 3, 6, 8, T(g["vr_eps"]))
    close(x, g["vr_x"], 1e-6, 1e-7)


def test_srnn_generate_matches_reference():
    g = np.load(os.path.join(GOLDEN, "generate.npz"))
    sd = {k[6:]: T(g[k]) for k in g.files if k.startswith("sr_sd.")}
    x = O.srnn_audio_generate(sd, 3, 5, 8, T(g["sr_eps"]), list(zip(T(g["sr_u"]), T(g["sr_u2"]))))
    close(x, g["sr_x"], 1e-6, 1e-6)


def test_wavenet_generate_matches_reference():
    g = np.load(os.path.join(GOLDEN, "generate.npz"))
    sd = {k[6:]: T(g[k]) for k in g.files if k.startswith("wn_sd.")}
    x = O.wavenet_generate(sd, 2, 7, 3, 2, list(zip(T(g["wn_u"]), T(g["wn_u2"]))))
    close(x, g["wn_x"], 1e-6, 1e-6)


# ---- split evaluation: tests/golden/split_eval.npz = the reference's loops on the reference's models --------------
def _merge_like_tracker(per_split):
    from blvm.evaluation import Tracker

    tr = Tracker()
    for metrics in per_split:
        tr.update(metrics, source="test")
    return tr.values("test")


@pytest.mark.parametrize("tag", ["consume", "extend"])
def test_split_eval_wavenet_host_splits_and_oracle(tag):
    """The product's host side (`WaveNet.split_sequence`: overlap = receptive field, "extend" mode with left padding when the split
    length does not exceed it, examples dropped as they end) cuts the reference's splits; the oracle evaluated on every split
    (`forward_split`: pad_causal, receptive-field padding on split 0 only) gives the reference's loss / log-prob per split — zeros
    and sign changes of the "extend" mode included — and the product's metric objects merge to the reference tracker's values."""
    from blvm.evaluation import BitsPerDimMetric, LLMetric, LossMetric
    from blvm.models import WaveNet
    from blvm.modules.distributions import DiscretizedLogisticMixtureDense

    g = np.load(os.path.join(GOLDEN, "split_eval.npz"))
    sd = {k[6:]: T(g[k]) for k in g.files if k.startswith("wn_sd.")}
    m = WaveNet(likelihood=DiscretizedLogisticMixtureDense(16, 1, num_mix=10, num_bins=2**16), n_layers=3, n_stacks=2, res_channels=16,
                kernel_size=2, base_dilation=2, n_stack_frames=1)  # fmt: skip
    assert m.receptive_field == int(g["wn_rf"])
    xs, sls = m.split_sequence(T(g["wn_x"]), T(g["wn_x_sl"]), length=int(g[f"wn_{tag}_length"]))
    assert len(xs) == int(g[f"wn_{tag}_n"])
    per_split = []
    for i, (x_i, sl_i) in enumerate(zip(xs, sls)):
        assert torch.equal(x_i, T(g[f"wn_{tag}_x{i}"])) and torch.equal(sl_i, T(g[f"wn_{tag}_x_sl{i}"])), i
        out = O.wavenet_forward(sd, x_i, sl_i, n_layers=3, n_stacks=2, pad_causal=True, pad_receptive_field=(i == 0))
        close(out["loss"], g[f"wn_{tag}_loss{i}"], 2e-6, 1e-6)
        close(out["log_prob"], g[f"wn_{tag}_log_prob{i}"], 2e-6, 1e-4)
        close(out["log_prob_twise"], g[f"wn_{tag}_ll_twise{i}"], 1e-5, 1e-5)
        n = sl_i - (0 if i == 0 else m.receptive_field)  # forward reduces the lengths it normalises by (wavenet.py:188)
        per_split.append([LossMetric(out["loss"], weight_by=out["log_prob"].numel()), LLMetric(out["log_prob"]),
                          BitsPerDimMetric(out["log_prob"], reduce_by=n)])  # fmt: skip
        np.testing.assert_allclose([mm.value for mm in per_split[-1]], g[f"wn_{tag}_metric_values{i}"], rtol=1e-5, atol=1e-6)
    merged = _merge_like_tracker(per_split)
    assert list(merged) == list(g[f"wn_{tag}_merged_names"])
    np.testing.assert_allclose(list(merged.values()), g[f"wn_{tag}_merged_values"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("i_split", [0, 1])
def test_split_eval_stcn_oracle(i_split):
    """STCN.forward_split (stcn.py:332-342): receptive-field padding on split 0 only; on later splits the lengths are reduced by
    rf * S without a clamp (an utterance shorter than that contributes a NEGATIVE count to the normaliser: kept)."""
    g = np.load(os.path.join(GOLDEN, "split_eval.npz"))
    assert str(g["st_split_sequence_raises"]) == "NotImplementedError"
    sd = {k[6:]: T(g[k]) for k in g.files if k.startswith("st_sd.")}
    eps = [T(g[f"st_eps{i_split}_{l}"]) for l in range(3)]
    out = O.stcn_forward(sd, T(g["st_x"]), T(g["st_x_sl"]), eps, n_layers=3, latent_size=[16, 16, 32], n_stack_frames=8,
                         pad_receptive_field=(i_split == 0))  # fmt: skip
    for l in range(3):
        close(out["z"][l], g[f"st_z{i_split}_{l}"], 1e-5, 1e-6)
        close(out["klds"][l], g[f"st_kld{i_split}_{l}"], 2e-5, 1e-5)
    close(out["loss"], g[f"st_loss{i_split}"], 2e-5, 0)
    close(out["elbo"], g[f"st_elbo{i_split}"], 2e-5, 1e-5)
    close(out["log_prob"], g[f"st_log_prob{i_split}"], 2e-5, 1e-5)


def test_split_eval_cwvae_host_splits_and_single_split_oracle():
    """CWVAE.split_sequence (clockwork_vae.py:163-174: strideable length, overlap rf - stride, nobody dropped) cuts the reference's
    splits; an utterance that fits ONE split is evaluated with same padding (`is_last_split`), which the oracle reproduces.  Every
    split that is NOT the last raises IndexError in the reference (fixture: 98 of 98 probed shapes) — nothing numeric to pin there;
    the product raising the same error is a GPU test (tests/test_gpu_split_eval.py)."""
    from blvm.models import CWVAEAudio

    g = np.load(os.path.join(GOLDEN, "split_eval.npz"))
    assert list(g["cw_not_last_raises"]) == ["IndexError"] and int(g["cw_not_last_cases"]) == 98
    m = CWVAEAudio(**CW_SMALL, z_size=[32, 16, 16], h_size=16, precision_posterior=True, likelihood="DMoL", num_mix=10)
    assert m.cwvae.overall_receptive_field == int(g["cw_overall_rf"]) and m.cwvae.overall_stride == int(g["cw_overall_stride"])
    x, x_sl = T(g["cw_x"]), T(g["cw_x_sl"])
    for length in (256, 300):
        xs, sls = m.split_sequence(x, x_sl, length=length)
        assert [list(t.shape) for t in xs] == g[f"cw_split{length}_shapes"].tolist()
        assert torch.equal(torch.stack(sls), T(g[f"cw_split{length}_x_sl"]))
        assert torch.equal(torch.stack([t[:, 0] for t in xs]), T(g[f"cw_split{length}_first"]))
    xs, sls = m.split_sequence(x, x_sl, length=1024)
    assert len(xs) == 1 and torch.equal(xs[0], T(g["cw_one_x"])) and torch.equal(sls[0], T(g["cw_one_x_sl"]))
    c = np.load(os.path.join(GOLDEN, "cwvae.npz"))  # the same reduced model (same seed): its weights live in cwvae.npz
    sd = {k[6:]: T(c[k]) for k in c.files if k.startswith("pw_sd.")}
    out = O.cwvae_audio_forward(sd, xs[0], sls[0], [T(g[f"cw_one_eps{l}"]) for l in range(3)], precision_posterior=True, **CW_SMALL)
    close(out["loss"], g["cw_one_loss"], 2e-5, 0)
    close(out["elbo"], g["cw_one_elbo"], 2e-5, 0)
    close(out["kld"], g["cw_one_kld"], 2e-5, 1e-5)
    for l in range(3):
        close(out["z"][l].transpose(0, 1), g[f"cw_one_z{l}"], 1e-5, 1e-6)
        close(out["state_n"][l][0], g[f"cw_one_state_z{l}"], 1e-5, 1e-6)
        close(out["state_n"][l][1], g[f"cw_one_state_h{l}"], 1e-5, 1e-6)


# ----------------------------------------------------------------------------------------------------------------------
# heads_stress.npz: crafted trained-model regimes of the likelihood and KL functions (oracle/gen_golden.py::gen_heads_stress).
# The GPU head tests use the float64 oracle as truth on exactly these inputs; here the oracle in float32 must reproduce the
# reference's float32 values AND autograd gradients on them (256-bin gradient, clamp ties, free-nats ties included).
# ----------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def hs():
    return np.load(os.path.join(GOLDEN, "heads_stress.npz"))


@pytest.mark.parametrize("bins", [2**16, 256])
def test_heads_stress_dmol_values_and_gradients(hs, bins):
    p = T(hs[f"dmol{bins}_par"]).clone().requires_grad_(True)
    y = T(hs[f"dmol{bins}_y"])
    lg, lc, ls = O.dmol_head(p, torch.eye(30), torch.zeros(30))
    ll = O.dmol_ll(y.unsqueeze(1), lg, lc, ls, bins)
    ll.sum().backward()
    close(ll.detach(), hs[f"dmol{bins}_ll"], 1e-6, 1e-6)
    close(p.grad, hs[f"dmol{bins}_grad"], 1e-6, 1e-6)
    # the crafted regimes are really there: raw log-scales exactly at the clamp, frames with |y| > 1 - 2/bins
    raw = T(hs[f"dmol{bins}_par"])[:, 20:]
    assert int((raw == -7.0).sum()) > 50 and int((raw < -7.0).sum()) > 20
    assert int((y.abs() > 1 - 2 / bins).sum()) >= 7


def test_heads_stress_gaussian_heads(hs):
    beta, eps = float(hs["gmm_beta"]), float(hs["gmm_sd_eps"])
    p = T(hs["gmm_par"]).clone().requires_grad_(True)
    y = T(hs["gmm_y"])
    sd = torch.nn.functional.softplus(p[:, 20:], beta=beta) + eps
    ll = O.gaussian_mixture_ll(y.unsqueeze(1), p[:, :10], p[:, 10:20].unsqueeze(1), sd.unsqueeze(1), epsilon=0)
    ll.sum().backward()
    close(ll.detach(), hs["gmm_ll"], 1e-6, 1e-6)
    close(p.grad, hs["gmm_grad"], 1e-6, 1e-6)
    p = T(hs["gauss_par"]).clone().requires_grad_(True)
    ll = O.gaussian_ll(y, p[:, 0], torch.nn.functional.softplus(p[:, 1], beta=beta) + eps, epsilon=0)
    ll.sum().backward()
    close(ll.detach(), hs["gauss_ll"], 1e-6, 1e-6)
    close(p.grad, hs["gauss_grad"], 1e-6, 1e-6)


def test_heads_stress_kl_free_nats_ties(hs):
    ins = [T(hs[f"kl_{k}"]).clone().requires_grad_(True) for k in ("mq", "sq", "mp", "sp")]
    kl = O.kl_gaussian(*ins)
    fn = O.discount_free_nats(kl, float(hs["kl_free_nats"]))
    close(kl.detach(), hs["kl_out"], 1e-6, 1e-6)
    close(fn.detach(), hs["kl_fn"], 1e-6, 1e-6)
    assert bool((kl.detach()[:, ::16] == 0.125).all())  # exact ties with the floor 32 / 256
    for tag, v in (("kl", kl), ("fn", fn)):
        grads = torch.autograd.grad(v.sum(), ins, retain_graph=True)
        for name, gr in zip(("mq", "sq", "mp", "sp"), grads):
            close(gr, hs[f"kl_grad_{tag}_{name}"], 1e-6, 1e-6)
    # at a tie d max(kl, floor)/d kl is 1/2 (torch.maximum), so the floored gradient there is half the raw one
    g_fn, g_kl = T(hs["kl_grad_fn_mq"])[:, ::16], T(hs["kl_grad_kl_mq"])[:, ::16]
    torch.testing.assert_close(g_fn, 0.5 * g_kl, rtol=0, atol=0)


# ----------------------------------------------------------------------------------------------------------------------
# samplers.npz: what the unmodified reference draws and returns on the sampler regimes (oracle/gen_golden.py::gen_samplers).  The
# float32 oracle on the recorded draws must give the reference's samples bit for bit (same torch ops in the same order); the
# float64 detail helper, which is the truth of tests/test_gpu_samplers.py, must hold the reference's samples to the rule of
# tests/draw_cases.py: decided draws at fp32 accuracy, the caps on undecided ones kept by the reference's own draws.
# ----------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def smp():
    import draw_cases as DC

    return DC, DC.load(GOLDEN)


def _ref_draws(fx, name):
    pick = lambda k: T(fx[f"{name}_ref_{k}"] if f"{name}_ref_{k}" in fx else fx[f"{name}_{k}"])  # noqa: E731
    return pick("u"), pick("v")


def test_samplers_dmol_sample_and_mode_match_reference(smp):
    DC, (regs, fx) = smp
    for name in DC.DMOL_REGIMES:
        par, (u, v) = regs[name]["par"], _ref_draws(fx, name)
        logits, locs, ls = O.dmol_head(par, torch.eye(30), torch.zeros(30))
        assert torch.equal(O.dmol_sample(logits, locs, ls, u, v.unsqueeze(1)).squeeze(1), T(fx[f"{name}_ref_x"])), name
        assert torch.equal(O.mix_mode(logits, locs).squeeze(1), T(fx[f"{name}_ref_mode"])), name
        res = DC.judge(name, T(fx[f"{name}_ref_x"]), par, u, v, 0, *DC.head_constants(name, 0, fx))
        DC.report(f"reference fp32 {name}", res)
        d = O.mix_draw_detail(par, None, None, 0)
        assert torch.equal(d["x"].float(), T(fx[f"{name}_ref_mode"])), name  # the mode: first maximum, location NOT clamped
    mode = T(fx["saturation_ref_mode"])
    assert int((mode.abs() > 1).sum()) > 100  # the reference's mode leaves |loc| > 1 as it is (distributions.py:363-368)
    ties = T(fx["ties_ref_mode"])
    assert torch.equal(ties[64:128], regs["ties"]["par"][64:128, 13]) and torch.equal(ties[128:], regs["ties"]["par"][128:, 10])


def test_samplers_gmm_sample_and_mode_match_reference(smp):
    DC, (regs, fx) = smp
    beta, eps = float(fx["gmm_beta"]), float(fx["gmm_sd_eps"])
    for name in DC.GMM_REGIMES:
        par, u, n = regs[name]["par"], regs[name]["u"], regs[name]["n"]
        logits, mu, raw = par[:, :10], par[:, 10:20].unsqueeze(1), par[:, 20:].unsqueeze(1)
        sd = raw if name == "gmm_sd0" else torch.nn.functional.softplus(raw, beta=beta) + eps
        assert torch.equal(O.gmm_sample(logits, mu, sd, u, n.unsqueeze(1)).squeeze(1), T(fx[f"{name}_ref_x"])), name
        assert torch.equal(O.mix_mode(logits, mu).squeeze(1), T(fx[f"{name}_ref_mode"])), name
        res = DC.judge(name, T(fx[f"{name}_ref_x"]), par, u, n, 1, *DC.head_constants(name, 1, fx))
        DC.report(f"reference fp32 {name}", res)
        assert torch.equal(O.mix_draw_detail(par, None, None, 1)["x"].float(), T(fx[f"{name}_ref_mode"])), name


# ----------------------------------------------------------------------------------------------------------------------
# the recurrent models at the frame-stack sizes 1 and 256 of the reference's benchmark table (tests/golden/stack_sizes.npz)
# ----------------------------------------------------------------------------------------------------------------------

STACK_SIZES_BETA, STACK_SIZES_FREE_NATS = 0.8, 1.0


def stack_sizes_setup(kind, S, cks_rel=1e-12):
    """The model, batch and noise of gen_stack_sizes for (kind, S), rebuilt from the seeds and checked against the fixture's checksums
    (the weights are not stored).  Returns (model on the CPU, x, x_sl, eps or None, fixture, key prefix); `test_gpu_stack_sizes.py`
    starts from the same set-up.  cks_rel: checksum tolerance relative to the sum of magnitudes -- 1e-12 on the host that wrote the
    fixture; another host's CPU rounds the orthogonal initialisation's QR and the mu-law's float32 log differently in the last place
    (seen: 2e-7 of a GRU weight's sum, 3e-9 of the batch's), so the GPU tests pass 1e-6: the same tensors to float32 rounding."""

    def same(t, cks, what):
        s, a = t.double().sum().item(), t.double().abs().sum().item()
        assert abs(s - cks[0]) <= cks_rel * cks[1] + 1e-9 and abs(a - cks[1]) <= cks_rel * cks[1], (what, s, a, cks[:2])

    from blvm.models import LSTMAudio, SRNNAudio, VRNNAudio

    g = np.load(os.path.join(GOLDEN, "stack_sizes.npz"))
    tag = f"{kind}{S}"
    torch.manual_seed(S)
    if kind == "vrnn":
        m = VRNNAudio(likelihood="DMoL", input_size=S, hidden_size=32, latent_size=16, residual_posterior=True, num_mix=10, num_bins=2**16)
    elif kind == "srnn":
        m = SRNNAudio(likelihood="DMoL", input_size=S, hidden_size=32, latent_size=16, residual_posterior=True, smoothing=True, num_mix=10, num_bins=2**16)
    else:
        m = LSTMAudio(stack_size=S, hidden_size=32, num_layers=1, num_mix=10, num_bins=2**16)
    sd = m.state_dict()
    assert list(sd.keys()) == g[f"{tag}_param_names"].tolist()
    for k, v in sd.items():
        cks = g[f"{tag}_cks.{k}"]
        assert list(v.shape) == [int(s) for s in cks[2:]], k
        same(v, cks, k)
    x_sl = T(g[f"{tag}_x_sl"])
    B, T_ = x_sl.numel(), int(x_sl.max())
    x = O.synth_batch(B, T_, seed=S)[0] * (torch.arange(T_).unsqueeze(0) < x_sl.unsqueeze(1))
    same(x, g[f"{tag}_x_cks"], "x")
    eps = None
    if kind != "lstm":
        torch.manual_seed(123)
        eps = torch.stack([torch.randn(B, 16) for _ in range(-(-T_ // S))], 0)
        same(eps, g[f"{tag}_eps_cks"], "eps")
    return m, x, x_sl, eps, g, tag


def stack_sizes_oracle(kind, S, sd, x, x_sl, eps):
    if kind == "vrnn":
        return O.vrnn_audio_forward(sd, x, x_sl, eps, beta=STACK_SIZES_BETA, free_nats=STACK_SIZES_FREE_NATS, stack=S)
    if kind == "srnn":
        return O.srnn_audio_forward(sd, x, x_sl, eps, beta=STACK_SIZES_BETA, free_nats=STACK_SIZES_FREE_NATS, stack=S)
    return O.lstm_audio_forward(sd, x, x_sl, stack=S, num_bins=2**16)


@pytest.mark.parametrize("S", [1, 256])
@pytest.mark.parametrize("kind", ["vrnn", "srnn", "lstm"])
def test_stack_sizes_forward_backward(kind, S):
    """The fp32 oracle at stack = 1 and 256 against the reference: the bars of the small-model tests above.  At S = 256 the stride
    ceil(T / T') = 214 is not the stack size, and x_sl = 500 is 3 steps to the KL mask and 2 stacks to the likelihood mask."""
    m, x, x_sl, eps, g, tag = stack_sizes_setup(kind, S)
    sd = {k: v.clone().requires_grad_(True) for k, v in m.state_dict().items()}
    out = stack_sizes_oracle(kind, S, sd, x, x_sl, eps)
    T_ = x.size(1)
    stride = -(-T_ // -(-T_ // S))
    if kind == "lstm":
        close(out["loss"], g[f"{tag}_loss"], 1e-6, 0)
        close(out["ll"], g[f"{tag}_log_prob"], 1e-6, 1e-4)
        close(out["h_n"], g[f"{tag}_h_n"][0], 1e-5, 1e-6)
        close(out["c_n"], g[f"{tag}_c_n"][0], 1e-5, 1e-6)
        assert g[f"{tag}_z_sl"].tolist() == [-(-n // S) for n in x_sl.tolist()]
    else:
        assert out["loss"].dtype == torch.float64
        close(out["loss"], g[f"{tag}_loss"], 1e-7, 0)
        close(out["elbo"], g[f"{tag}_elbo"], 1e-7, 0)
        close(out["log_prob"], g[f"{tag}_log_prob"], 1e-7, 0)
        close(out["kl"], g[f"{tag}_kl"], 1e-6, 1e-6)
        assert g[f"{tag}_z_sl"].tolist() == [-(-n // stride) for n in x_sl.tolist()]
        if S == 256:
            assert stride == 214 and any(-(-n // stride) != -(-n // S) for n in x_sl.tolist())
        if kind == "vrnn":
            close(out["h_n"], g[f"{tag}_h_n"], 1e-5, 1e-6)
            mv = O.vrnn_metrics(out, x_sl, STACK_SIZES_BETA, STACK_SIZES_FREE_NATS)
            for name, val in zip(g[f"{tag}_metric_names"].tolist(), g[f"{tag}_metric_values"].tolist()):
                assert mv[name] == pytest.approx(val, rel=1e-6, abs=1e-9), name
        else:
            close(out["d_n"], g[f"{tag}_d_n"][0], 1e-5, 1e-6)
            close(out["a_n"], g[f"{tag}_a_n"][0], 1e-5, 1e-6)
            close(out["z_n"], g[f"{tag}_z_n"], 1e-5, 1e-6)
    out["loss"].backward()
    names = g[f"{tag}_grad_names"].tolist()
    assert names == [k for k, _ in m.named_parameters()]
    stored = set()
    for name, norm in zip(names, g[f"{tag}_grad_norms"].tolist()):
        gr = sd[name].grad
        assert gr.double().norm().item() == pytest.approx(norm, rel=2e-5), name  # (what the per-tensor bar below implies for a norm)
        if f"{tag}_grad.{name}" in g.files:
            ref = T(g[f"{tag}_grad.{name}"])
            err = (gr - ref).norm() / (ref.norm() + 1e-12)
            assert err < 2e-5, (name, float(err))
            stored.add(name)
        else:
            assert gr.numel() > 8192, name
    first, last = ("embedding.0.weight", "decoder.4.bias") if kind == "lstm" else (f"{kind}.encoder.2.weight", f"{kind}.decoder.4.bias")
    assert {first, last} <= stored and sd[first].shape == (32, S) and sd[last].shape == (30 * S,)
