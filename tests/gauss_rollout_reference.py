"""The VRNNAudio and SRNNAudio generation loops in float64 for the GMM head (kind 1) and the Gaussian head (kind 2), composed from
`blvm_oracle` pieces the goldens pin (`_mlp`, `gaussian_head`, `gru_cell`, `gmm_sample`, `softplus_beta64`, `mix_draw_detail`).  Draws
are arguments: eps [T,B,Z], u [T,B,S,K] (GMM) and n [T,B,S]; u = n = None takes the head's mode.  Every function returns the per-draw
pick margins `s_best - s_runner` of the GMM head ([T,B,S]; None for the Gaussian head), so that a test can show no pick was a toss-up.

TEST INFRASTRUCTURE: not imported by the product.
"""
import math

import torch
import torch.nn.functional as F

import blvm_oracle as O

LN2 = math.log(2.0)
HEAD_EPS = 1e-4  # `epsilon` of both Gaussian heads in VRNNAudio / SRNNAudio
GMM, GAUSS = 1, 2


def head_constants(kind):
    """(softplus beta, epsilon) of the head's scale, as the model constructors make them: the GMM head's beta is ln2 / initial_sd
    (epsilon is not subtracted there), the Gaussian head's ln2 / (initial_sd - epsilon)."""
    return (LN2, HEAD_EPS) if kind == GMM else (LN2 / (1.0 - HEAD_EPS), HEAD_EPS)


def to64(sd):
    return {k: torch.as_tensor(v).double() for k, v in sd.items()}


def head_draw(sd, prefix, dec, kind, u_t, n_t):
    """dec [B,S,F] float64 -> (x [B,S], margins [B,S] or None)."""
    B, S, _ = dec.shape
    par = F.linear(dec, sd[f"{prefix}.likelihood.params.weight"], sd[f"{prefix}.likelihood.params.bias"])
    beta, eps = head_constants(kind)
    if kind == GAUSS:
        mu, sdv = par[..., 0], O.softplus_beta64(par[..., 1], beta) + eps
        return (mu if n_t is None else mu + sdv * n_t.double()), None
    K = par.shape[-1] // 3
    det = O.mix_draw_detail(par.reshape(B * S, 3 * K), None if u_t is None else u_t.reshape(B * S, K), None if n_t is None else n_t.reshape(B * S),
                            kind=1, sd_beta=beta, sd_eps=eps)  # fmt: skip
    margins = (det["s_best"] - det["s_runner"]).reshape(B, S)
    logits, mu = par[..., :K], par[..., K : 2 * K].unsqueeze(-2)
    if u_t is None:
        x = O.mix_mode(logits, mu).squeeze(-1)
    else:
        sdv = (O.softplus_beta64(par[..., 2 * K :], beta) + eps).unsqueeze(-2)
        x = O.gmm_sample(logits, mu, sdv, u_t.double(), n_t.double().unsqueeze(-1)).squeeze(-1)
    assert torch.equal(x, det["x"].reshape(B, S)), "gmm_sample and mix_draw_detail disagree"
    return x, margins


def vrnn_generate(sd, kind, x0, eps, u, n, h0=None, prefix="vrnn"):
    """VRNN.generate: x0 [B,S] -> dict(x [B,T,S], h_n [B,R], margins)."""
    sd = to64(sd)
    cell = f"{prefix}.vrnn_cell"
    T, B = eps.shape[0], x0.shape[0]
    S = x0.shape[1]
    R = sd[f"{cell}.gru_cell.weight_hh"].size(1)
    x = x0.double().reshape(B, S)
    h = torch.zeros(B, R, dtype=torch.float64) if h0 is None else h0.double()
    xs, margins = [], []
    for t in range(T):
        enc = O._mlp(x, sd, f"{prefix}.encoder", (2, 4, 6), F.leaky_relu)
        p = O._mlp(h, sd, f"{cell}.prior", (0, 2, 4), F.relu)
        mu_p, sd_p = O.gaussian_head(p, sd[f"{cell}.prior.6.params.weight"], sd[f"{cell}.prior.6.params.bias"])
        z = eps[t].double() * sd_p + mu_p
        phi = O._mlp(z, sd, f"{cell}.phi_z", (0, 2, 4, 6), F.relu)
        h = O.gru_cell(torch.cat([enc, phi], -1), h, sd[f"{cell}.gru_cell.weight_ih"], sd[f"{cell}.gru_cell.weight_hh"],
                       sd[f"{cell}.gru_cell.bias_ih"], sd[f"{cell}.gru_cell.bias_hh"])  # fmt: skip
        dec = O._mlp(torch.cat([phi, h], -1), sd, f"{prefix}.decoder", (0, 2, 4), F.leaky_relu).view(B, S, -1)
        x, m = head_draw(sd, prefix, dec, kind, None if u is None else u[t], None if n is None else n[t])
        xs.append(x)
        margins.append(m)
    return dict(x=torch.stack(xs, 1), h_n=h, margins=None if kind == GAUSS else torch.stack(margins))


def srnn_generate(sd, kind, x0, eps, u, n, d0=None, z0=None, prefix="srnn"):
    """SRNN.generate, unconditional: x0 [B,S] -> dict(x [B,T,S], d_n [B,R], z [T,B,Z], h_p [B,R+Z] = cat[d_T, z_{T-1}], margins)."""
    sd = to64(sd)
    g = f"{prefix}.d_forward_recurrent"
    T, B = eps.shape[0], x0.shape[0]
    S = x0.shape[1]
    R = sd[f"{g}.weight_hh_l0"].size(1)
    Z = sd[f"{prefix}.prior.6.params.weight"].size(0) // 2
    x = x0.double().reshape(B, S)
    d_t = torch.zeros(B, R, dtype=torch.float64) if d0 is None else d0.double()
    z_t = torch.zeros(B, Z, dtype=torch.float64) if z0 is None else z0.double()
    xs, zs, margins, h_p = [], [], [], None
    for t in range(T):
        enc = O._mlp(x, sd, f"{prefix}.encoder", (2, 4, 6), F.leaky_relu)
        d_t = O.gru_cell(enc, d_t, sd[f"{g}.weight_ih_l0"], sd[f"{g}.weight_hh_l0"], sd[f"{g}.bias_ih_l0"], sd[f"{g}.bias_hh_l0"])
        h_p = torch.cat([d_t, z_t], -1)
        hp = O._mlp(h_p, sd, f"{prefix}.prior", (0, 2, 4), F.leaky_relu)
        mu_p, sd_p = O.gaussian_head(hp, sd[f"{prefix}.prior.6.params.weight"], sd[f"{prefix}.prior.6.params.bias"])
        z_t = eps[t].double() * sd_p + mu_p
        zs.append(z_t)
        dec = O._mlp(torch.cat([z_t, d_t], -1), sd, f"{prefix}.decoder", (0, 2, 4), F.leaky_relu).view(B, S, -1)
        x, m = head_draw(sd, prefix, dec, kind, None if u is None else u[t], None if n is None else n[t])
        xs.append(x)
        margins.append(m)
    return dict(x=torch.stack(xs, 1), d_n=d_t, z=torch.stack(zs), h_p=h_p, margins=None if kind == GAUSS else torch.stack(margins))
