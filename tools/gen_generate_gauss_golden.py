"""Writes tests/golden/generate_gauss.npz: ancestral sampling from the UNMODIFIED reference's VRNNAudio("GMM") and SRNNAudio("GMM") at
S=16, H=32, Z=16, B=5, T=7, with the draws the reference made replayed beside its samples.  Run like oracle/gen_golden.py, with the
reference on the path (it is imported, nothing of it is copied):

    BLVM_DATA_ROOT_DIRECTORY=/tmp/blvm_data PYTHONDONTWRITEBYTECODE=1 \
    PYTHONPATH=oracle/refshim:<reference checkout> python tools/gen_generate_gauss_golden.py

Draw order per step (the reference's generate loops and its Gaussian-mixture sampler): randn(B, Z) for the prior sample, then
uniform_(1e-6, 1 - 1e-6) over [B,S,K] for the component pick, then randn(B, S, 1) for the picked component.  The models are constructed
and seeded as `gen_generate16` of oracle/gen_golden.py seeds its DMoL twins; the seed of the draws is the first one, counting from 0, for
which every component pick of the float64 restatement (tests/gauss_rollout_reference.py) has a margin s_best - s_runner of at least
1e-3, so that no element of the fixture hangs on a toss-up.  `e_ref` = the largest absolute difference between the reference's fp32
samples and that restatement on the same draws: the yardstick of the GPU tests.

TEST INFRASTRUCTURE: not imported by the product.
"""
import os
import sys
import warnings

import numpy as np
import torch

warnings.filterwarnings("ignore")
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import blvm.models as RM  # noqa: E402  (the reference, via PYTHONPATH)

import gauss_rollout_reference as G  # noqa: E402

S, H, Z, B, T, K = 16, 32, 16, 5, 7, 10
MIN_MARGIN = 1e-3


def replay(seed):
    torch.manual_seed(seed)
    e, u, n = [], [], []
    for _ in range(T):
        e.append(torch.randn(B, Z))
        u.append(torch.empty(B, S, K).uniform_(1e-6, 1 - 1e-6))
        n.append(torch.randn(B, S, 1))
    return torch.stack(e), torch.stack(u), torch.stack(n).squeeze(-1)


def first_seed(restate):
    for seed in range(1000):
        e, u, n = replay(seed)
        r = restate(e, u, n)
        if float(r["margins"].min()) >= MIN_MARGIN:
            return seed, e, u, n, r
    raise SystemExit("no seed below 1000 keeps every pick margin above 1e-3")


def main():
    arrays = {}
    torch.manual_seed(17)
    v = RM.VRNNAudio(likelihood="GMM", input_size=S, hidden_size=H, latent_size=Z, residual_posterior=True, num_mix=10, num_bins=2**16)
    x0 = torch.rand(B, S, 1, generator=torch.Generator().manual_seed(5)) * 0.2 - 0.1
    sd = v.state_dict()
    seed, e, u, n, r = first_seed(lambda e, u, n: G.vrnn_generate(sd, G.GMM, x0.reshape(B, S), e, u, n))
    torch.manual_seed(seed)
    (xv, xv_sl), _ = v.generate(n_samples=B, max_timesteps=T, x=x0)
    e_vr = float((xv[:, 1:].double() - r["x"]).abs().max())
    assert torch.equal(xv[:, 0], x0.reshape(B, S))
    arrays.update(vr_x=xv, vr_x_sl=xv_sl, vr_x0=x0, vr_eps=e, vr_u=u, vr_n=n, vr_seed=seed, vr_min_margin=float(r["margins"].min()))
    for k, p in sd.items():
        arrays[f"vr_sd.{k}"] = p

    torch.manual_seed(19)
    sr = RM.SRNNAudio(likelihood="GMM", input_size=S, hidden_size=H, latent_size=Z, residual_posterior=True, smoothing=True)
    sd = sr.state_dict()
    seed, e, u, n, r = first_seed(lambda e, u, n: G.srnn_generate(sd, G.GMM, torch.zeros(B, S), e, u, n))
    torch.manual_seed(seed)
    (xs, xs_sl), out = sr.generate(n_samples=B, max_timesteps=T)
    e_sr = float((xs.squeeze(-1).double() - r["x"]).abs().max())
    e_hp = float((out.h_p.reshape(B, -1).double() - r["h_p"]).abs().max())
    arrays.update(sr_x=xs, sr_x_sl=xs_sl, sr_eps=e, sr_u=u, sr_n=n, sr_h_p=out.h_p, sr_seed=seed, sr_min_margin=float(r["margins"].min()))
    for k, p in sd.items():
        arrays[f"sr_sd.{k}"] = p
    arrays.update(e_ref=max(e_vr, e_sr), e_ref_vrnn=e_vr, e_ref_srnn=e_sr, e_ref_h_p=e_hp)
    path = os.path.join(ROOT, "tests", "golden", "generate_gauss.npz")
    np.savez_compressed(path, **{k: (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)) for k, a in arrays.items()})
    print(f"wrote generate_gauss.npz: {os.path.getsize(path) / 1024:.1f} KiB; seeds {arrays['vr_seed']}, {arrays['sr_seed']}; "
          f"e_ref vrnn {e_vr:.3e} srnn {e_sr:.3e} h_p {e_hp:.3e}")  # fmt: skip


if __name__ == "__main__":
    main()
