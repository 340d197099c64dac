"""GPU: the tiles of the persistent chains (csrc/pchain.h) with the store the next link polls issued first.

Every tile stores the T16 copy of its output — what the next link polls — in front of the row-major copy, which is only read
after the launch (`put`; the dz and GRU-backward tiles: all T16 stores of their two outputs, then the row-major ones), and
`tile_head` stores z before it evaluates the prior's softplus and before any statistic is stored (residual 0 and 1; residual 2
and 3 need sd_p for z and keep the old order).  Only the order of independent statements and stores changed, so

* the static walk (csrc/vrnn_static.hip) and the interpreter (csrc/pchain.hip, `blvm_pchain_static(0)`) must agree BIT FOR BIT,
  forward and backward: loss, per-utterance ELBO and KL, z, h_n, and what the backward walk writes without an atomic sum behind
  it, d_h0 and d_enc.  h = z = 256, T' = 4, B = 1 / 17 / 64, free nats 0 and 2, and three sets of lengths: all rows full, one
  row that ends inside step 1, one row of length 0 — the short row is the only row (B = 1), the first row of the second row tile
  (B = 17) or the last row of the first (B = 64), so `live` is false on both sides of a 16-row tile edge.  The comparison is on
  the bit patterns, so it also holds where a value is not finite (B = 1 with its only row empty: a step over zero frames);
* the two orders the reorder left alone are still right: one forward each in residual 2 (precision-weighted posterior) and 3
  (generation: z from the prior) through the RSSM cell's engine program, which is what reaches them, against the float64 oracle at
  the bars of `tests/test_gpu_rssm_paths.py` (relative L2 <= 1e-5, also per batch row; generation rtol 1e-4 / atol 1e-5)."""
import ctypes
import functools

import pytest
import torch

import blvm_oracle as O
from blvm import _hip
from blvm.models import VRNNAudio
from blvm.modules.rssm import RSSMCell

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 64   # samples per frame, as bench.py
H = 256  # the static walk is built for H = Z = 256 (R = 512)
TP = 4
EXACT = ["loss", "elbo", "kl", "z", "h_n", "d_h0", "d_enc"]
SHORT_ROW = {1: 0, 17: 16, 64: 15}
BAR_VALUE = 1e-5


def _lib():
    lib = _hip.load()
    assert lib.blvm_device_ok() == 1
    return lib


@functools.lru_cache(maxsize=None)
def _model():
    torch.manual_seed(21)
    return VRNNAudio(likelihood="DMoL", input_size=S, hidden_size=H, latent_size=H, residual_posterior=True).to(DEV)


def _lengths(B, lengths):
    x_sl = torch.full((B,), TP * S, dtype=torch.int64)
    if lengths == "ends_in_step_1":
        x_sl[SHORT_ROW[B]] = S + S // 2
    elif lengths == "empty_row":
        x_sl[SHORT_ROW[B]] = 0
    else:
        assert lengths == "full"
    return x_sl


@functools.lru_cache(maxsize=None)
def _inputs(B):
    g = torch.Generator().manual_seed(22 + B)
    x = (torch.rand(B, TP * S, generator=g) * 2 - 1).to(DEV)
    eps = torch.randn(TP, B, H, generator=g).to(DEV)
    h0 = (torch.rand(B, 2 * H, generator=g) * 2 - 1).to(DEV)
    return x, eps, h0


def _step(m, B, x_sl, free_nats, static):
    """One forward + backward on the chosen path: the step's results, the backward walk's own outputs, the static launches."""
    lib = _lib()
    was = lib.blvm_pchain_static(1 if static else 0)
    n0 = lib.blvm_pchain_static(-2)
    cell = m.vrnn.vrnn_cell
    seq, res = cell.sequence, {}

    def tapped(enc, *a, **kw):
        enc.register_hook(lambda g: res.__setitem__("d_enc", g.detach().clone()))
        return seq(enc, *a, **kw)

    try:
        cell.sequence = tapped
        x, eps, h0 = _inputs(B)
        h = h0.clone().requires_grad_(True)
        m.zero_grad(set_to_none=True)
        loss, _, out = m(x, x_sl, beta=1.0, free_nats=free_nats, eps=eps, h0=h)
        loss.backward()
        torch.cuda.synchronize()
        res.update(loss=loss.detach().clone(), elbo=out.elbo.detach().clone(), kl=out.kl.detach().clone(), z=out.z.detach().clone(),
                   h_n=out.h_n.detach().clone(), d_h0=h.grad.detach().clone())
        launches = lib.blvm_pchain_static(-2) - n0
    finally:
        del cell.sequence  # (back to the class's method)
        lib.blvm_pchain_static(was)
    assert _hip.take_async_errors() == (0, 0)
    return res, launches


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


@pytest.mark.timeout(120)
@pytest.mark.parametrize("lengths", ["full", "ends_in_step_1", "empty_row"])
@pytest.mark.parametrize("free_nats", [0.0, 2.0])
@pytest.mark.parametrize("B", [1, 17, 64])
def test_static_walk_matches_interpreter_bit_for_bit(B, free_nats, lengths):
    m, x_sl = _model(), _lengths(B, lengths)
    st, n_st = _step(m, B, x_sl, free_nats, True)
    it, n_it = _step(m, B, x_sl, free_nats, False)
    assert (n_st, n_it) == (2, 0)  # forward and backward ran on the static kernels, and only with the selector on
    assert set(st) == set(it) == set(EXACT)
    bad = [k for k in EXACT if not _same_bits(st[k], it[k])]
    assert not bad, f"static and interpreter differ in {bad}"
    if int(x_sl.sum()) > 0:  # (a step over zero frames divides by them)
        assert all(bool(torch.isfinite(st[k]).all()) for k in EXACT)
        assert float(st["d_h0"].abs().max()) > 0 and float(st["d_enc"].abs().max()) > 0
    if lengths == "empty_row" and B > 1:  # the empty row takes no part in the step: nothing flows back into it
        r = SHORT_ROW[B]
        assert float(st["d_enc"][:, r].abs().max()) == 0.0 and float(st["kl"][r]) == 0.0


# ---- residual 2 and 3 of tile_head: the RSSM cell's engine program against float64 ------------------------------------------------


def _rssm_counts():
    buf = (ctypes.c_ulonglong * 6)()
    _hip.check(_hip.load().blvm_rssm_path_counts(buf), "blvm_rssm_path_counts")
    return list(buf)


class _engine_program:
    """The block's RSSM forward runs as ONE engine program (that is what calls tile_head), and nothing else ran."""

    def __enter__(self):
        self.lib = _lib()
        self.before = self.lib.blvm_pchain_max_batch()
        self.lib.blvm_pchain_configure(128, 0)
        self.c0 = _rssm_counts()

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        delta = [a - b for a, b in zip(_rssm_counts(), self.c0)]
        self.lib.blvm_pchain_configure(self.before, 0)
        if exc[0] is None:
            assert delta == [1, 0, 0, 0, 0, 0], delta
            assert _hip.take_async_errors() == (0, 0)


def _rel(a, b, row_dim=None):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape and bool(torch.isfinite(a).all())
    err = float((a - b).norm() / (b.norm() + 1e-30))
    if row_dim is not None:
        a2, b2 = a.movedim(row_dim, 0).reshape(a.shape[row_dim], -1), b.movedim(row_dim, 0).reshape(b.shape[row_dim], -1)
        err = max(err, float(((a2 - b2).norm(dim=1) / (b2.norm(dim=1) + 1e-30)).max()))
    return err


#                       T  B   H   Z   C   E     B = 17: a full row tile and a tile of one row
RSSM_SHAPE = (3, 17, 64, 32, 32, 32)


def _rssm_inputs():
    T, B, Hc, Z, C, E = RSSM_SHAPE
    gen = torch.Generator().manual_seed(6)
    enc, ctx, eps = torch.randn(T, B, E, generator=gen), torch.randn(T, B, C, generator=gen), torch.randn(T, B, Z, generator=gen)
    z0, h0 = 0.3 * torch.randn(B, Z, generator=gen), 0.3 * torch.randn(B, Hc, generator=gen)
    return enc, ctx, eps, z0, h0


def test_head_precision_weighted_vs_oracle_float64():
    """residual 2: z, the state and the four statistics (sd_q is the combined scale) of a precision-weighted RSSM forward."""
    T, B, Hc, Z, C, E = RSSM_SHAPE
    torch.manual_seed(5)
    cell = RSSMCell(z_dim=Z, h_dim=Hc, c_dim=C, e_dim=E, precision_posterior=True)
    enc, ctx, eps, z0, h0 = _rssm_inputs()
    sd64 = {k: v.detach().double() for k, v in cell.state_dict().items()}
    with torch.no_grad():
        zs_r, hs_r, d = O.rssm_sequence(sd64, enc.double(), ctx.double(), (z0.double(), h0.double()), eps.double(), precision_posterior=True)
    cell = cell.to(DEV)
    x_sl = torch.full((B,), T * 3, dtype=torch.int32, device=DEV)
    with torch.no_grad(), _engine_program():
        zs, hs, _, _, mu_q, sd_q, mu_p, sd_p = cell.sequence(enc.to(DEV), ctx.to(DEV), (z0.to(DEV), h0.to(DEV)), eps.to(DEV), x_sl, 3, 0.0)
    errs = {k: _rel(got, ref, 1) for k, got, ref in (("zs", zs[1:], zs_r), ("hs", hs[1:], hs_r), ("enc_mu", mu_q, d["enc_mu"]),
            ("enc_sd", sd_q, d["enc_sd"]), ("prior_mu", mu_p, d["prior_mu"]), ("prior_sd", sd_p, d["prior_sd"]))}  # fmt: skip
    print("precision-weighted head, rel_l2 (worst of tensor and rows): " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    bad = {k: v for k, v in errs.items() if v > BAR_VALUE}
    assert not bad, bad


def test_head_generation_vs_oracle_float64():
    """residual 3: z drawn from the prior, non-zero eps, a given state and context."""
    T, B, Hc, Z, C, E = RSSM_SHAPE
    torch.manual_seed(5)
    cell = RSSMCell(z_dim=Z, h_dim=Hc, c_dim=C, e_dim=E)
    _, ctx, eps, z0, h0 = _rssm_inputs()
    sd64 = {k: v.detach().double() for k, v in cell.state_dict().items()}
    state, zs_r, hs_r = (z0.double(), h0.double()), [], []
    with torch.no_grad():
        for t in range(T):
            state = O.rssm_generate_step(sd64, state, ctx[t].double(), eps[t].double())
            zs_r.append(state[0])
            hs_r.append(state[1])
    cell = cell.to(DEV)
    with _engine_program():
        zs, hs = cell.generate_sequence(ctx.to(DEV), (z0.to(DEV), h0.to(DEV)), eps.to(DEV), T, B)
    zs, hs = zs.double().cpu(), hs.double().cpu()
    assert torch.equal(zs[0], z0.double()) and torch.equal(hs[0], h0.double())
    torch.testing.assert_close(zs[1:], torch.stack(zs_r, 0), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(hs[1:], torch.stack(hs_r, 0), rtol=1e-4, atol=1e-5)
