"""Both implementations of the RSSM sequence entry points (K5, csrc/rssm.hip), forward and backward, against float64.

`blvm_rssm_seq_fwd/_bwd` run a sequence either as one program of the persistent-chain engine (B <= 128 with the engine on) or as
one launch per link and step (B > 128, or the engine switched off).  The second implementation has kernels of its own
(`gru_cell_stage_kernel`, `rssm_dh_stage_kernel`), a BPTT loop of its own (the three-segment link that carries `G += DGH[t+1] Whh`,
`dz.has_gemm = !last`, the `d_z0` / `d_h0` tail launches), is the only user of modes 2 (precision-weighted) and 3 (generate) of
the shared head / dz stage kernels, and puts its links on 32x32 tiles from B = 128 on when every width allows it.  It is where
`CWVAE(with_resets=True)` trains its lower levels: the segments between two resets become batch rows (`CWVAE._fold`).
`blvm_rssm_path_counts` says which arm a call took and which tiles its links ran on; every case asserts it, so a change of the
dispatch conditions cannot silently move a case onto another kernel.

Reference: `blvm_oracle.rssm_sequence` / `rssm_generate_step` / `cwvae_audio_forward` with `kl_gaussian`, `discount_free_nats` and
`sequence_mask`, stepped on the CPU in float64.  Parameters and inputs are generated in fp32 and widened exactly.  The same oracle
evaluated in fp32 is printed beside every figure as the yardstick of what fp32 arithmetic costs on these shapes.

Loss of the cell cases: (zs[1:] wz).sum() + (hs[1:] wh).sum() + 0.7 kld.sum() + 1.3 kld_fn.sum() with random wz, wh: both KL
coefficients are live and different, and the direct gradient wrt h is non-zero at every step.  Lengths are ragged through `x_sl`
with stride 3: a row that ends before the last step and a row whose length is an exact multiple of the stride (`t stride < x_sl`).

Free nats: the floor is not chosen by hand.  It is the midpoint of the widest gap between neighbouring values of the float64
oracle's element-wise KL (live steps) inside its inter-quartile range, so that elements lie on both sides of the `k > fn_floor`
branch of the dz stage kernel, and the inputs are accepted only if (a) the share of live elements above the floor is within
[0.25, 0.75] and (b) half the gap is at least 20 times the largest |KL(fp32 oracle) - KL(float64 oracle)|: an fp32 evaluation cannot
put an element on the other side.

Bounds (the project's bars): relative L2 <= 1e-5 for states, latents, distribution parameters and KL sums; <= 1e-3 per tensor for
every gradient (parameters, enc, ctx, z0, h0); generation rtol 1e-4 / atol 1e-5; model-level loss / ELBO / log-likelihood 1e-5
relative.  States and input gradients are also held to their bar per batch row, so a wrong last row of a partial tile fails by
its index instead of being averaged away."""
import contextlib
import copy
import ctypes
import functools

import pytest
import torch

import blvm_oracle as O
from blvm import _hip
from blvm.modules.rssm import RSSMCell

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR_VALUE, BAR_GRAD, BAR_MODEL = 1e-5, 1e-3, 1e-5
STRIDE = 3
COUNTER_NAMES = ("forward on the engine program", "forward on launch-per-link", "backward on the engine program",
                 "backward on launch-per-link", "16x16-tile link launches", "32x32-tile link launches")  # fmt: skip
MODES = {"plain": {}, "residual": dict(residual_posterior=True), "precision": dict(precision_posterior=True)}

#        T  B    H    Z   C    E    mode         state0 given
CASES = {
    "A": (5, 5, 32, 16, 16, 32, "plain", True),  # partial 16-row tile; every step kernel at NW = 4; d_z0 / d_h0 tails
    "B": (5, 5, 96, 32, 0, 32, "residual", False),  # top level: C = 0, null z0 / h0 (no tails); gru_cell<8>, head<8>
    "C": (4, 8, 192, 64, 192, 192, "precision", True),  # C4 widths: gru_cell<16>, rssm_dh<8>, head<16>, 16-wave links; mode 2
    "D": (4, 129, 64, 32, 32, 32, "precision", True),  # one row beyond the engine; every link on 32x32 tiles, last tile: 1 row
    "E": (4, 129, 48, 16, 16, 16, "residual", True),  # large batch, widths rule the wide kernel out: 9 row tiles of 16
}


@pytest.fixture(scope="module", autouse=True)
def _require_hip_and_restore_engine():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    lib = _hip.load()
    assert lib.blvm_device_ok() == 1, "libblvm_hip: no gfx950 device visible"
    before = lib.blvm_pchain_max_batch()
    try:
        yield
    finally:
        lib.blvm_pchain_configure(before, 0)


@contextlib.contextmanager
def engine(on):
    """The execution switch of K1-K5 for the block: True = engine up to 128 rows, False = off, None = as found."""
    lib = _hip.load()
    before = lib.blvm_pchain_max_batch()
    if on is not None:
        lib.blvm_pchain_configure(128 if on else 0, 0)
    try:
        yield
    finally:
        lib.blvm_pchain_configure(before, 0)


def path_counts():
    buf = (ctypes.c_ulonglong * 6)()
    _hip.check(_hip.load().blvm_rssm_path_counts(buf), "blvm_rssm_path_counts")
    return list(buf)


@contextlib.contextmanager
def expect_path(want, what):
    """The RSSM entry points called inside the block took exactly the arms `want` (six counter increments)."""
    before = path_counts()
    yield
    torch.cuda.synchronize()
    delta = [a - b for a, b in zip(path_counts(), before)]
    print(f"{what}: " + ", ".join(f"{COUNTER_NAMES[k]} x{n}" for k, n in enumerate(delta) if n))
    assert delta == list(want), f"{what}: expected {dict(zip(COUNTER_NAMES, want))}, the counters report {dict(zip(COUNTER_NAMES, delta))}"


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


class Checks:
    """Collects every figure of a case (printed) and every miss; `done()` asserts there was none."""

    def __init__(self, tag):
        self.tag, self.failures, self.worst = tag, [], {}

    def close(self, kind, name, got, ref, bar, yard=None, row_dim=None):
        got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        if not bool(torch.isfinite(got).all()):
            self.failures.append(f"{name}: non-finite values")
            return
        err = float((got - ref).norm() / (ref.norm() + 1e-30))
        rows = ""
        if row_dim is not None:
            g2, r2 = got.movedim(row_dim, 0).reshape(got.shape[row_dim], -1), ref.movedim(row_dim, 0).reshape(ref.shape[row_dim], -1)
            rr = (g2 - r2).norm(dim=1) / (r2.norm(dim=1) + 1e-30)
            k = int(rr.argmax())
            rows = f", worst row {k}: {float(rr[k]):.3e}"
            if float(rr[k]) > bar:
                self.failures.append(f"{name} row {k}: rel_l2 {float(rr[k]):.3e} > {bar:.0e}")
            err_all = max(err, float(rr[k]))
        else:
            err_all = err
        self.worst[kind] = max(self.worst.get(kind, 0.0), err_all)
        y = "" if yard is None else f", fp32 oracle {yard:.3e}"
        print(f"{self.tag} {name}: rel_l2 {err:.3e}{rows} (bar {bar:.0e}{y})")
        if err > bar:
            self.failures.append(f"{name}: rel_l2 {err:.3e} > {bar:.0e}")

    def done(self):
        torch.cuda.synchronize()
        errs = _hip.take_async_errors()
        if errs != (0, 0):
            self.failures.append(f"a persistent launch gave up on a bounded spin: {errs}")
        print(f"{self.tag} maxima: " + ", ".join(f"{k} {v:.3e}" for k, v in self.worst.items()))
        assert not self.failures, f"{self.tag}:\n  " + "\n  ".join(self.failures)


# ----------------------------------------------------------------------------------------------------------------------
# inputs and references (computed once per case, shared by the engine-on and engine-off runs, never modified)
# ----------------------------------------------------------------------------------------------------------------------


def ragged_lengths(T, B):
    """x_sl for `t * STRIDE < x_sl`: row 0 full, row 1 an exact multiple of the stride that ends early, the last row (alone in its
    tile at B = 129) ends after two steps, the others spread over 1 .. T * STRIDE."""
    n = T * STRIDE
    sl = [(7 * b + 3) % n + 1 for b in range(B)]
    sl[0], sl[1], sl[-1] = n, 2 * STRIDE, STRIDE + 1
    sl = torch.tensor(sl, dtype=torch.int64)
    steps = torch.div(sl + STRIDE - 1, STRIDE, rounding_mode="floor")
    assert int(sl.min()) >= 1 and int(steps.max()) == T and bool((steps < T).any())
    assert bool(((sl % STRIDE == 0) & (sl < n)).any())
    return sl


def floor_from_reference(kl64, kl32, live):
    """Per-element free-nats floor from the float64 KL alone (module docstring); asserts the input conditions (a) and (b)."""
    v = kl64[live].sort().values
    w = kl32.double()[live]
    n = v.numel()
    lo, hi = n // 4, (3 * n) // 4
    gaps = v[lo + 1 : hi + 1] - v[lo:hi]
    i = int(gaps.argmax())
    floor, half_gap = float((v[lo + i] + v[lo + i + 1]) / 2), float(gaps[i]) / 2
    share = float((v > floor).double().mean())
    err32 = float((w - kl64[live]).abs().max())
    assert 0.25 <= share <= 0.75, f"(a) share of live elements above the floor {share:.3f}"
    assert half_gap >= 20 * err32, f"(b) half gap {half_gap:.3e} < 20 x fp32 KL error {err32:.3e}"
    return floor, share, half_gap, err32


def _oracle_cell(cell, kw, tensors, x_sl, given, dtype, free_nats):
    """The cell stepped by the oracle in `dtype`; free_nats None: forward only (element-wise KL), else loss and backward."""
    enc, ctx, eps, z0, h0, wz, wh = (None if t is None else t.to(dtype) for t in tensors)
    T, B = eps.shape[:2]
    sd = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in cell.state_dict().items()}
    leaves = {"enc": enc.clone().requires_grad_(True)}
    if ctx is not None:
        leaves["ctx"] = ctx.clone().requires_grad_(True)
    if given:
        leaves["z0"], leaves["h0"] = z0.clone().requires_grad_(True), h0.clone().requires_grad_(True)
    ctx_o = leaves["ctx"] if ctx is not None else torch.zeros(T, B, 0, dtype=dtype)
    st0 = (leaves["z0"], leaves["h0"]) if given else (torch.zeros(B, cell.z_dim, dtype=dtype), torch.zeros(B, cell.h_dim, dtype=dtype))
    with torch.set_grad_enabled(free_nats is not None):
        zs, hs, d = O.rssm_sequence(sd, leaves["enc"], ctx_o, st0, eps, **kw)
        kl = O.kl_gaussian(d["enc_mu"], d["enc_sd"], d["prior_mu"], d["prior_sd"])
    if free_nats is None:
        return kl
    mask = O.sequence_mask(torch.ceil(x_sl / STRIDE).long(), max_len=T).t().unsqueeze(-1)
    kld, kld_fn = (kl * mask).sum((0, 2)), (O.discount_free_nats(kl, free_nats) * mask).sum((0, 2))
    ((zs * wz).sum() + (hs * wh).sum() + 0.7 * kld.sum() + 1.3 * kld_fn.sum()).backward()
    out = dict(zs=zs, hs=hs, kld=kld, kld_fn=kld_fn, **d)
    out = {k: v.detach() for k, v in out.items()}
    out["grads"] = {**{k: v.grad for k, v in leaves.items()}, **{k: v.grad for k, v in sd.items()}}
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    T, B, H, Z, C, E, mode, given = CASES[name]
    torch.manual_seed(5)
    cell = RSSMCell(z_dim=Z, h_dim=H, c_dim=C, e_dim=E, **MODES[mode])
    gen = torch.Generator().manual_seed(6)
    enc = torch.randn(T, B, E, generator=gen)
    ctx = torch.randn(T, B, C, generator=gen) if C else None
    eps = torch.randn(T, B, Z, generator=gen)
    z0, h0 = 0.3 * torch.randn(B, Z, generator=gen), 0.3 * torch.randn(B, H, generator=gen)
    wz, wh = torch.randn(T, B, Z, generator=gen), torch.randn(T, B, H, generator=gen)
    tensors = (enc, ctx, eps, z0, h0, wz, wh)
    x_sl = ragged_lengths(T, B)
    live = (torch.arange(T).unsqueeze(1) * STRIDE < x_sl.unsqueeze(0)).unsqueeze(-1).expand(T, B, Z)
    kl64 = _oracle_cell(cell, MODES[mode], tensors, x_sl, given, torch.float64, None)
    kl32 = _oracle_cell(cell, MODES[mode], tensors, x_sl, given, torch.float32, None)
    floor, share, half_gap, err32 = floor_from_reference(kl64, kl32, live)
    free_nats = floor * Z
    print(f"case {name}: free nats {free_nats:.6f} (floor {floor:.6f} per element), {share:.3f} of {int(live.sum())} live elements above, "
          f"half gap {half_gap:.3e} = {half_gap / err32:.0f} x the fp32 oracle's KL error {err32:.3e}")  # fmt: skip
    r64 = _oracle_cell(cell, MODES[mode], tensors, x_sl, given, torch.float64, free_nats)
    r32 = _oracle_cell(cell, MODES[mode], tensors, x_sl, given, torch.float32, free_nats)
    yard = {k: rel(r32[k], v) for k, v in r64.items() if k != "grads"}
    yard.update({f"d_{k}": rel(r32["grads"][k], v) for k, v in r64["grads"].items()})
    return dict(cell=cell, tensors=tensors, x_sl=x_sl, free_nats=free_nats, ref=r64, yard=yard)


def run_cell_case(name, engine_on, want):
    T, B, H, Z, C, E, mode, given = CASES[name]
    r = reference(name)
    ref, yard = r["ref"], r["yard"]
    enc, ctx, eps, z0, h0, wz, wh = (None if t is None else t.to(DEV) for t in r["tensors"])
    cell = copy.deepcopy(r["cell"]).to(DEV)
    leaves = {"enc": enc.requires_grad_(True)}
    if ctx is not None:
        leaves["ctx"] = ctx.requires_grad_(True)
    if given:
        leaves["z0"], leaves["h0"] = z0.requires_grad_(True), h0.requires_grad_(True)
    tag = f"rssm {name} ({mode}, T={T} B={B} H={H} Z={Z} C={C} E={E}, engine {'as found' if engine_on is None else ('on' if engine_on else 'off')})"
    c = Checks(tag)
    with engine(engine_on), expect_path(want, tag):
        zs, hs, kld, kld_fn, mu_q, sd_q, mu_p, sd_p = cell.sequence(
            leaves["enc"], leaves.get("ctx"), (leaves["z0"], leaves["h0"]) if given else None, eps,
            r["x_sl"].to(DEV, dtype=torch.int32), STRIDE, r["free_nats"])  # fmt: skip
        ((zs[1:] * wz).sum() + (hs[1:] * wh).sum() + 0.7 * kld.sum() + 1.3 * kld_fn.sum()).backward()
    for k, got, rows in (("zs", zs[1:], 1), ("hs", hs[1:], 1), ("kld", kld, None), ("kld_fn", kld_fn, None), ("enc_mu", mu_q, 1),
                         ("enc_sd", sd_q, 1), ("prior_mu", mu_p, 1), ("prior_sd", sd_p, 1)):  # fmt: skip
        c.close("values", k, got, ref[k], BAR_VALUE, yard[k], row_dim=rows)
    if given:
        c.close("values", "zs[0]", zs[0], r["tensors"][3], 0.0)
        c.close("values", "hs[0]", hs[0], r["tensors"][4], 0.0)
    else:
        c.close("values", "zs[0] | hs[0]", torch.cat([zs[0], hs[0]], -1), torch.zeros(B, Z + H), 0.0)
    for k, leaf in leaves.items():
        assert leaf.grad is not None, k
        c.close("input gradients", f"d_{k}", leaf.grad, ref["grads"][k], BAR_GRAD, yard[f"d_{k}"], row_dim=leaf.dim() - 2)
    for k, p in cell.named_parameters():
        assert p.grad is not None, k
        c.close("parameter gradients", f"d_{k}", p.grad, ref["grads"][k], BAR_GRAD, yard[f"d_{k}"])
    c.done()


def per_link(T, given, tile):
    """Counter increments of one forward + backward on launch-per-link: 4 linear links per step each way, plus the d_z0 and
    d_h0 tail launches when an initial state is given."""
    n = 8 * T + (2 if given else 0)
    return [0, 1, 0, 1, n if tile == 16 else 0, n if tile == 32 else 0]


PROGRAM = [1, 0, 1, 0, 0, 0]


# ----------------------------------------------------------------------------------------------------------------------
# training cases
# ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["A", "B", "C"])
@pytest.mark.parametrize("engine_on", [False, True], ids=["engine_off", "engine_on"])
def test_rssm_cell_small_batch_both_arms_vs_oracle_float64(name, engine_on):
    """Cases A-C with the engine off (launch-per-link on 16x16 tiles: the RSSM's own step kernels at every NW, modes 0 / 1 / 2 of
    the shared head and dz kernels, C = 0 and a null initial state, the tail launches) and, same inputs and reference, with the
    engine on (the program)."""
    T, given = CASES[name][0], CASES[name][7]
    run_cell_case(name, engine_on, PROGRAM if engine_on else per_link(T, given, 16))


def test_rssm_cell_129_rows_on_32x32_tiles_vs_oracle_float64():
    """Case D, engine as found: B = 129 alone sends the call to launch-per-link, and every link (two segments at K = Z | H, three
    at 2Z | 2Z | 3H, one at 3H, the d_z0 and d_h0 tails) runs on 32x32 tiles; the last 32-row tile holds a single row."""
    run_cell_case("D", None, per_link(CASES["D"][0], True, 32))


def test_rssm_cell_129_rows_on_16x16_tiles_vs_oracle_float64():
    """Case E, engine as found: a large batch whose widths (H = 48, Z = 16) rule the 32x32 kernel out: nine row tiles of 16, the
    last one with one row."""
    run_cell_case("E", None, per_link(CASES["E"][0], True, 16))


# ----------------------------------------------------------------------------------------------------------------------
# generation (mode 3)
# ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("B,H,Z,C,engine_on,tile", [(5, 32, 16, 16, False, 16), (129, 64, 32, 32, None, 32)], ids=["B5_engine_off", "B129"])
def test_rssm_generate_sequence_per_link_vs_oracle_float64(B, H, Z, C, engine_on, tile):
    """`RSSMCell.generate_sequence` (mode 3 of the head kernel: z drawn from the prior) on launch-per-link, non-zero eps, a given
    state and context, against `rssm_generate_step` stepped in float64: zs and hs, rtol 1e-4 / atol 1e-5."""
    T, E = 4, 16
    torch.manual_seed(5)
    cell = RSSMCell(z_dim=Z, h_dim=H, c_dim=C, e_dim=E)
    gen = torch.Generator().manual_seed(6)
    ctx, eps = torch.randn(T, B, C, generator=gen), torch.randn(T, B, Z, generator=gen)
    z0, h0 = 0.3 * torch.randn(B, Z, generator=gen), 0.3 * torch.randn(B, H, generator=gen)
    sd64 = {k: v.detach().double() for k, v in cell.state_dict().items()}
    state, zs_r, hs_r = (z0.double(), h0.double()), [], []
    with torch.no_grad():
        for t in range(T):
            state = O.rssm_generate_step(sd64, state, ctx[t].double(), eps[t].double())
            zs_r.append(state[0]); hs_r.append(state[1])  # noqa: E702
    zs_r, hs_r = torch.stack(zs_r, 0), torch.stack(hs_r, 0)
    cell = cell.to(DEV)
    tag = f"rssm generate (T={T} B={B} H={H} Z={Z} C={C})"
    want = [0, 1, 0, 0, 4 * T if tile == 16 else 0, 4 * T if tile == 32 else 0]
    with engine(engine_on), expect_path(want, tag):
        zs, hs = cell.generate_sequence(ctx.to(DEV), (z0.to(DEV), h0.to(DEV)), eps.to(DEV), T, B)
    zs, hs = zs.double().cpu(), hs.double().cpu()
    print(f"{tag}: max |zs - ref| {float((zs[1:] - zs_r).abs().max()):.3e}, max |hs - ref| {float((hs[1:] - hs_r).abs().max()):.3e}, "
          f"rel_l2 zs {rel(zs[1:], zs_r):.3e} hs {rel(hs[1:], hs_r):.3e}")  # fmt: skip
    assert torch.equal(zs[0], z0.double()) and torch.equal(hs[0], h0.double())
    torch.testing.assert_close(zs[1:], zs_r, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(hs[1:], hs_r, rtol=1e-4, atol=1e-5)
    torch.cuda.synchronize()
    assert _hip.take_async_errors() == (0, 0)


# ----------------------------------------------------------------------------------------------------------------------
# model level: with_resets folds the bottom level onto launch-per-link
# ----------------------------------------------------------------------------------------------------------------------


def test_cwvae_with_resets_bottom_level_on_per_link_vs_oracle_float64():
    """CWVAEAudio with resets, B = 3, T = 368 (a multiple of 16: SURVEY quirk 8), x_sl = [368, 301, 97], free nats 0.5, precision-
    weighted posterior.  Level 0 (92 steps, a reset every 2) folds to 46 x 3 = 138 rows: launch-per-link in mode 2 on 32x32 tiles;
    level 1 (46 steps) folds to 69 rows and the top level has 3: the engine.  So one training step takes both arms in both
    directions.  Loss, per-utterance ELBO, log-likelihood, KL, the latents of all three levels and every parameter gradient against
    the float64 oracle, at the plain bars.  For scale, the oracle itself evaluated in fp32 (printed beside every figure) is within
    1.2e-6 (loss / ELBO / log-likelihood) and 1.4e-7 (KL, latents) of float64, but its gradients through the per-channel
    normalisations are ill-conditioned — up to 1.8e-3 from float64 (cells.2.gru_in.0.bias); the HIP path, whose normalisation
    statistics are accumulated in float64, stays below 1e-4 and is held to the 1e-3 bar without the fp32-yardstick allowance."""
    from blvm.models import CWVAEAudio

    kw = dict(z_size=[32, 16, 16], h_size=32, strides=[4, 2, 2], num_level_layers=2, stride_per_layer=2, likelihood="DMoL",
              num_bins=2**16, precision_posterior=True)  # fmt: skip
    torch.manual_seed(5)
    m = CWVAEAudio(**kw)
    m.cwvae.with_resets = True
    B, Tn = 3, 368
    x_sl = torch.tensor([368, 301, 97])
    x, _ = O.synth_batch(B, Tn, seed=6)
    gen = torch.Generator().manual_seed(7)
    T_l = [92, 46, 23]
    eps = [torch.randn(T_l[l], B, kw["z_size"][l], generator=gen) for l in range(3)]

    def oracle(dtype):
        sd = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in m.state_dict().items()}
        out = O.cwvae_audio_forward(sd, x.to(dtype), x_sl, [e.to(dtype) for e in eps], beta=1.0, free_nats=0.5, strides=kw["strides"],
                                    num_level_layers=2, stride_per_layer=2, num_bins=2**16, precision_posterior=True, with_resets=True)  # fmt: skip
        out["loss"].backward()
        return out, {k: v.grad for k, v in sd.items()}

    o64, g64 = oracle(torch.float64)
    o32, g32 = oracle(torch.float32)
    assert [int(z.shape[0]) for z in o64["z"]] == T_l

    m = m.to(DEV)
    tag = "cwvae with_resets (B=3 T=368)"
    with expect_path([2, 1, 2, 1, 0, 8 * 2], tag):  # levels 2 and 1 on the engine; level 0: 2 folded steps of 4 + 4 links, no tails
        loss, _, o = m(x.to(DEV), x_sl, beta=1.0, free_nats=0.5, eps=[e.to(DEV) for e in eps])
        loss.backward()
    c = Checks(tag)
    for k, got in (("loss", loss.reshape(1)), ("elbo", o.elbo), ("log_prob", o.log_prob)):
        got, ref = got.detach().double().cpu().reshape(-1), o64[k].detach().double().reshape(-1)
        err, y = float(((got - ref) / ref).abs().max()), float(((o32[k].detach().double().reshape(-1) - ref) / ref).abs().max())
        c.worst["loss / elbo"] = max(c.worst.get("loss / elbo", 0.0), err)
        print(f"{tag} {k}: max rel {err:.3e} (bar {BAR_MODEL:.0e}, fp32 oracle {y:.3e})")
        if not err <= BAR_MODEL:
            c.failures.append(f"{k}: max rel {err:.3e} > {BAR_MODEL:.0e}")
    c.close("values", "kld", o.kld, o64["kld"], BAR_VALUE, rel(o32["kld"], o64["kld"]))
    for l in range(3):
        ref = o64["z"][l].transpose(0, 1)
        c.close("values", f"z[{l}]", o.z[l], ref, BAR_VALUE, rel(o32["z"][l].transpose(0, 1), ref))
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        y = rel(g32[k], g64[k])
        c.close("parameter gradients", f"d_{k}", p.grad, g64[k], BAR_GRAD, y)
    c.done()
