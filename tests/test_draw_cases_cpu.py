"""CPU: the conditions the sampler tests (tests/test_gpu_samplers.py) rest on, asserted on the committed inputs of
tests/golden/samplers.npz with the float64 oracle alone: no kernel is involved.  If one of these failed, a GPU test could pass
without having reached the regime it is named after."""
import numpy as np
import pytest
import torch

import blvm_oracle as O
import draw_cases as DC

from conftest import GOLDEN


@pytest.fixture(scope="module")
def loaded():
    return DC.load(GOLDEN)


def detail(reg, kind, consts, floor=True):
    return O.mix_draw_detail(reg["par"], reg["u"], DC.noise(reg, kind), kind, *consts, floor=floor)


def test_undecided_caps_and_fp32_oracle_inside_the_bars(loaded):
    """Every case of the direct GPU test: the undecided share is within its cap (0.5 %; none in floor, saturation, ties), and the
    oracle's formulas evaluated in float32 by torch on the CPU meet the rule against their float64 selves, so the bars are wide
    enough for correct fp32 arithmetic without a look at the kernel."""
    regs, fx = loaded
    worst = {}
    for cid, reg, kind, consts in DC.direct_cases(regs, fx):
        v = DC.noise(reg, kind)
        res = DC.judge(reg["name"], DC.oracle32(reg["par"], reg["u"], v, kind, *consts), reg["par"], reg["u"], v, kind, *consts)
        DC.report(f"cpu fp32 oracle {cid}", res)
        worst[cid] = res["worst"]
        res = DC.judge(reg["name"], DC.oracle32(reg["par"], None, v, kind, *consts), reg["par"], None, v, kind, *consts)  # the mode's pick
        assert res["undecided"] == 0, cid
    assert max(worst.values()) <= 0.5, worst  # the bar is at least twice what fp32 torch needs


def test_saturation_clamps_and_trained_stays_inside(loaded):
    regs, fx = loaded
    d = detail(regs["saturation"], 0, DC.head_constants("saturation", 0, fx))
    assert float((d["pre"].abs() > 1 + 1e-3).double().mean()) >= 0.30
    assert bool((d["x"].abs() <= 1).all())
    d = detail(regs["trained"], 0, DC.head_constants("trained", 0, fx))
    assert float((d["x"].abs() < 1).double().mean()) >= 0.30
    for sgn in (-1, 1):  # both ends are reached
        assert int((sgn * d["pre"] > 1).sum()) > 0
    locs = regs["saturation"]["par"][:, 10:20].abs()
    assert sorted(set(np.float32(locs.reshape(-1).numpy()).tolist())) == sorted(float(np.float32(x)) for x in DC.SAT_LOCS)


def test_floor_rows_reach_the_floor(loaded):
    """Below the floor, removing it from the oracle moves the float64 value by more than 100 bars (raw <= -7.5) and by more than
    2 bars at raw = -7.001; at -7 and -6.999 the floor changes nothing by construction: those rows pin a floor set too HIGH (a floor
    of -6.9 moves them by more than 100 bars).  Nothing clamps, and |logit v| >= 3."""
    regs, fx = loaded
    reg, consts = regs["floor"], DC.head_constants("floor", 0, fx)
    c = DC.classify(reg["par"], reg["u"], reg["v"], 0, *consts)
    off = detail(reg, 0, consts, floor=False)
    raw = reg["par"][torch.arange(reg["par"].shape[0]), 20 + c["best"]].double()
    moved = (off["x"] - c["x"]).abs() / c["bar"]
    for value in DC.FLOOR_RAWS:
        rows = raw == float(np.float32(value))
        assert int(rows.sum()) >= 10, value
        if value <= -7.5:
            assert float(moved[rows].min()) > 100, (value, float(moved[rows].min()))
        elif value < -7.0:
            assert float(moved[rows].min()) > 2, (value, float(moved[rows].min()))
        else:
            assert float(moved[rows].max()) == 0
            high = O.mix_draw_detail(reg["par"], reg["u"], reg["v"], 0, -6.9)
            assert float(((high["x"] - c["x"]).abs() / c["bar"])[rows].min()) > 100
    v = reg["v"].double()
    assert float((torch.log(v) - torch.log1p(-v)).abs().min()) >= 3.0
    assert bool((c["pre"].abs() < 1).all())


def test_dominated_leader_is_overturned_sometimes(loaded):
    regs, fx = loaded
    reg = regs["dominated"]
    d = detail(reg, 0, DC.head_constants("dominated", 0, fx))
    lead = reg["par"][:DC.N_LEAD, :10].argmax(1)
    top2 = reg["par"][:DC.N_LEAD, :10].double().topk(2, dim=1).values
    assert torch.equal(top2[:, 0] - top2[:, 1], torch.full((DC.N_LEAD,), 8.0, dtype=torch.float64))
    wins = float((d["best"][:DC.N_LEAD] == lead).double().mean())
    assert 0.90 <= wins < 1.0, wins
    sharp = reg["par"][DC.N_LEAD:, :10].double()
    assert float((sharp.max(1).values - sharp.min(1).values).min()) >= 90
    g = regs["gmm_beta"]["par"][192:, :10].double()
    spread = g.max(1).values - g.min(1).values
    assert float(spread.min()) >= 60 and float(spread.max()) <= 125


def test_ties_are_structural_and_the_lower_index_wins(loaded):
    regs, fx = loaded
    reg = regs["ties"]
    par, u = reg["par"], reg["u"]
    assert bool((par[:64, :10] == par[:64, :1]).all()) and bool((u[:64] == u[:64, :1]).all())
    for rows, (a, b) in ((slice(64, 128), (3, 7)), (slice(128, 192), (0, 9))):
        assert torch.equal(par[rows, a], par[rows, b]) and torch.equal(u[rows, a], u[rows, b])
        others = [m for m in range(10) if m not in (a, b)]
        assert bool((par[rows][:, others].max(1).values < par[rows, a]).all())
    for uu in (None, u):
        c = DC.classify(par, uu, reg["v"], 0)
        assert int(c["undecided"].sum()) == 0
        assert bool((c["best"][:64] == 0).all()) and bool((c["runner"][:64] == 1).all())
        won = c["structural"]
        assert bool((c["best"][won] < c["runner"][won]).all())
        if uu is None:
            assert bool(won.all())
            assert bool((c["best"][64:128] == 3).all()) and bool((c["best"][128:] == 0).all())
        else:  # the tied pair wins most noisy draws; where a third component overtakes it the draw is an ordinary decided one
            assert int(won[64:].sum()) >= 64 and int((~won[64:]).sum()) >= 4


def test_ends_of_the_uniform_ranges(loaded):
    regs, fx = loaded
    reg = regs["ends"]
    assert set(np.unique(reg["u"].numpy()).tolist()) == set(float(x) for x in DC.END_U)
    assert set(np.unique(reg["v"].numpy()).tolist()) == set(float(x) for x in DC.END_V)
    d = detail(reg, 0, DC.head_constants("ends", 0, fx))
    inf = torch.isinf(d["pre"])
    assert torch.equal(inf, reg["v"] == 1.0) and int(inf.sum()) == 48
    assert bool((d["x"][inf] == 1.0).all()) and bool(torch.isfinite(d["x"]).all()) and bool((d["x"].abs() <= 1).all())


def test_gmm_scale_arms(loaded):
    """gmm_sd0: raw is a positive sd, the float64 activation of gmm_beta's raw rounded to fp32.  gmm_beta: rows 64..127 straddle the
    softplus's threshold beta raw = 20, rows 0..63 sit at the sd_eps floor."""
    regs, fx = loaded
    beta, eps = float(fx["gmm_beta"]), float(fx["gmm_sd_eps"])
    raw = regs["gmm_beta"]["par"][:, 20:]
    sd = regs["gmm_sd0"]["par"][:, 20:]
    assert bool((sd > 0).all())
    assert torch.equal(sd, (O.softplus_beta64(raw, beta) + eps).float())
    z = raw[64:128].double() * beta
    assert int((z > 20).sum()) > 50 and int((z <= 20).sum()) > 50
    assert bool(((sd[:64].double() - eps).abs() < 1e-3 * eps).all())
    assert torch.equal(regs["gmm_sd0"]["par"][:, :20], regs["gmm_beta"]["par"][:, :20])


def test_draw_site_cases_keep_the_caps(loaded):
    """The launches of the in-kernel draw sites: rows a >= 0 times a signed diagonal, every (regime, S, B, T) within its cap of
    undecided draws, the float32 oracle inside half the bars; the floor, saturation and ties rows still do what they are named after."""
    regs, fx = loaded
    for site, S, B, T in DC.SITE_SHAPES:
        todo = [(name, None) for name in DC.DMOL_REGIMES] if S > 1 else list(DC.SINGLE_ROWS)
        for name, first in todo:
            case = DC.site_case(regs[name], S, B, T, first)
            f = case["flat"]
            assert bool((case["a"] >= 0).all()) and tuple(f["par"].shape) == (T * B * S, 30) and tuple(f["u"].shape) == (T * B * S, 10)
            res = DC.judge(f["name"], DC.oracle32(f["par"], f["u"], f["v"], 0), f["par"], f["u"], f["v"], 0)
            assert res["worst"] <= 0.5, (site, name, res["worst"])
            d = res["detail"]
            if name == "floor":
                off = O.mix_draw_detail(f["par"], f["u"], f["v"], 0, floor=False)
                assert float(((off["x"] - d["x"]).abs() > 100 * d["bar"]).double().mean()) > 0.3
            if name == "saturation":
                assert float((d["pre"].abs() > 1 + d["bar"]).double().mean()) > 0.3
            if name == "ties":
                assert int(d["structural"].sum()) > 0.3 * d["structural"].numel() and bool((d["best"][d["structural"]] < d["runner"][d["structural"]]).all())


def test_the_rule_itself():
    """`judge` on hand-made draws: an undecided pick may go either way and counts against the cap, a decided one may not; beyond the
    clamp only exactly +-1 passes; a mode is the location bit for bit; a failure names the draw through `where`."""
    K = 10
    par = torch.zeros(4, 3 * K)
    par[:, :K] = -5.0
    par[:, K:2 * K] = torch.linspace(-0.9, 0.9, K)
    par[:, 2 * K:] = -4.0
    u = torch.full((4, K), 0.5)
    v = torch.full((4,), 0.5)
    par[0, 2], par[0, 6] = 1.0, 1.0 + 2.0**-20  # gap 1e-6: below 16 u (2 + ...) = 4e-6 -> undecided
    par[1, 2], par[1, 6] = 1.0, 1.001           # decided
    par[2, 4], par[2, K + 4], v[2] = 3.0, 0.999, 0.99  # beyond the clamp: 0.999 + e^-4 * 4.6
    par[3, 1] = 2.0
    d = DC.classify(par, u, v, 0)
    assert d["undecided"].tolist() == [True, False, False, False] and d["best"].tolist() == [6, 6, 4, 1]
    x = d["x"].float()
    ok = DC.judge("made", x, par, u, v, 0, cap=1.0)
    assert ok["undecided"] == 1 and ok["worst"] <= 1.0 and float(x[2]) == 1.0
    other = x.clone()
    other[0] = par[0, K + 2]  # the runner-up's value on the undecided draw
    DC.judge("made", other, par, u, v, 0, cap=1.0)
    with pytest.raises(AssertionError, match="undecided"):
        DC.judge("made", x, par, u, v, 0, cap=0.0)
    wrong = x.clone()
    wrong[1] = par[1, K + 2]  # the runner-up's value on a decided draw
    with pytest.raises(AssertionError, match="draw row 1"):
        DC.judge("made", wrong, par, u, v, 0, cap=1.0, where=lambda i: f"row {i}")
    near = x.clone()
    near[2] = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    with pytest.raises(AssertionError, match="draw 2"):
        DC.judge("made", near, par, u, v, 0, cap=1.0)
    off = x.clone()
    off[3] = off[3] + 4 * float(d["bar"][3])
    with pytest.raises(AssertionError, match="draw 3"):
        DC.judge("made", off, par, u, v, 0, cap=1.0)
    mode = DC.classify(par, None, None, 0)
    assert mode["best"].tolist() == [6, 6, 4, 1]
    loc = par[torch.arange(4), K + mode["best"]]
    DC.judge("made", loc, par, None, None, 0, cap=1.0)
    with pytest.raises(AssertionError):
        DC.judge("made", loc + 2.0**-24, par, None, None, 0, cap=1.0)


def test_fixture_holds_the_rows_build_makes(loaded):
    """The crafted rows and draws of samplers.npz are `draw_cases.build` on heads_stress.npz, bit for bit: the regimes are defined in one
    place.  What the reference drew (u, v where a regime does not craft them, the Gaussian mixtures' n) is only in the fixture."""
    import os

    regs, fx = loaded
    built = DC.build(np.load(os.path.join(GOLDEN, "heads_stress.npz")))
    assert set(built) == set(DC.DMOL_REGIMES + DC.GMM_REGIMES)
    for name, r in built.items():
        for key, value in r.items():
            assert torch.equal(value, regs[name][key]), (name, key)
        assert tuple(regs[name]["u"].shape) == (r["par"].shape[0], 10) and regs[name]["n"].shape[0] == r["par"].shape[0]
    for name in ("saturation", "dominated", "trained"):  # drawn as the reference draws them: inside its open ranges' fp32 images
        u, v = regs[name]["u"], regs[name]["v"]
        assert float(u.min()) >= np.float32(1e-5) and float(u.max()) <= np.float32(1 - 1e-5) and float(v.min()) >= np.float32(1e-8) and float(v.max()) <= 1.0
