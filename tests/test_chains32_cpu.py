"""CPU: what tests/test_gpu_chains32.py relies on, established with the float32 stand-in (the oracle of tests/chains32.py evaluated in
float32, one thread) in the kernel's place.

  * The recorded table tests/golden/chains32_bars.json is reproduced entry by entry: the seed exactly (float64 decides it); KINK32
    between 3 and 6 times the stand-in's largest |pre(float32) - pre(float64)| measured here (recorded at 4 x; the float32 sums of
    another host may differ); every gradient bar, per tensor and per batch row, at least 4 x the stand-in's worst distance measured
    here, at most the larger of 2e-5 and 5 x that distance, and never above 1e-4.
  * Every case: at most 1/4 of the rows are left out at a kink, never all rows of a 16-row tile, never row 0, row 1, the last row or
    the first row of the last tile; between 1/4 and 3/4 of the live KL elements lie above the free-nats floor; the lengths hold a
    full row, a row that ends before the last step and one whose length is an exact multiple of the stride (T' >= 3).
  * The stand-in itself passes `chains32.judge` on every forward and backward case.
  * The pins bite: each of seven weakenings of the stand-in fails `judge` on every case it applies to.  Whether the weakened
    gradients would still pass the 1e-3 per-tensor bar of the model-level tests is printed beside each."""
import contextlib

import pytest
import torch

import blvm_oracle as O
import chains32 as C
import links16 as L


@pytest.mark.parametrize("ct", C.BWD_CASES, ids=C.case_id)
def test_recorded_table_is_reproduced(ct):
    c, Tp = ct
    e = C.table()[C.case_id(ct)]
    m = C.measure(ct, e["kink32"])
    assert m["seed"] == e["seed"], (m["seed"], e["seed"])
    assert 0.75 * m["kink32"] <= e["kink32"] <= 1.5 * m["kink32"], (e["kink32"], m["kink32"])
    for kind, floor in (("bars", m["floor"]), ("row_bars", m["row_floor"])):
        assert set(e[kind]) == set(floor), (kind, sorted(set(e[kind]) ^ set(floor)))
        for n, v in floor.items():
            bar = e[kind][n]
            assert L.FP32_GRAD_BAR <= bar <= C.MAX_BAR, (kind, n, bar)
            assert C.STANDIN_FACTOR * v <= bar <= max(L.FP32_GRAD_BAR, 5 * v), (kind, n, bar, v)
    print(f"{C.case_id(ct)}: kink32 {e['kink32']:.1e} (here {m['kink32']:.1e}), seed {e['seed']}, stand-in worst tensor {max(m['floor'].values()):.2e}, "
          f"worst batch row {max(m['row_floor'].values()):.2e}")  # fmt: skip


def _lengths_hold(inp, Tp, B):
    sl = C.ragged_lengths(Tp, B)
    steps = torch.div(sl + C.STRIDE - 1, C.STRIDE, rounding_mode="floor")
    assert int(sl[0]) == Tp * C.STRIDE and int(sl.min()) >= 1 and int(steps.max()) == Tp
    if Tp >= 3:
        assert bool((steps < Tp).any()) and int(sl[1]) % C.STRIDE == 0 and int(sl[1]) < Tp * C.STRIDE
    live = inp["lens"] > 0
    assert torch.equal(inp["lens"][live], sl[live])


@pytest.mark.parametrize("ct", C.BWD_CASES, ids=C.case_id)
def test_backward_case_conditions_and_standin(ct):
    c, Tp = ct
    inp, free_nats, share, e = C.backward_case(ct)
    near = inp["near_kink"]
    assert C.kink_conditions(near) == []
    assert bool((inp["w"][:, near] == 0).all()) and bool((inp["lens"][near] == 0).all())
    assert 0.25 <= share <= 0.75, share
    _lengths_hold(inp, Tp, c.B)
    with C.one_thread():
        stand, ref = C.standin_result(c, inp, free_nats)
    fails, fig = C.judge(c, Tp, stand, ref, inp, e)
    print(f"{C.case_id(ct)}: {int(near.sum())} of {c.B} rows left out, {share:.3f} of the live KL elements above the floor; stand-in: worst value row "
          f"{fig['row']:.2e}, KL element {fig['kl']:.2e}, gradient tensor {fig['tensor']:.2e}, batch row {fig['grad_row']:.2e}")  # fmt: skip
    assert not fails, fails


@pytest.mark.parametrize("ct", C.FWD_CASES, ids=C.case_id)
def test_forward_case_conditions_and_standin(ct):
    c, Tp = ct
    inp, free_nats, share = C.inputs(c, Tp)
    assert 0.25 <= share <= 0.75, share
    _lengths_hold(inp, Tp, c.B)
    with C.one_thread(), torch.no_grad():
        stand = C.oracle(c, inp, torch.float32, free_nats=free_nats)
        ref = C.oracle(c, inp, forced_stats=stand, free_nats=free_nats)
    fails, fig = C.judge(c, Tp, stand, ref, inp)
    print(f"{C.case_id(ct)}: {share:.3f} of the live KL elements above the floor; stand-in: worst value row {fig['row']:.2e}, KL element {fig['kl']:.2e}")
    assert not fails, fails


# ----------------------------------------------------------------------------------------------------------------------
# the pins bite
# ----------------------------------------------------------------------------------------------------------------------


@contextlib.contextmanager
def spy_on(bias, fn):
    """Inside the block every product of the oracle that adds `bias` (a float32 [N] tensor, by value) has its output passed through
    fn(call index, output); -> the list of what fn returned."""
    orig, calls = O.rounded_linear, []

    def spy(x, W, b, rnd, rnd_wgrad=None):
        y = orig(x, W, b, rnd, rnd_wgrad)
        if b is not None and b.shape == bias.shape and torch.equal(b.detach().float(), bias):
            y = fn(len(calls), y)
            calls.append(y)
        return y

    O.rounded_linear = spy
    try:
        yield calls
    finally:
        O.rounded_linear = orig


def mutants(c, Tp, inp, free_nats, stand):
    """(name, result dict) of every weakening that applies to the case."""
    B, H = c.B, c.H
    run = lambda **kw: C.oracle(c, kw.pop("inp", inp), torch.float32, backward=True, free_nats=free_nats, **kw)  # noqa: E731
    if Tp >= 3:  # the KL mask `t * stride <= x_sl` on row 1, whose length is an exact multiple of the stride
        longer = dict(inp, lens=inp["lens"].clone())
        longer["lens"][1] += 1
        yield "KL mask <= on one row", run(inp=longer)
    if c.residual and B % 16:  # the residual add dropped on the last row of the partial tile (batch rows are independent: splice)
        plain, got = run(residual=False), dict(stand)
        for k in ("decin", "zs", "z", "mu_q", "sd_q", "mu_p", "sd_p"):
            if k in got:
                got[k] = got[k].clone()
                got[k][:, B - 1] = plain[k][:, B - 1]
        yield "residual add dropped on the last row", got
    yield "KL coefficients swapped", run(coef=C.COEF[::-1])
    if c.given:  # the recurrent term missing from the initial state's gradient: only the direct term is left
        got = dict(stand)
        if c.family == "vrnn":
            got["d_h0"] = inp["w"][0, :, H:].clone()
        else:
            got["d_z0"] = torch.zeros(B, c.Z)
        yield "recurrent term missing from the initial state's gradient", got
    bias = inp["prior_b1"]
    with spy_on(bias, lambda k, y: y.retain_grad() or y) as calls:
        with torch.enable_grad():
            again = run()
    got = dict(again)
    got["d_prior_b1"] = again["d_prior_b1"] - calls[0].grad[0]  # row (t = 0, b = 0)
    yield "one (t, b) row missing from a bias gradient", got

    def wrong_branch(k, y):
        if k == 0:
            j = int((y[0] > 0).nonzero()[0])
            scale = torch.ones_like(y)
            scale[0, j] = 0.0 if c.family == "vrnn" else 0.01  # ReLU | LeakyReLU(0.01): the other branch's derivative
            y.register_hook(lambda g: g * scale)
        return y

    with spy_on(bias, wrong_branch):
        yield "one unit's derivative on the wrong branch", run()
    if not c.residual:
        yield "plain posterior computed as residual", run(residual=True)


@pytest.mark.parametrize("ct", C.BWD_CASES, ids=C.case_id)
def test_every_weakening_fails_the_bars(ct):
    c, Tp = ct
    inp, free_nats, _, e = C.backward_case(ct)
    survivors = []
    with C.one_thread():
        stand, ref = C.standin_result(c, inp, free_nats)
        for name, got in mutants(c, Tp, inp, free_nats, stand):
            fails, fig = C.judge(c, Tp, got, ref, inp, e)
            print(f"{C.case_id(ct)} | {name}: {len(fails)} misses (first: {fails[0] if fails else '-'}); worst gradient tensor {fig['tensor']:.2e}: "
                  f"{'passes' if fig['old_bar'] else 'fails'} the 1e-3 per-tensor bar")  # fmt: skip
            if not fails:
                survivors.append(name)
    assert not survivors, survivors
