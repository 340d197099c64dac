"""`blvm_oracle.rounded_linear` (the contract of one product in a 16-bit operand mode), the teacher-forced sequence oracles built from
it, and the stand-in measurements behind the bars of tests/test_gpu_16bit_links.py: the same oracle evaluated free-running in
float32 takes the kernel's place, for exactly the cases and inputs the GPU file runs (tests/links16.py), over STANDIN_SEEDS seeds."""
import pytest
import torch
import torch.nn.functional as F

import blvm_oracle as O
import links16 as L

F64 = torch.float64
IDENT = O.operand_rounding("f32")


def _leaves(seed, n=37, K=24, N=40, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(s, generator=g) * scale).double().requires_grad_(True) for s in ((n, K), (N, K), (N,))], torch.randn(n, N, generator=g).double() * scale


def _bits_equal(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_identity_is_linear_and_its_autograd_bit_for_bit():
    (x, W, b), w = _leaves(0)
    y = O.rounded_linear(x, W, b, IDENT)
    got = torch.autograd.grad((y * w).sum(), (x, W, b))
    y_ref = F.linear(x, W, b)
    ref = torch.autograd.grad((y_ref * w).sum(), (x, W, b))
    assert _bits_equal(y, y_ref)
    for a, r in zip(got, ref):
        assert _bits_equal(a, r)
    y0 = O.rounded_linear(x, W, None, IDENT)  # no bias
    assert _bits_equal(y0, F.linear(x, W))


@pytest.mark.parametrize("mode,dt", [("bf16", torch.bfloat16), ("f16", torch.float16)])
def test_rounded_modes_are_the_explicit_formulas(mode, dt):
    rnd = O.operand_rounding(mode)
    (x, W, b), w = _leaves(1)
    r = lambda t: t.detach().float().to(dt).double()  # noqa: E731
    y = O.rounded_linear(x, W, b, rnd)
    dx, dW, db = torch.autograd.grad((y * w).sum(), (x, W, b))
    assert _bits_equal(y.detach(), r(x) @ r(W).t() + b.detach())
    assert _bits_equal(dx, r(w) @ r(W))
    assert _bits_equal(dW, r(w).t() @ r(x))
    assert _bits_equal(db, w.sum(0))  # the UNROUNDED upstream gradient
    assert not torch.equal(db, r(w).sum(0))
    assert not torch.equal(y.detach(), F.linear(x, W, b).detach())  # and the rounding is really there


def test_bias_gradient_ignores_rnd():
    (x, W, b), w = _leaves(2)
    dbs = [torch.autograd.grad((O.rounded_linear(x, W, b, O.operand_rounding(m)) * w).sum(), b)[0] for m in ("f32", "bf16", "f16")]
    assert _bits_equal(dbs[0], dbs[1]) and _bits_equal(dbs[0], dbs[2]) and _bits_equal(dbs[0], w.sum(0))


def test_weight_gradient_rounding_of_a_launch_per_step_arm():
    """rnd the identity, rnd_wgrad the mode's: the product and its data gradient are F.linear's, dW multiplies rounded operands."""
    rnd = O.operand_rounding("bf16")
    (x, W, b), w = _leaves(3)
    y = O.rounded_linear(x, W, b, IDENT, rnd)
    dx, dW, db = torch.autograd.grad((y * w).sum(), (x, W, b))
    assert _bits_equal(y.detach(), F.linear(x, W, b).detach())
    assert _bits_equal(dx, w @ W.detach())
    assert _bits_equal(dW, rnd(w).t() @ rnd(x.detach()))
    assert _bits_equal(db, w.sum(0))


def test_rounding_is_torchs_conversion_at_the_edges():
    v = torch.tensor([65519.0, 65520.0, -7e4, 6.0e-5, 1e-7, 2.9e-8, 1.0 + 2.0**-11, 1.0 + 2.0**-11 + 2.0**-20, 1.0 + 3 * 2.0**-11])
    h = O.operand_rounding("f16")(v.double())
    assert h.dtype == F64 and torch.equal(h, v.half().double())
    assert h.tolist()[:3] == [65504.0, float("inf"), float("-inf")]  # overflow goes to inf, never saturates
    assert float(h[4]) == 2 * 2.0**-24 and float(h[5]) == 0.0  # subnormals are kept, to the grid of 2^-24
    assert h.tolist()[6:] == [1.0, 1.0 + 2.0**-10, 1.0 + 2.0**-9]  # ties to even, above the tie up
    b = O.operand_rounding("bf16")(torch.tensor([1.0 + 2.0**-8, 1.0 + 3 * 2.0**-8, 3.0e38], dtype=F64))
    assert b.tolist()[:2] == [1.0, 1.0 + 2.0**-6] and float(b[2]) == float(torch.tensor(3.0e38).bfloat16())


@pytest.mark.parametrize("family", ["lstm", "gru"])
def test_unrounded_sequence_oracles_are_the_existing_references(family):
    """With rnd the identity the new time loops are `lstm_sequence_ref` / `gru_sequence` (between reverse_sequences), values and
    gradients."""
    if family == "lstm":
        case = L.LSTM_CASES[0]
        inp = L.lstm_inputs(case)
        got = L.lstm_oracle(inp, "f32", case[4])
        lv = {n: inp[n].double().requires_grad_(True) for n in L.LSTM_GRADS}
        out, hn, cn = O.lstm_sequence_ref(lv["x"], lv["h0"], lv["c0"], inp["lens"], lv["Wih"], lv["Whh"], lv["bih"], lv["bhh"])
        ref = dict(out=out, h_n=hn, c_n=cn)
        names = L.LSTM_GRADS
    else:
        case = L.GRU_CASES[1]  # reversed
        inp = L.gru_inputs(case)
        got = L.gru_oracle(inp, "f32", case[4], True)
        lv = {n: inp[n].double().requires_grad_(True) for n in L.GRU_GRADS}
        out, hn = O.gru_sequence(O.reverse_sequences(lv["x"], inp["lens"]), lv["h0"], lv["Wih"], lv["Whh"], lv["bih"], lv["bhh"])
        out = O.reverse_sequences(out, inp["lens"])
        ref = dict(out=out, h_n=hn)
        names = L.GRU_GRADS
    (out * inp["w"].double()).sum().backward()
    for k, v in ref.items():
        assert L.rel_l2(got[k], v) < 1e-14, k
    for n in names:
        assert L.rel_l2(got["d_" + n], lv[n].grad) < 1e-13, n


def _same(free, forced):
    for k in free:
        if k.startswith("d_"):
            assert L.rel_l2(forced[k], free[k]) < 1e-14, k
        else:
            assert _bits_equal(free[k], forced[k]), k


@pytest.mark.parametrize("mode", L.MODES)
def test_teacher_forcing_keeps_the_value_and_the_gradient_path(mode):
    """Forced with its own free-running out the oracle returns the same values bit for bit (value + (own - own.detach()) is the value)
    and the same gradients up to the order of their sums (the gradient path is own's); forced with other values the next step starts
    from THOSE values."""
    case = L.LSTM_CASES[0]
    inp = L.lstm_inputs(case)
    free = L.lstm_oracle(inp, mode, case[4])
    own = L.lstm_oracle(inp, mode, case[4], forced_out=free["out"])
    _same(free, own)
    gcase = L.GRU_CASES[3]
    ginp = L.gru_inputs(gcase)
    gfree = L.gru_oracle(ginp, mode, gcase[4], True)
    gown = L.gru_oracle(ginp, mode, gcase[4], True, forced_out=gfree["out"])
    _same(gfree, gown)
    # other values: step t + 1 is one cell step from them
    fcase = L.GRU_CASES[0]
    finp = L.gru_inputs(fcase)
    forced = torch.randn(finp["w"].shape, generator=torch.Generator().manual_seed(5)).double()
    got = L.gru_oracle(finp, mode, fcase[4], False, forced_out=forced)
    rnd = O.operand_rounding(mode)
    p = {n: finp[n].double() for n in L.GRU_GRADS}
    gi, gh = F.linear(rnd(p["x"][2]), rnd(p["Wih"]), p["bih"]), F.linear(rnd(forced[1]), rnd(p["Whh"]), p["bhh"])
    (i_r, i_z, i_n), (h_r, h_z, h_n) = gi.chunk(3, -1), gh.chunk(3, -1)
    z = torch.sigmoid(i_z + h_z)
    step = (1 - z) * torch.tanh(i_n + torch.sigmoid(i_r + h_r) * h_n) + z * forced[1]  # the carried h itself is not rounded
    assert L.rel_l2(got["out"][2], step) < 1e-14


def _standin(family, case, mode, seed):
    inputs, oracle = (L.lstm_inputs, L.lstm_oracle) if family == "lstm" else (L.gru_inputs, L.gru_oracle)
    kw = dict(arm=case[4]) if family == "lstm" else dict(arm=case[4], reverse=case[5])
    inp = inputs(case, seed)
    stand = oracle(inp, mode, dtype=torch.float32, **kw)  # in the kernel's place: free-running, float32
    ref = oracle(inp, mode, forced_out=stand["out"], **kw)
    unr = oracle(inp, "f32", **kw)
    return stand, ref, unr


@pytest.fixture
def one_thread():
    """The float32 stand-in's sums in one fixed order."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


CASES = [("lstm", c) for c in L.LSTM_CASES] + [("gru", c) for c in L.GRU_CASES]


@pytest.mark.parametrize("mode", L.MODES)
@pytest.mark.parametrize("family,case", CASES, ids=[f"{f}-{(L.lstm_id if f == 'lstm' else L.gru_id)(c)}" for f, c in CASES])
def test_standin_floors_and_bars(family, case, mode, one_thread):
    """The conditions on the bars of the GPU file, for its cases and inputs (seed 0 is the GPU file's):
      forward: every (t, b) row of the stand-in is 10 times under the tight bar;
      each gradient bar is at least 3 x the stand-in's largest distance and at most half the smallest rounded-vs-unrounded distance;
      the loose multiple is at least twice the stand-in's worst batch row, in median row distances between the two oracles;
      the stand-in itself is at least MODE_ON times closer to the rounded oracle."""
    names = L.LSTM_GRADS if family == "lstm" else L.GRU_GRADS
    T_, B, arm = case[0], case[1], case[4]
    floor, dist = {n: 0.0 for n in names}, {n: float("inf") for n in names}
    fwd = worst_row = 0.0
    for seed in range(L.STANDIN_SEEDS):
        stand, ref, unr = _standin(family, case, mode, seed)
        fwd = max(fwd, float(L.row_dist(stand["out"].reshape(T_ * B, -1), ref["out"].reshape(T_ * B, -1), 0).max()))
        assert L.MODE_ON * L.rel_l2(stand["out"], ref["out"]) <= L.rel_l2(stand["out"], unr["out"])
        for n in names:
            floor[n] = max(floor[n], L.rel_l2(stand["d_" + n], ref["d_" + n]))
            dist[n] = min(dist[n], L.rel_l2(ref["d_" + n], unr["d_" + n]))
            if n in L.ROW_GRADS:
                rows = L.row_dist(stand["d_" + n], ref["d_" + n], L.row_dim_of(n))
                worst_row = max(worst_row, float(rows.max()) / (L.loose_bar(ref, unr, n) / L.LOOSE_MULTIPLE))
    print(f"{family} {case} {mode}: forward rows {fwd:.2e}, worst gradient row {worst_row:.2f} medians; "
          + "  ".join(f"d_{n} floor {floor[n]:.1e} bar {L.grad_bar(family, mode, arm, n):.1e} mode {dist[n]:.1e}" for n in names))
    assert fwd <= L.BAR_VALUE / 10
    assert 2 * worst_row <= L.LOOSE_MULTIPLE, worst_row
    for n in names:
        bar = L.grad_bar(family, mode, arm, n)
        assert 3 * floor[n] <= bar, (n, floor[n], bar)
        assert bar <= dist[n] / 2, (n, bar, dist[n])


def test_wavenet_block_oracle_unrounded_is_the_convolution_stack():
    """rnd the identity: conv1d (dilated, kernel 2) -> tanh * sigmoid -> 1x1 conv, the last T_skip frames of its skip rows."""
    case = L.WN_CASES[0]
    C, B, L_, d, T_skip = case
    inp = L.wn_inputs(case)
    got = L.wn_oracle(inp, "f32", case)
    lv = {n: inp[n].double().requires_grad_(True) for n in ("x",) + L.WN_PARAMS}
    pre = F.conv1d(lv["x"].permute(1, 2, 0), lv["conv_w"], lv["conv_b"], dilation=d)
    rs = F.conv1d(torch.tanh(pre[:, :C]) * torch.sigmoid(pre[:, C:]), lv["rs_w"].unsqueeze(-1), lv["rs_b"])
    skip = rs[:, C:, -T_skip:].permute(2, 0, 1)
    (skip * inp["w"].double()).sum().backward()
    assert L.rel_l2(got["skip"], skip) < 1e-14
    assert L.rel_l2(got["d_x"], lv["x"].grad) < 1e-13 and L.rel_l2(got["d_conv_w"], lv["conv_w"].grad) < 1e-13
    assert L.rel_l2(got["d_conv_b"], lv["conv_b"].grad) < 1e-13
    assert L.rel_l2(got["d_rs_w"], lv["rs_w"].grad[C:]) < 1e-13 and L.rel_l2(got["d_rs_b"], lv["rs_b"].grad[C:]) < 1e-13


@pytest.mark.parametrize("mode", L.MODES)
@pytest.mark.parametrize("case", L.WN_CASES, ids=L.wn_id)
def test_wavenet_standin_floors_and_bars(case, mode, one_thread):
    """The WaveNet block of the GPU file: the float32 stand-in's rows stay under the loose bar with the multiple at least twice its
    worst flipped row; with the GPU file's seed (0) it uses at most half of the caps on all rows and on a row tile (a tile with one
    flip aside), and at most floor(T / 2) - 1 steps of a batch row; the per-tensor bars sit between 3 x the floor and half the mode's distance (d_rs_b: no
    product, so no distance, and the fp32 bar)."""
    names = ("x",) + L.WN_PARAMS
    floor, dist, worst = {n: 0.0 for n in names}, {n: float("inf") for n in names}, 0.0
    for seed in range(L.STANDIN_SEEDS):
        inp = L.wn_inputs(case, seed)
        stand, ref, unr = L.wn_oracle(inp, mode, case, torch.float32), L.wn_oracle(inp, mode, case), L.wn_oracle(inp, "f32", case)
        assert L.MODE_ON * L.rel_l2(stand["skip"], ref["skip"]) <= L.rel_l2(stand["skip"], unr["skip"])
        for name, tight in (("skip", L.BAR_VALUE), ("d_x", L.WN_BAR_DX)):
            fails, fig = L.two_tier(stand[name], ref[name], unr[name], tight, L.WN_LOOSE_MULTIPLE, L.WN_TILE, 2 if name == "d_x" else 1)
            worst = max(worst, fig["worst_over_in_medians"])
            assert fig["worst"] <= fig["loose"]
            if seed == 0:
                assert not fails, fails
                assert fig["share"] <= 1 / 16 and fig["group_fill"] <= 1 / 2 and fig["row_steps"] <= fig["steps"] // 2 - 1, fig
        for n in names:
            floor[n] = max(floor[n], L.rel_l2(stand["d_" + n], ref["d_" + n]))
            dist[n] = min(dist[n], L.rel_l2(ref["d_" + n], unr["d_" + n]))
    print(f"wavenet {case} {mode}: worst flipped row {worst:.2f} medians; " + "  ".join(f"d_{n} floor {floor[n]:.1e} bar {L.WN_GRAD_BAR[mode][n]:.1e} mode {dist[n]:.1e}" for n in names))
    assert 2 * worst <= L.WN_LOOSE_MULTIPLE
    for n in names:
        bar = L.WN_GRAD_BAR[mode][n]
        assert 3 * floor[n] <= bar, (n, floor[n], bar)
        if n == "rs_b":
            assert dist[n] == 0.0 and bar == 2e-5
        else:
            assert bar <= dist[n] / 2, (n, bar, dist[n])


@pytest.mark.parametrize("mode", L.MODES)
@pytest.mark.parametrize("case", L.SRNN_CASES, ids=L.srnn_id)
def test_srnn_standin_forward_conditions(case, mode, one_thread):
    """The SRNN chain of the GPU file, forward: with the case's seed the float32 stand-in passes the two-tier rule using at most half
    of the caps on all rows and on a step's rows (a step with one flip aside) and at most floor(T' / 2) - 1 steps of a batch row; over
    seeds 0 .. 4 the loose multiple is at least twice its worst flipped row; the mode is on."""
    worst = 0.0
    chosen = L.SRNN_SEED.get(case, 0)
    for seed in sorted(set(range(L.STANDIN_SEEDS)) | {chosen}):
        inp = L.srnn_inputs(case, seed)
        stand = L.srnn_oracle(inp, mode, case, torch.float32)
        ref, unr = L.srnn_oracle(inp, mode, case, forced_zs=stand["zs"]), L.srnn_oracle(inp, "f32", case)
        e_r, e_u = L.median_row_distances(stand["zs"][1:], ref["zs"][1:], unr["zs"][1:])
        assert L.MODE_ON * e_r <= e_u, (e_r, e_u)
        for name in L.SRNN_STATS:
            g, r, u = (x[name][1:] if name == "zs" else x[name] for x in (stand, ref, unr))
            fails, fig = L.two_tier(g, r, u, L.BAR_VALUE, L.SRNN_LOOSE_MULTIPLE)
            if seed < L.STANDIN_SEEDS:
                worst = max(worst, fig["worst_over_in_medians"])
            if seed == chosen:
                assert not fails, (name, fails)
                assert fig["share"] <= 1 / 16 and fig["group_fill"] <= 1 / 2 and fig["row_steps"] <= case[0] // 2 - 1, (name, fig)
    print(f"srnn {case} {mode}: worst flipped row {worst:.2f} medians")
    assert 2 * worst <= L.SRNN_LOOSE_MULTIPLE


@pytest.mark.parametrize("mode", L.MODES)
@pytest.mark.parametrize("fc", L.BWD_CASES, ids=L.bwd_id)
def test_chain_standin_backward_conditions(fc, mode):
    """The backward cases of the GPU file (T' = 2): every bar is at least 3 x the float32 stand-in's largest distance at that case and
    at most half the smallest distance between the rounded and the unrounded oracle; the tensors without a bar are those for which no
    such bar exists; the row multiples are at least twice the stand-in's worst rows."""
    family, case = fc
    floor, dist, worst = L.bwd_standin(family, case, mode)
    bars, without = L.bwd_bars(family, case, mode)
    assert set(bars) | set(without) == set(dist) and not set(bars) & set(without)
    for n, bar in bars.items():
        assert 3 * floor[n] <= bar <= dist[n] / 2, (n, floor[n], bar, dist[n])
        assert bar >= L.FP32_GRAD_BAR
    print(f"{L.bwd_id(fc)} {mode}: worst row {worst:.2f} medians; without a bar: {without}; " + "  ".join(f"d_{n} {floor[n]:.1e}/{bars[n]:.1e}/{dist[n]:.1e}" for n in bars))
    assert 2 * worst <= L.BWD_LOOSE_MULTIPLE, worst
    assert 3 * L.one_flip(case, mode) <= min(bars.values(), default=1.0)
    if case[1] >= 49:  # the larger batches are there so that most tensors have a bar (the B = 5 shapes have none: 10 rows)
        assert len(bars) >= 3 and (mode == "f16" or 2 * len(bars) > len(dist)), (len(bars), without)


def test_chain_backward_rows_rule():
    """Every batch row is held to the loose multiple: one row off by a percent fails by its index; so does a non-finite row."""
    fc = ("srnn", L.SRNN_CASES[4])
    inp = L.bwd_inputs(*fc)
    ref, unr = L.bwd_oracle(fc[0], inp, "f16", fc[1]), L.bwd_oracle(fc[0], inp, "f32", fc[1])
    assert L.bwd_rows(fc[0], ref, ref, unr) == ([], 0.0)
    bad = {k: v.clone() for k, v in ref.items()}
    live = int((~inp["near_kink"]).nonzero()[-1])
    bad["d_d"][:, live] *= 1.01
    fails, worst = L.bwd_rows(fc[0], bad, ref, unr)
    assert len(fails) == 1 and f"d_d row {live}:" in fails[0] and worst > L.BWD_LOOSE_MULTIPLE
    bad["d_z0"][live] = float("nan")
    assert any("non-finite" in f for f in L.bwd_rows(fc[0], bad, ref, unr)[0])


def test_recorded_backward_bars_cover_every_case():
    """tests/golden/links16_bwd_bars.json has an entry per backward case and mode, names only gradients the case has, and holds the
    counts the documents state: 735 (bf16) and 392 (fp16) of 1083 tensors have a bar."""
    n = {m: 0 for m in L.MODES}
    for fc in L.BWD_CASES:
        for mode in L.MODES:
            bars, without = L.bwd_bars(fc[0], fc[1], mode)
            assert set(bars) <= set(L.bwd_grad_names(*fc)) and len(bars) + len(without) == len(L.bwd_grad_names(*fc))
            n[mode] += len(bars)
    assert len(L._frozen_bars()) == 2 * len(L.BWD_CASES) and n == {"bf16": 735, "f16": 392}
    assert sum(len(L.bwd_grad_names(*fc)) for fc in L.BWD_CASES) == 1083


def test_near_kink_rows_are_bounded():
    """The rows that `links16.bwd_inputs` gives no loss (a hidden pre-activation within KINK of zero): at most half of a case's
    rows, at most a fifth of all (measured: 366 of 2422, 15 %; the most in one case 28 of 61, at H = 128 where a row has 1792 hidden
    units), and never the whole last row tile, so that every tile position keeps a row that is compared."""
    masked = total = 0
    for fc in L.BWD_CASES:
        near = L.bwd_inputs(*fc)["near_kink"]
        B = fc[1][1]
        masked, total = masked + int(near.sum()), total + B
        assert 2 * int(near.sum()) <= B, (L.bwd_id(fc), int(near.sum()))
        assert not bool(near[16 * ((B - 1) // 16):].all()) and not bool(near[:16].all()), L.bwd_id(fc)
    print(f"rows without loss: {masked} of {total}")
    assert 5 * masked <= total


def test_two_tier_rejects_non_finite_values():
    ref = torch.randn(6, 5, 4, dtype=F64)
    got = ref.clone()
    got[2, 1, 0] = float("nan")
    assert L.two_tier(ref, ref, ref * 1.001, 1e-5, 2.0)[0] == []
    assert L.two_tier(got, ref, ref * 1.001, 1e-5, 2.0)[0] == ["non-finite values"]


@pytest.mark.parametrize("mode", L.MODES)
@pytest.mark.parametrize("case", L.VRNN_CASES, ids=L.vrnn_id)
def test_vrnn_standin_forward_conditions(case, mode, one_thread):
    """The VRNN sequence of the GPU file: the strict piece (the GRU cell from stored phi and h) sits 10 times under the tight bar in
    every row; the two-tier pieces meet the conditions of `test_srnn_standin_forward_conditions` with the case's seed."""
    H, worst = case[2], 0.0
    chosen = L.VRNN_SEED.get(case, 0)
    for seed in sorted(set(range(L.STANDIN_SEEDS)) | {chosen}):
        inp = L.vrnn_inputs(case, seed)
        stand = L.vrnn_oracle(inp, mode, case, torch.float32)
        ref, unr = L.vrnn_oracle(inp, mode, case, forced=stand), L.vrnn_oracle(inp, "f32", case)
        n = case[0] * case[1]
        for (name, g, strict), (_, r, _), (_, u, _) in zip(L.vrnn_pieces(stand, H), L.vrnn_pieces(ref, H), L.vrnn_pieces(unr, H)):
            if strict:
                rows = L.row_dist(g.reshape(n, -1), r.reshape(n, -1), 0)
                assert 0.0 < float(rows.median()) and float(rows.max()) <= L.BAR_VALUE / 10  # (0: the oracle handed back the forced value)
                e_r, e_u = L.median_row_distances(g, r, u)
                assert L.MODE_ON * e_r <= e_u, (e_r, e_u)
                continue
            fails, fig = L.two_tier(g, r, u, L.BAR_VALUE, L.VRNN_LOOSE_MULTIPLE)
            if seed < L.STANDIN_SEEDS:
                worst = max(worst, fig["worst_over_in_medians"])
            if seed == chosen:
                assert not fails, (name, fails)
                assert fig["share"] <= 1 / 16 and fig["group_fill"] <= 1 / 2 and fig["row_steps"] <= case[0] // 2 - 1, (name, fig)
    print(f"vrnn {case} {mode}: worst flipped row {worst:.2f} medians")
    assert 2 * worst <= L.VRNN_LOOSE_MULTIPLE


def test_vrnn_sequence_oracle_unrounded_is_the_cell_loop():
    """rnd the identity: `vrnn_cell_step` over the steps (ReLU MLPs, Gaussian heads, residual posterior, phi_z, GRU cell)."""
    case = L.VRNN_CASES[2]
    Tp, B, H, Z, _ = case
    inp = L.vrnn_inputs(case)
    got = L.vrnn_oracle(inp, "f32", case)
    pre = "c"
    sd = {}
    for c, name in (("prior", "prior"), ("post", "posterior")):
        for k in range(3):
            sd[f"{pre}.{name}.{2 * k}.weight"], sd[f"{pre}.{name}.{2 * k}.bias"] = inp[f"{c}_w{k}"].double(), inp[f"{c}_b{k}"].double()
        sd[f"{pre}.{name}.6.params.weight"], sd[f"{pre}.{name}.6.params.bias"] = inp[f"{c}_hw"].double(), inp[f"{c}_hb"].double()
    for k in range(4):
        sd[f"{pre}.phi_z.{2 * k}.weight"], sd[f"{pre}.phi_z.{2 * k}.bias"] = inp[f"phi_w{k}"].double(), inp[f"phi_b{k}"].double()
    for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
        sd[f"{pre}.gru_cell.{n}"] = inp["gru_" + n.replace("weight_", "w").replace("bias_", "b")].double()
    h = inp["h0"].double()
    for t in range(Tp):
        h_prev = h
        h, o = O.vrnn_cell_step(sd, inp["enc"][t].double(), h, inp["eps"][t].double(), True, pre)
        for k in L.VRNN_STATS:
            assert L.rel_l2(got[k][t], o[k]) < 1e-13, (k, t)
        assert L.rel_l2(got["decin"][t], torch.cat([o["phi"], h_prev], -1)) < 1e-13, t
    assert L.rel_l2(got["decin"][Tp, :, H:], h) < 1e-13
