"""CPU: the K10 case tables, links and bars of tests/wavenet_block_cases.py checked by themselves, no device touched.
  * the tables hit every edge class of `edge_requirements()`, and the row counts quoted from the launcher give the plans they are
    there for (1 537 rows: 49 chunks over 48 slices at NSPLIT = 12; 8 309 rows: 520 chunks of 16, two per workgroup);
  * the float64 links equal the oracle's `residual_stack_skips` and `wavenet_block_rounded_ref` (no rounding) where those apply;
  * every bar leaves room: TIMES * the float32 yardstick's own error is at most ROOM = 1e-2 of the slice's scale, for every case and
    tensor, so a wrong element of the size of the data is a hundred bars away;
  * the float32 and float64 links agree on the support of the one-hot cases' gradients, and that support is rows t and t + d of one
    sample; with shift > rows the band of d_x that neither tap reaches is exactly zero;
  * `compare` fails for a yardstick output with ONE defect of the kind a subtly wrong kernel has (one row of a 64-row tile, one column
    tile of a weight gradient) where the whole-tensor norm of the existing test passes it."""
import functools

import pytest
import torch

import blvm_oracle as O
import wavenet_block_cases as K

F64, F32 = torch.float64, torch.float32
ids = lambda c: c.name  # noqa: E731


@functools.lru_cache(maxsize=None)
def block_results(c):
    t = K.block_inputs(c)
    torch32 = K.block_link(c, t, F32)
    return t, K.block_link(c, t, F64), K.block_yardstick(c, t, torch32), torch32


@functools.lru_cache(maxsize=None)
def stack_results(c):
    t = K.stack_inputs(c)
    return t, K.stack_link(c, t, F64), K.stack_link(c, t, F32)


def block_tensors(c):
    return [(k, "columns") for k in K.BLOCK_COLUMNS if not (k == "o" and not c.has_o) and not (k == "skip" and not c.S)] + [(k, "elements") for k in K.BLOCK_ELEMENTS]


# ---- the tables -------------------------------------------------------------------------------------------------------------------


def test_tables_hit_every_edge_class():
    missing = [name for name, (pred, table) in K.edge_requirements().items() if not any(pred(c) for c in table)]
    assert not missing, "\n".join(missing)
    for table in (K.BLOCK_CASES + K.WGRAD_CASES, K.STACK_CASES, K.CONV_K2_CASES):
        names = [c.name for c in table]
        assert len(set(names)) == len(names)
    for c in K.BLOCK_CASES + K.WGRAD_CASES:
        assert c.L_out > 0 and 0 < c.T_skip <= c.L_out and c.off >= 0 and (c.S > 0 or c.has_d_o) and (c.has_o or not c.has_d_o), c.name
        assert c.align in ("", "skip", "o") and not (c.align == "o" and not c.has_o) and not (c.align == "skip" and not c.S), c.name
    for c in K.WGRAD_CASES:
        assert c.fused and c.B == 1 and c.dilation == 1
    for c in K.STACK_CASES:
        L = c.L
        for i in range(c.n_run):
            L -= c.dilations[i]
            assert L >= c.T_skip, c.name


def test_row_counts_quoted_from_the_launcher():
    assert K.ROWS_49_CHUNKS == 1537 and K.ROWS_CHUNK_PLUS_ONE == (17, 33)
    p = K.wgrad_plan(1537, 96, True, 1)
    assert (p.npw, p.nsplit, p.kb, p.n_chunks, p.chunks_per_wg, p.slices) == (1, 12, 32, 49, 2, 25) and p.idle > 0
    p = K.wgrad_plan(K.ROWS_TWO_CHUNKS, 96, True, 6)
    assert (p.npw, p.nsplit, p.kb, p.n_chunks, p.chunks_per_wg, p.slices, p.grid) == (6, 1, 16, 520, 2, 260, 260)
    p = K.wgrad_plan(K.ROWS_IDLE_WGS, 96, True)
    assert p.npw == 3 and p.nsplit == 4 and p.chunks_per_wg == 2 and p.slices % 8 == 1 and p.grid == 8 * 4 * 9
    assert K.wgrad_plan(K.ROWS_IDLE_WGS - 1, 96, True).chunks_per_wg == 1
    # the default form changes to the whole output only at 512 * 64 chunks of 16 rows: far above every case here
    assert K.wgrad_plan(16 * K.WHOLE_MIN_CHUNKS - 16, 96, True).nsplit == 4 and K.wgrad_plan(16 * K.WHOLE_MIN_CHUNKS - 15, 96, True).nsplit == 1
    for c in K.WGRAD_CASES:
        for f in K.npw_forms(c.C):
            for dual in (True, False):
                p = K.wgrad_plan(c.rows, c.C, dual, f)
                assert p.slices * p.chunks_per_wg >= p.n_chunks > (p.slices - 1) * p.chunks_per_wg and p.grid >= p.slices * p.nsplit
                assert p.nsplit == 1 or p.grid % (8 * p.nsplit) == 0


# ---- the links against the oracle module ------------------------------------------------------------------------------------------


def test_stack_link_equals_the_oracle_stack():
    c = K.StackCase("all_blocks", 16, 2, 40, (1, 2, 4, 1), (0, 1, 2, 3), 9)
    t = K.stack_inputs(c)
    got = K.stack_link(c, t, F64)
    sd = {"s.in_transform.weight": torch.eye(c.C, dtype=F64).unsqueeze(-1), "s.in_transform.bias": torch.zeros(c.C, dtype=F64)}
    for i, (cw, cb, rw, rb) in enumerate(t["params"]):
        sd.update({f"s.res_blocks.{i}.conv.weight": cw.double(), f"s.res_blocks.{i}.conv.bias": cb.double(),
                   f"s.res_blocks.{i}.conv1x1rs.weight": rw.double().unsqueeze(-1), f"s.res_blocks.{i}.conv1x1rs.bias": rb.double()})  # fmt: skip
    ref = O.residual_stack_skips(sd, "s", t["x"].double().permute(1, 2, 0), c.dilations, c.T_skip)
    for o, r in zip(got["outs"], ref):
        assert float((o - r.permute(2, 0, 1)).abs().max()) <= 1e-13


@pytest.mark.parametrize("c", [c for c in K.BLOCK_CASES if c.S and c.regime != "onehot"][::5], ids=ids)
def test_block_link_equals_the_oracle_block(c):
    t, ref, _, _ = block_results(c)
    own = O.wavenet_block_rounded_ref(t["x"].double(), t["conv_w"].double(), t["conv_b"].double(), t["rs_w"].double(), t["rs_b"].double(),
                                      c.dilation, c.T_skip, lambda v: v)  # fmt: skip
    assert float((own - ref["own"]).abs().max()) <= 1e-12 * (1 + float(own.abs().max()))
    assert torch.equal(ref["skip"], t["skip0"].double() + ref["own"])


# ---- room under the bars ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("c", K.BLOCK_CASES + K.WGRAD_CASES, ids=ids)
def test_block_bars_leave_room(c):
    t, ref, yard, torch32 = block_results(c)
    worst = {}
    for k, kind in block_tensors(c):
        worst[k] = K.yardstick_room(yard[k], ref[k], kind)
        worst[f"{k} (torch)"] = K.yardstick_room(torch32[k], ref[k], kind)
    if c.rows >= K.PARTITION_ROWS:
        for f in K.npw_forms(c.C):
            part = K.block_partition_yardstick(c, t, torch32, f)
            for k in K.BLOCK_ELEMENTS:
                worst[f"{k} (partition, NPW {f})"] = K.yardstick_room(part[k], ref[k], "elements")
    print({k: f"{v:.1e}" for k, v in worst.items()})
    assert max(worst.values()) < K.ROOM, worst


@pytest.mark.parametrize("c", K.STACK_CASES, ids=ids)
def test_stack_bars_leave_room(c):
    t, ref, yard = stack_results(c)
    worst = {f"out{g}": K.yardstick_room(y, r) for g, (y, r) in enumerate(zip(yard["outs"], ref["outs"]))}
    worst["d_x"] = K.yardstick_room(yard["d_x"], ref["d_x"])
    for i, (y, r) in enumerate(zip(yard["grads"], ref["grads"])):
        worst[f"grad{i}"] = K.yardstick_room(y, r, "elements")
    print({k: f"{v:.1e}" for k, v in worst.items()})
    assert max(worst.values()) < K.ROOM, worst


def test_conv_k2_bars_leave_room():
    for c in K.CONV_K2_CASES:
        t = K.conv_k2_inputs(c)
        ref, yard = K.conv_k2_link(c, t, F64), K.conv_k2_link(c, t, F32)
        kind = "elements" if c.L_out == 1 else "columns"
        worst = {k: K.yardstick_room(yard[k], ref[k], kind if k in ("out", "d_x") else "elements") for k in ("out", "d_x", "dW", "db")}
        assert max(worst.values()) < K.ROOM, (c.name, worst)


# ---- the kernel-order restatement -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("c", [c for c in K.BLOCK_CASES if c.fused], ids=ids)
def test_kernel_order_restatement_is_a_float32_evaluation_of_the_same_block(c):
    """`block_kernel_order` against the float64 link: each of its tensors within a few times the torch float32 link's own worst error
    or the floor of the tensor (it is another float32 order of the same sums, no more and no less accurate), and with the same zeros."""
    t, ref, _, torch32 = block_results(c)
    order = K.block_kernel_order(c, t)
    for k in K.KERNEL_ORDER_YARDSTICK + ("d_pre",):
        r = ref[k].double()
        e_order, e_torch = float((order[k].double() - r).abs().max()), float((torch32[k].double() - r).abs().max())
        print(f"[{c.name}] {k}: worst error, kernel order {e_order:.3e}, torch float32 {e_torch:.3e}, rms {float(r.pow(2).mean().sqrt()):.3e}")
        assert e_order <= max(8 * e_torch, K.FLOOR * float(r.pow(2).mean().sqrt())), k
        if c.regime in ("init", "onehot"):  # (a saturated tanh is exactly 1 in float32 long before it is in float64: more zeros there)
            assert torch.equal(order[k] == 0, r == 0), k


def test_grown_regime_moves_the_error_between_elements():
    """Why the fused cases measure pre, act, dconv_w and dconv_b against the kernel-order restatement: in `grown` both float32 orders
    are off by the same amount at their worst elements of dconv_w, well above FLOOR x rms, but at DIFFERENT elements, so that either
    one, taken as the kernel, misses TIMES x the other at single elements."""
    for name in ("C64_grown", "C96_grown"):
        c = next(c for c in K.BLOCK_CASES if c.name == name)
        t, ref, _, torch32 = block_results(c)
        order = K.block_kernel_order(c, t)
        r = ref["dconv_w"]
        e_o, e_t = (order["dconv_w"].double() - r).abs(), (torch32["dconv_w"].double() - r).abs()
        floor = K.FLOOR * float(r.pow(2).mean().sqrt())
        ratio = K.compare(f"[{name}] dconv_w, kernel order as the kernel", order["dconv_w"], torch32["dconv_w"], r, "elements", check=False).ratio
        print(f"[{name}] dconv_w worst: kernel order {float(e_o.max()):.3e} at {int(e_o.argmax())}, torch {float(e_t.max()):.3e} at {int(e_t.argmax())}, "
              f"floor {floor:.3e}, ratio {ratio:.2f}")
        assert float(e_o.max()) > floor and float(e_t.max()) > floor and int(e_o.argmax()) != int(e_t.argmax())
        assert 1 / 8 < float(e_o.max()) / float(e_t.max()) < 8  # the same size


# ---- exact properties of the links ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("c", [c for c in K.BLOCK_CASES if c.regime == "onehot"], ids=ids)
def test_onehot_support_sets(c):
    _, ref, _, yard = block_results(c)
    t, b, _ = K.hot_position(c)
    want = torch.zeros(c.L_in, c.B, c.C, dtype=torch.bool)
    want[t, b], want[t + c.dilation, b] = True, True
    for link in (ref, yard):
        assert torch.equal(link["d_x"] != 0, want)
        assert torch.equal((link["d_pre"] != 0).any(2), want[: c.L_out].any(2) & (torch.arange(c.L_out) == t)[:, None])
        for k in K.BLOCK_ELEMENTS:
            assert torch.equal(link[k] != 0, ref[k] != 0), k
    if not c.has_d_o:
        assert float(ref["drs_w"][: c.C].abs().max()) == 0.0 and float(ref["drs_b"][: c.C].abs().max()) == 0.0


def test_band_that_neither_tap_reaches_is_zero():
    hit = [c for c in K.BLOCK_CASES if c.shift > c.rows]
    assert hit
    for c in hit:
        _, ref, _, yard = block_results(c)
        for link in (ref, yard):
            band = link["d_x"].reshape(c.L_in * c.B, c.C)[c.rows : c.shift]
            assert band.shape[0] == c.shift - c.rows and float(band.abs().max()) == 0.0
            assert bool((link["d_x"].reshape(c.L_in * c.B, c.C)[: c.rows] != 0).all())


# ---- what the per-column comparison sees and a whole-tensor norm does not ------------------------------------------------------------


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_compare_sees_one_wrong_row_and_one_wrong_column_tile():
    c = next(c for c in K.BLOCK_CASES if c.name == "C64_rows65")
    _, ref, yard, _ = block_results(c)
    assert K.compare("o", yard["o"], yard["o"], ref["o"], check=False).ok
    o = yard["o"].clone()
    o.view(c.rows, c.C)[c.rows - 1] *= 1 + 2e-4  # the one row of the second workgroup, off by 2e-4 of itself
    assert rel_l2(o, ref["o"]) < 2e-5 / 0.6  # (what such a row weighs in the norm the existing test takes)
    assert not K.compare("o, one row", o, yard["o"], ref["o"], check=False).ok

    c = next(c for c in K.WGRAD_CASES if c.C == 96 and c.rows == K.ROWS_49_CHUNKS)
    _, ref, yard, _ = block_results(c)
    w = yard["dconv_w"].clone()
    w[16:32, 80:96, 1] *= 1 + 5e-5  # one 16 x 16 tile of one tap
    assert rel_l2(w, ref["dconv_w"]) < 2e-5  # the existing test's bound on a weight gradient
    assert K.compare("dconv_w", yard["dconv_w"], yard["dconv_w"], ref["dconv_w"], "elements", check=False).ok
    assert not K.compare("dconv_w, one tile", w, yard["dconv_w"], ref["dconv_w"], "elements", check=False).ok


def test_partition_sums_are_the_sums():
    c = next(c for c in K.WGRAD_CASES if c.C == 32 and c.rows == K.ROWS_49_CHUNKS)
    t, ref, _, yard = block_results(c)
    for f in K.npw_forms(c.C):
        part = K.block_partition_yardstick(c, t, yard, f)
        for k in K.BLOCK_ELEMENTS:
            assert part[k].shape == ref[k].shape and part[k].dtype == F32
            assert float((part[k] - ref[k]).abs().max()) <= 1e-5 * float(ref[k].abs().max()), (k, f)


def test_scale_act_ref_is_the_float32_expression():
    x = torch.tensor([-2.0, -0.0, 0.0, 0.3, 1e-30], dtype=F32)
    y = K.scale_act_ref(x, 0.5, 0.2)
    assert y.dtype == F32 and torch.equal(y, torch.tensor([-0.2, -0.0, 0.0, 0.15, 5e-31], dtype=F32))
    assert torch.equal(K.scale_act_ref(x, 1.0, 1.0), x) and torch.equal(K.scale_act_ref(x, 1.0, 0.0), torch.relu(x))
