"""CPU: the fp16 AMP training path — `--amp_dtype`, loss scaling in `clip_and_step` (the reference's GradScaler order,
experiments/experiment_vrnn_audio.py:221-230), two ranks skipping the same step, and the operand-type table of the C ABI."""
import os
import re
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import PKG, ROOT


def _common():
    for p in (PKG, os.path.join(ROOT, "experiments"), ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    import _common as C

    return C


def _parser():
    sys.path.insert(0, PKG)
    from blvm.utils.argparsers import build_parser

    return build_parser()


def test_amp_dtype_option():
    p = _parser()
    a = p.parse_args([])
    assert a.amp_dtype == "bf16" and a.use_amp is False
    a = p.parse_args(["--use_amp", "True"])  # --use_amp alone keeps selecting bf16
    assert a.use_amp is True and a.amp_dtype == "bf16"
    a = p.parse_args(["--use_amp", "True", "--amp_dtype", "f16"])
    assert a.use_amp is True and a.amp_dtype == "f16"
    for bad in ("fp16", "f32", "half"):
        with pytest.raises(SystemExit):
            p.parse_args(["--amp_dtype", bad])


def test_operand_dtype_table_matches_the_header():
    sys.path.insert(0, PKG)
    from blvm import _hip

    hdr = open(os.path.join(ROOT, "include", "blvm_hip.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define BLVM_DTYPE_(\w+) (\d+)", hdr)}
    assert defs == {"F32": 0, "BF16": 1, "F16": 2}
    assert _hip.DTYPES == {"f32": defs["F32"], "bf16": defs["BF16"], "f16": defs["F16"]}


def _model(seed=0):
    torch.manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(4, 3)), torch.nn.Parameter(torch.randn(5))]


def _loss(params, k=1.0):
    return k * ((params[0] ** 2).sum() * 3.0 + (params[1] ** 3).sum())


def _snapshot(params, opt):
    return [p.detach().clone() for p in params], [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state[p].items()} for p in params]


def test_clip_and_step_with_a_scaler_clips_the_unscaled_gradients():
    C = _common()
    max_value, max_norm = 5.0, 7.0
    # reference: plain gradients, clipped and applied directly
    ref = _model()
    opt_r = torch.optim.Adam(ref, lr=0.1)
    _loss(ref).backward()
    assert C.clip_and_step(ref, opt_r, max_value, max_norm)
    # scaled: backward on scale * loss; clip_and_step unscales before clipping
    mod = _model()
    opt_m = torch.optim.Adam(mod, lr=0.1)
    scaler = torch.amp.GradScaler("cpu", init_scale=2.0**16, growth_interval=2000)
    scaler.scale(_loss(mod)).backward()
    assert float(mod[0].grad.abs().max()) > 1e3  # the gradients really are scaled on the way in
    assert C.clip_and_step(mod, opt_m, max_value, max_norm, scaler=scaler)
    for a, b in zip(mod, ref):
        torch.testing.assert_close(a.grad, b.grad, rtol=1e-6, atol=0)  # same unscaled, clipped gradient
        torch.testing.assert_close(a.detach(), b.detach(), rtol=1e-6, atol=1e-7)
        assert float(a.grad.abs().max()) <= max_value
    assert scaler.get_scale() == 2.0**16


@pytest.mark.parametrize("skip_nonfinite", [False, True])
def test_clip_and_step_with_a_scaler_skips_an_inf_step(skip_nonfinite):
    C = _common()
    params = _model()
    opt = torch.optim.Adam(params, lr=0.1)
    scaler = torch.amp.GradScaler("cpu", init_scale=2.0**16, growth_interval=2000)
    scaler.scale(_loss(params)).backward()
    assert C.clip_and_step(params, opt, 1000.0, 3000.0, skip_nonfinite, scaler)  # one ordinary step: Adam holds moments
    before, state = _snapshot(params, opt)
    opt.zero_grad(set_to_none=True)
    scaler.scale(_loss(params)).backward()
    params[1].grad[2] = float("inf")  # an fp16 overflow in the backward
    assert not C.clip_and_step(params, opt, 1000.0, 3000.0, skip_nonfinite, scaler)
    assert scaler.get_scale() == 2.0**15  # halved once: the step is counted (and backed off) once
    for p, b, st in zip(params, before, state):
        assert torch.equal(p.detach(), b)
        for k, v in st.items():
            assert torch.equal(opt.state[p][k], v) if torch.is_tensor(v) else opt.state[p][k] == v
    opt.zero_grad(set_to_none=True)  # the run recovers at the lower scale
    scaler.scale(_loss(params)).backward()
    assert C.clip_and_step(params, opt, 1000.0, 3000.0, skip_nonfinite, scaler)
    assert all(not torch.equal(p.detach(), b) and torch.isfinite(p).all() for p, b in zip(params, before))
    assert scaler.get_scale() == 2.0**15


def test_clip_and_step_without_a_scaler_is_unchanged():
    C = _common()
    a, b = _model(), _model()
    oa, ob = torch.optim.Adam(a, lr=0.1), torch.optim.Adam(b, lr=0.1)
    _loss(a, 40.0).backward()
    _loss(b, 40.0).backward()
    assert C.clip_and_step(a, oa, 5.0, 7.0) and C.clip_and_step(b, ob, 5.0, 7.0, scaler=None)
    for x, y in zip(a, b):
        assert torch.equal(x.detach(), y.detach()) and torch.equal(x.grad, y.grad)
    a[0].grad = torch.full_like(a[0], float("nan"))
    assert C.clip_and_step(a, oa, 5.0, 7.0)  # no scaler, no skip flag: steps regardless, as before


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _scaler_worker(rank, world, port, q):
    for p in (PKG, os.path.join(ROOT, "experiments"), ROOT):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    import _common as C
    from blvm.training.ddp import FlatGradAllReduce

    params = _model()  # same weights on both ranks
    opt = torch.optim.Adam(params, lr=0.1)
    scaler = torch.amp.GradScaler("cpu", init_scale=2.0**16, growth_interval=2000)
    red = FlatGradAllReduce(params)
    steps = []
    for step in range(3):
        opt.zero_grad(set_to_none=True)
        scaler.scale(_loss(params, 1.0 + rank)).backward()  # different data per rank
        if step == 1 and rank == 1:
            params[0].grad[1, 1] = float("inf")  # only rank 1 overflows
        red(10.0, status=0.0)
        steps.append(C.clip_and_step(params, opt, 1000.0, 3000.0, False, scaler))
    q.put((rank, steps, scaler.get_scale(), [p.detach().tolist() for p in params]))  # (plain lists: no shared-memory handles)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_skip_the_same_step_and_keep_equal_scales():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_scaler_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict((r, (s, sc, w)) for r, s, sc, w in (q.get(timeout=240) for _ in range(2)))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert res[0][0] == res[1][0] == [True, False, True]  # both ranks skipped step 1, though only rank 1 saw the inf
    assert res[0][1] == res[1][1] == 2.0**15
    for a, b in zip(res[0][2], res[1][2]):
        assert a == b  # the replicas stay identical
