"""GPU: ``optim.MasterSGD(capturable=True)`` (``rn_sgd_master_step_dev``, csrc/optim.hip) -- the hyperparameters and the step count in
a device block -- against the by-value step it must reproduce bit for bit (``rn_sgd_master_step``), captured under a per-step LR
schedule, across a first step that a loss scaler skips, through ``graph.CapturedTrainStep``, ``SimpleTrainer``, the exchange's
``grads=`` views and checkpoints in every direction, and inside the out-of-bounds guard.

Bars: device block against by value: ``torch.equal``.  Against ``torch.optim.SGD``: rtol 2e-5, atol 1e-6 (tests/test_model_gpu.py,
MasterSGD against torch).  Replay against eager on R18: losses rtol 2e-2, parameters atol 2e-3 (tests/test_graph_gpu.py)."""
import copy
import ctypes as C
import itertools
import logging
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 3, 4, 5, 1023, 1025]
BIG = 1024 * 1024 + 1024 + 3                  # past one pass of the 1024-block grid at 4 elements per thread, plus a scalar tail
_STEPS_WORD, _FIRST_WORD = 5, 6


# ---- 1. the bits of the by-value step ------------------------------------------------------------------------------------------
def _state(sizes, mode, seed):
    """Masters, momentum buffers, 16-bit copies (None for plain fp32 tensors) and three steps' gradients.  ``mode``: "f32": fp32 only;
    "bf16" / "f16": every other tensor a 16-bit copy with 16-bit gradients; "bf16_g32": 16-bit copies with fp32 gradients."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    dt = {"f32": None, "bf16": torch.bfloat16, "f16": torch.float16, "bf16_g32": torch.bfloat16}[mode]
    with16 = [dt is not None and i % 2 == 0 for i in range(len(sizes))]
    w = [torch.randn(n, device=DEV, generator=g) for n in sizes]
    grads = []
    for _ in range(3):
        gs = [torch.randn(n, device=DEV, generator=g) * 0.1 for n in sizes]
        grads.append([x.to(dt) if h and mode != "bf16_g32" else x for x, h in zip(gs, with16)])
    return w, with16, dt, grads


def _copy(w, with16, dt):
    return ([x.clone() for x in w], [torch.full_like(x, float("nan")) for x in w],        # (the first step must not read the buffers)
            [x.to(dt) if h else None for x, h in zip(w, with16)])


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() if t is not None else 0 for t in ts])


def _parity(sizes, mode, combos, amp, seed=0):
    from pytorch_retinanet_amd._lib import RN_BF16, RN_F16, check, lib
    w, with16, dt, grads = _state(sizes, mode, seed)
    n_t = len(sizes)
    ns = (C.c_int64 * n_t)(*sizes)
    grads16 = int(mode in ("bf16", "f16"))
    dt16 = RN_F16 if dt == torch.float16 else RN_BF16
    st = torch.cuda.current_stream().cuda_stream
    scale = torch.full((1,), 4.0, device=DEV) if amp else None
    found = torch.zeros(1, device=DEV) if amp else None
    coef = torch.full((1,), 0.75, device=DEV) if amp else None
    opt = lambda t: t.data_ptr() if t is not None else None
    for momentum, dampening, nesterov, wd in combos:
        a, b = _copy(w, with16, dt), _copy(w, with16, dt)
        has_m = int(momentum != 0)
        moms = lambda s: _ptrs(s[1] if has_m else [None] * n_t)
        hp = torch.zeros(8, dtype=torch.int32, device=DEV)
        for s in range(3):                                        # every rewritable value changes between the steps
            lr, mo, da, dec = 0.05 * (1 + s), momentum * (1 - 0.1 * s), dampening * (1 + s), wd * (1 + 0.5 * s)
            gs = [x * 4.0 for x in grads[s]] if amp else grads[s]          # (the scaler's 4: exact)
            check(lib.rn_sgd_master_step(_ptrs(a[0]), moms(a), _ptrs(gs), _ptrs(a[2]), ns, n_t, grads16, dt16, lr, mo, da, dec, int(nesterov),
                                         int(s == 0), opt(scale), opt(found), opt(coef), st), "rn_sgd_master_step")
            check(lib.rn_sgd_hparams_set(hp.data_ptr(), lr, mo, da, dec, int(nesterov), -1, st), "rn_sgd_hparams_set")
            check(lib.rn_sgd_master_step_dev(_ptrs(b[0]), moms(b), _ptrs(gs), _ptrs(b[2]), ns, n_t, grads16, dt16, has_m, hp.data_ptr(),
                                             opt(scale), opt(found), opt(coef), st), "rn_sgd_master_step_dev")
        torch.cuda.synchronize()
        what = f"mode={mode} amp={amp} momentum={momentum} dampening={dampening} nesterov={nesterov} wd={wd}"
        for i in range(n_t):
            assert torch.equal(a[0][i], b[0][i]), f"master {i} (n={sizes[i]}) {what}"
            if has_m:
                assert torch.equal(a[1][i], b[1][i]) and bool(torch.isfinite(b[1][i]).all()), f"buffer {i} (n={sizes[i]}) {what}"
            else:
                assert bool(torch.isnan(b[1][i]).all()), f"buffer {i} touched without momentum, {what}"
            if a[2][i] is not None:
                assert torch.equal(a[2][i], b[2][i]) and torch.equal(b[2][i], b[0][i].to(dt)), f"16-bit copy {i} {what}"
        assert hp.tolist()[_STEPS_WORD:_FIRST_WORD + 1] == [3, 0], hp.tolist()
        assert not any(torch.equal(x, y) for x, y in zip(b[0], w)), "nothing moved"


COMBOS = list(itertools.product((0.0, 0.9), (0.0, 0.1), (False, True), (0.0, 1e-4)))


@pytest.mark.parametrize("amp", [False, True], ids=["plain", "scale_found_clip"])
@pytest.mark.parametrize("mode", ["f32", "bf16", "f16", "bf16_g32"])
def test_device_block_step_has_the_bits_of_the_by_value_step(mode, amp):
    _parity(SIZES, mode, COMBOS, amp)


@pytest.mark.parametrize("n_tensors", [49, 97])
def test_device_block_step_past_one_table(n_tensors):
    sizes = [(i * 53) % 300 + 1 for i in range(n_tensors)]
    _parity(sizes, "bf16", [(0.9, 0.0, True, 1e-4), (0.9, 0.1, False, 0.0)], True, seed=1)


def test_device_block_step_past_one_grid_pass():
    _parity([BIG, 5], "f16", [(0.9, 0.1, False, 1e-4)], True, seed=2)


def test_zero_momentum_with_buffers_keeps_the_gradient():
    "has_momentum != 0 with momentum == 0 in the block: the masters take the plain step, the buffer takes g + weight_decay * w."
    from pytorch_retinanet_amd._lib import RN_BF16, check, lib
    w, with16, dt, grads = _state(SIZES, "f32", 4)
    a, b = _copy(w, with16, dt), _copy(w, with16, dt)
    n_t, st = len(SIZES), torch.cuda.current_stream().cuda_stream
    ns = (C.c_int64 * n_t)(*SIZES)
    hp = torch.zeros(8, dtype=torch.int32, device=DEV)
    check(lib.rn_sgd_hparams_set(hp.data_ptr(), 0.05, 0.0, 0.0, 1e-2, 0, 3, st), "rn_sgd_hparams_set")
    check(lib.rn_sgd_master_step_dev(_ptrs(b[0]), _ptrs(b[1]), _ptrs(grads[0]), _ptrs(b[2]), ns, n_t, 0, RN_BF16, 1, hp.data_ptr(), None, None,
                                     None, st), "rn_sgd_master_step_dev")
    check(lib.rn_sgd_master_step(_ptrs(a[0]), _ptrs([None] * n_t), _ptrs(grads[0]), _ptrs(a[2]), ns, n_t, 0, RN_BF16, 0.05, 0.0, 0.0, 1e-2, 0, 0,
                                 None, None, None, st), "rn_sgd_master_step")
    torch.cuda.synchronize()
    for i in range(n_t):
        assert torch.equal(a[0][i], b[0][i])
        assert torch.equal(b[1][i], grads[0][i] + np.float32(1e-2) * w[i])
    assert hp.tolist()[_STEPS_WORD] == 4


# ---- the class -----------------------------------------------------------------------------------------------------------------
def _make(sizes, mode, seed=0):
    """Two identical parameter lists: ``mode`` "f32" plain fp32; "bf16" / "f16": every other tensor a 16-bit copy with its fp32 master."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    dt16 = {"f32": None, "bf16": torch.bfloat16, "f16": torch.float16}[mode]
    a, b = [], []
    for i, n in enumerate(sizes):
        w = torch.randn(n, device=DEV, generator=g)
        for out in (a, b):
            if dt16 is not None and i % 2 == 0:
                p = torch.nn.Parameter(w.to(dt16))
                p.master = w.clone()
            else:
                p = torch.nn.Parameter(w.clone())
            out.append(p)
    return a, b


def _grads(params, seed):
    g = torch.Generator(device=DEV).manual_seed(1000 + seed)
    return [(torch.randn(p.shape, device=DEV, generator=g) * 0.1).to(p.dtype) for p in params]


def _w(p):
    return p.master if hasattr(p, "master") else p.data


def _assert_same(opt, ref, mine, theirs, what=""):
    for i, (p, r) in enumerate(zip(mine, theirs)):
        assert torch.equal(_w(p), _w(r)), f"master {i} {what}"
        assert torch.equal(p.data, r.data), f"working copy {i} {what}"
        mb, rb = opt.state[p]["momentum_buffer"], ref.state[r]["momentum_buffer"]
        assert (mb is None) == (rb is None) and (mb is None or torch.equal(mb, rb)), f"buffer {i} {what}"


def test_one_capture_follows_a_schedule():
    """opt.step() alone in a torch.cuda.graph after one eager step, six replays with a new lr written before each: every replay has
    the bits of the eager by-value step at that lr, and the device counter reads 7."""
    from pytorch_retinanet_amd.optim import MasterSGD
    mine, theirs = _make(SIZES + [300, 77], "bf16", seed=3)
    kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-4)
    opt, ref = MasterSGD(mine, capturable=True, **kw), MasterSGD(theirs, **kw)
    static = [torch.zeros_like(p) for p in mine]
    for p, g in zip(mine, static):
        p.grad = g
    graph = None
    for s in range(7):
        lr = 0.05 * (s + 1) / 7 if s < 4 else 0.05 * 0.5 ** (s - 3)
        for g, x, r in zip(static, _grads(mine, s), theirs):
            g.copy_(x)
            r.grad = x
        opt.param_groups[0]["lr"] = ref.param_groups[0]["lr"] = lr
        if s == 0:
            opt.step()                                               # (creates the buffers and the device block)
        else:
            if graph is None:
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    opt.step()                                       # (recorded, not run)
            opt.sync_device_hparams()
            graph.replay()
        ref.step()
        torch.cuda.synchronize()
        _assert_same(opt, ref, mine, theirs, f"after step {s} (lr {lr})")
    assert opt.group_steps() == [7]


def test_skipped_first_step_stays_first():
    """found_inf = 1 on step one moves nothing, the counter included; step two with dampening = 0.1 is the by-value kernel's
    first_step = 1 launch and torch.optim.SGD's first step.  The default mode still refuses dampening under loss scaling."""
    from pytorch_retinanet_amd._lib import RN_BF16, RN_F16, check, lib
    from pytorch_retinanet_amd.optim import MasterSGD
    mine, theirs = _make(SIZES + [300], "f16", seed=5)
    kw = dict(lr=0.05, momentum=0.9, dampening=0.1, weight_decay=1e-4)
    opt = MasterSGD(mine, capturable=True, **kw)
    opt.grad_scale, opt.found_inf = torch.full((1,), 8.0, device=DEV), torch.ones(1, device=DEV)
    gs = _grads(mine, 0)
    for p, g in zip(mine, gs):
        p.grad = g * 8.0
    snap = [(_w(p).clone(), p.data.clone()) for p in mine]
    opt.step()
    torch.cuda.synchronize()
    assert opt.group_steps() == [0]
    for p, (w, c16) in zip(mine, snap):
        assert torch.equal(_w(p), w) and torch.equal(p.data, c16) and not bool(opt.state[p]["momentum_buffer"].any())
    # step two: the first that is taken
    opt.found_inf.zero_()
    gs = _grads(mine, 1)
    for p, g in zip(mine, gs):
        p.grad = g * 8.0
    n_t = len(theirs)
    moms = [torch.full_like(_w(r), float("nan")) for r in theirs]
    check(lib.rn_sgd_master_step(_ptrs([_w(r) for r in theirs]), _ptrs(moms), _ptrs([p.grad for p in mine]),
                                 _ptrs([r.data if hasattr(r, "master") else None for r in theirs]), (C.c_int64 * n_t)(*[r.numel() for r in theirs]),
                                 n_t, 1, RN_F16, 0.05, 0.9, 0.1, 1e-4, 0, 1, opt.grad_scale.data_ptr(), opt.found_inf.data_ptr(), None,
                                 torch.cuda.current_stream().cuda_stream), "rn_sgd_master_step")
    tparams = [torch.nn.Parameter(w.clone()) for w, _ in snap]
    topt = torch.optim.SGD(tparams, foreach=False, **kw)
    for t, g in zip(tparams, gs):
        t.grad = g.float()
    topt.step()
    opt.step()
    torch.cuda.synchronize()
    assert opt.group_steps() == [1]
    for p, r, m, t in zip(mine, theirs, moms, tparams):
        assert torch.equal(_w(p), _w(r)) and torch.equal(p.data, r.data) and torch.equal(opt.state[p]["momentum_buffer"], m)
        torch.testing.assert_close(_w(p), t.detach(), rtol=2e-5, atol=1e-6)
        torch.testing.assert_close(opt.state[p]["momentum_buffer"], topt.state[t]["momentum_buffer"], rtol=2e-5, atol=1e-6)
    default = MasterSGD(theirs, **kw)
    default.grad_scale, default.found_inf = opt.grad_scale, opt.found_inf
    for r, g in zip(theirs, gs):
        r.grad = g
    with pytest.raises(ValueError, match="dampening == 0"):
        default.step()


def _r18(K=5, seed=5):
    import pytorch_retinanet_amd as P
    torch.manual_seed(seed)
    net = P.Retinanet(num_classes=K, backbone_kind="resnet18", pretrained=False, min_size=128, max_size=160).to(DEV)
    return net.to(memory_format=torch.channels_last).train()


def _batches(n, K=5, seed=3):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        images = [torch.from_numpy(rng.random((3, 128, 160), dtype=np.float32)).to(DEV) for _ in range(2)]
        targets = []
        for _ in range(2):
            b, l = synth.gt_boxes(rng, 3, 128, 160, num_classes=K, wh_lo=20.0, wh_hi=90.0)
            targets.append({"boxes": torch.from_numpy(b).to(DEV), "labels": torch.from_numpy(l).to(DEV)})
        out.append((images, targets))
    return out


def _params(net):
    return {n: _w(p).detach().float().cpu() for n, p in net.named_parameters()}


def test_captured_train_step_replays_under_a_per_step_warmup():
    """CapturedTrainStep + MasterSGD(capturable=True) + a per-step LambdaLR warm-up on R18, 8 batches: one capture, six replays, and
    losses and masters within test_graph_gpu.py's bars of the eager run with capturable=False."""
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from pytorch_retinanet_amd.optim import MasterSGD, use_bf16_conv_weights
    data = _batches(8, seed=5)
    res = {}
    for capturable in (False, True):
        net = _r18(seed=11)
        use_bf16_conv_weights(net)
        opt = MasterSGD(net.parameters(), lr=1e-2, momentum=0.9, weight_decay=1e-3, capturable=capturable)
        sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: (s + 1) / 8)
        initial = _params(net)
        step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=2, enabled=capturable)
        losses = []
        for im, tg in data:
            losses.append(float(step(im, tg)["loss"]))
            sch.step()
        torch.cuda.synchronize()
        res[capturable] = (losses, _params(net), step.replays, step.captures, opt.group_steps())
    assert res[False][2] == 0 and res[True][2] == len(data) - 2 and res[True][3] == 1, (res[True][2:4], res[False][2:4])
    assert res[True][4] == res[False][4] == [8]
    assert np.all(np.isfinite(res[True][0]))
    np.testing.assert_allclose(res[True][0], res[False][0], rtol=2e-2)
    for k, a in res[False][1].items():
        torch.testing.assert_close(res[True][1][k], a, rtol=0, atol=2e-3, msg=k)
    moved = sum(float((res[True][1][k] - initial[k]).abs().max()) > 0 for k in initial)
    assert moved > len(initial) // 2


def test_simple_trainer_captures_master_sgd_with_a_step_scheduler_only_when_capturable():
    import pytorch_retinanet_amd as P
    res = {}
    for capturable in (False, True):
        torch.manual_seed(7)
        conf = P.load_hparams()
        conf.model.update(backbone_kind="resnet18", pretrained=False, num_classes=5, min_size=128, max_size=160)
        conf.dataset.kind = "synthetic"
        conf.dataset.update(length=12, height=128, width=160, boxes_per_image=3)
        conf.dataloader.train_bs = 2
        conf.dataloader.valid_bs = 2
        conf.dataloader.args.pin_memory = False
        conf.optimizer.class_name = "pytorch_retinanet_amd.optim.MasterSGD"
        conf.optimizer.params = {"lr": 1e-2, "momentum": 0.9, "weight_decay": 1e-3, "capturable": capturable}
        conf.scheduler.class_name = "torch.optim.lr_scheduler.LambdaLR"
        conf.scheduler.params = {"lr_lambda": lambda s: min(1.0, (s + 1) / 4)}
        conf.scheduler.interval, conf.scheduler.monitor = "step", None
        model = P.RetinaNetModel(conf)
        model.prepare_data()
        model.val_ds = None
        trainer = P.SimpleTrainer(max_epochs=1, device=DEV)
        losses = []
        handler = logging.Handler()
        handler.emit = lambda rec: losses.append(rec.args[-1])
        trainer.log.addHandler(handler)
        trainer.log_every, old = 1, trainer.log.level
        trainer.log.setLevel(logging.INFO)
        try:
            steps = trainer.fit(model)
        finally:
            trainer.log.removeHandler(handler)
            trainer.log.setLevel(old)
        assert steps == 6 and len(losses) == 6 and all(math.isfinite(v) for v in losses), (steps, losses)
        assert model.optimizer.capturable == capturable
        assert model.optimizer.param_groups[0]["lr"] == pytest.approx(1e-2)        # the schedule ran through the replays
        res[capturable] = (trainer.captured_steps, losses, _params(model.net))
    assert res[True][0] > 0 and res[False][0] == 0, (res[True][0], res[False][0])
    np.testing.assert_allclose(res[True][1], res[False][1], rtol=2e-2)
    for k, a in res[False][2].items():
        torch.testing.assert_close(res[True][2][k], a, rtol=0, atol=2e-3, msg=k)


def test_bucketed_ddp_world1_with_capturable_master_sgd_equals_plain_step():
    "BucketedGradAllReduce at world size 1 + MasterSGD(capturable=True).step(grads=grad_views()) == its plain step (R18, K = 5)."
    import pytorch_retinanet_amd as P
    from pytorch_retinanet_amd.optim import MasterSGD, use_bf16_conv_weights
    data = _batches(2)

    def run(use_ddp):
        net = _r18()
        use_bf16_conv_weights(net)
        opt = MasterSGD(net.parameters(), lr=1e-2, momentum=0.9, weight_decay=1e-4, capturable=True)
        ddp = P.BucketedGradAllReduce(net, bucket_mb=8.0) if use_ddp else None
        for images, targets in data:
            ddp.zero_grad() if ddp else opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = net(images, [dict(t) for t in targets])
            (out["classification_loss"] + out["regression_loss"]).backward()
            if ddp:
                ddp.finish()
                opt.step(grads=ddp.grad_views())
            else:
                opt.step()
        assert opt.group_steps() == [2]
        return _params(net)

    a, b = run(True), run(False)
    for k in a:
        torch.testing.assert_close(a[k], b[k], rtol=0, atol=5e-4, msg=k)


def _saved(sd):
    "A state_dict through a checkpoint file (state_dict() hands out the live buffers)."
    import io
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    return torch.load(buf)


def test_checkpoints_move_between_both_modes_and_torch():
    """Two steps in each of capturable MasterSGD, by-value MasterSGD and torch.optim.SGD on the same gradients; every checkpoint is
    loaded into a fresh optimizer of each other kind (on copies of the weights it was taken at), and the next step of the loaded
    optimizer is the by-value optimizer's: the same bits for this class, the bar of MasterSGD against torch for torch."""
    from pytorch_retinanet_amd.optim import MasterSGD
    kw = dict(lr=0.05, momentum=0.9, dampening=0.1, weight_decay=1e-4)
    sizes = SIZES + [300]
    cap_p, val_p = _make(sizes, "bf16", seed=7)
    tor_p = [torch.nn.Parameter(_w(p).clone()) for p in cap_p]
    cap, val, tor = MasterSGD(cap_p, capturable=True, **kw), MasterSGD(val_p, **kw), torch.optim.SGD(tor_p, foreach=False, **kw)

    def step(o, ps, s):
        for p, g in zip(ps, _grads(cap_p, s)):
            p.grad = g if p.dtype == g.dtype else g.float()
        o.step()
    for s in range(2):
        for o, ps in ((cap, cap_p), (val, val_p), (tor, tor_p)):
            step(o, ps, s)
    torch.cuda.synchronize()
    _assert_same(cap, val, cap_p, val_p, "before the checkpoints")
    assert cap.state_dict()["state"][0]["steps"] == 2 and val.state_dict()["state"][0]["steps"] == 2
    assert set(cap.state_dict()["state"][0]) == {"momentum_buffer", "steps"}

    def fresh(kind):
        "A new optimizer of ``kind`` on copies of the by-value run's weights, with other hyperparameters than the checkpoint's."
        ps, _ = _make(sizes, "bf16", seed=99)
        with torch.no_grad():
            for p, r in zip(ps, val_p):
                _w(p).copy_(_w(r))
                p.data.copy_(_w(r))
        if kind == "torch":
            ps = [torch.nn.Parameter(_w(r).clone()) for r in val_p]
            return torch.optim.SGD(ps, lr=5.0, momentum=0.5, foreach=False), ps
        return MasterSGD(ps, lr=5.0, momentum=0.5, capturable=kind == "cap"), ps
    sds = {"cap": _saved(cap.state_dict()), "val": _saved(val.state_dict()), "torch": _saved(tor.state_dict())}
    loaded = []
    for src, dst in (("cap", "val"), ("cap", "torch"), ("val", "cap"), ("torch", "cap"), ("torch", "val"), ("val", "torch"), ("cap", "cap")):
        o, ps = fresh(dst)
        o.load_state_dict(copy.deepcopy(sds[src]))       # (torch keeps the loaded buffers themselves and steps on them)
        assert o.param_groups[0]["lr"] == 0.05 and o.param_groups[0]["dampening"] == 0.1, (src, dst)
        if dst == "cap":
            assert o.group_steps() == [2 if src != "torch" else 1], (src, dst)
        step(o, ps, 2)
        loaded.append((src, dst, o, ps))
    step(val, val_p, 2)
    torch.cuda.synchronize()
    for src, dst, o, ps in loaded:
        exact = dst != "torch" and src != "torch"            # (torch's own two steps differ from ours in the last bits)
        for i, (p, r) in enumerate(zip(ps, val_p)):
            mb = o.state[p]["momentum_buffer"]
            if exact:
                assert torch.equal(_w(p), _w(r)) and torch.equal(p.data, r.data) and torch.equal(mb, val.state[r]["momentum_buffer"]), (src, dst, i)
            else:
                torch.testing.assert_close(_w(p), _w(r), rtol=2e-5, atol=1e-6, msg=f"{src}->{dst} master {i}")
                torch.testing.assert_close(mb, val.state[r]["momentum_buffer"], rtol=2e-5, atol=1e-6, msg=f"{src}->{dst} buffer {i}")
            assert mb.dtype == torch.float32
        if dst == "cap":
            assert o.group_steps() == [3 if src != "torch" else 2]


def test_structural_settings_are_fixed_once_the_block_exists():
    from pytorch_retinanet_amd.optim import MasterSGD
    mine, _ = _make([5, 300], "bf16", seed=9)
    for p, g in zip(mine, _grads(mine, 0)):
        p.grad = g
    opt = MasterSGD(mine, lr=0.05, momentum=0.9, capturable=True)
    opt.step()
    opt.param_groups[0].update(momentum=0.0, dampening=0.2, weight_decay=1e-3, lr=0.01)        # rewritable
    opt.step()
    opt.param_groups[0]["nesterov"] = True
    opt.param_groups[0].update(momentum=0.9, dampening=0.0)
    with pytest.raises(ValueError, match="nesterov"):
        opt.step()
    opt.param_groups[0]["nesterov"] = False
    opt.step()
    plain = MasterSGD([torch.nn.Parameter(torch.randn(7, device=DEV))], lr=0.05, capturable=True)
    plain.param_groups[0]["params"][0].grad = torch.randn(7, device=DEV)
    plain.step()
    assert plain.state[plain.param_groups[0]["params"][0]]["momentum_buffer"] is None
    plain.param_groups[0]["momentum"] = 0.9
    with pytest.raises(ValueError, match="momentum"):
        plain.sync_device_hparams()
    torch.cuda.synchronize()
    assert opt.group_steps() == [3] and plain.group_steps() == [1]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_sgd_dev_step_stays_inside_its_operands(dt):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "guard_probe.py"), "sgd_dev", dt], capture_output=True, text=True,
                       env=env, timeout=300, cwd=ROOT)
    tail = (r.stdout + r.stderr)[-1500:]
    assert r.returncode == 0, f"probe sgd_dev died (GPU memory access fault?):\n{tail}"
    assert "ok sgd_dev" in r.stdout, tail
