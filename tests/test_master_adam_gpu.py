"""GPU: ``optim.MasterAdam`` / ``MasterAdamW`` (``rn_adam_master_step``, csrc/adam.hip) against ``torch.optim.Adam`` / ``AdamW``
(single-tensor fp32 path, same device, same gradients), captured with a per-step LR schedule, under ``torch.amp.GradScaler``,
through the exchange's ``grads=`` views, ``graph.CapturedTrainStep`` and ``SimpleTrainer``, across checkpoints in either direction,
and inside the out-of-bounds guard.

Bars: masters within 2e-6 relative (or 1e-3 * lr absolute: an element whose update nearly cancels it), moments within 2 ulp (of
the element, or of 1e-3 of the tensor's largest moment for elements near zero), the 16-bit working copy exactly round(master)."""
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
SIZES = [1, 3, 1023, 4097, 4098] + [(i * 53) % 700 + 1 for i in range(41)]      # 46 tensors: two launches; 4098 and most: tail path


def _ulps(a: torch.Tensor, b: torch.Tensor, slack: float = 0.0) -> float:
    """Largest distance between two fp32 tensors of one shape, less ``slack`` (absolute), in units in the last place of the reference
    element, with a floor of 1e-3 of the tensor's largest magnitude: an element that nearly cancels carries the absolute error of its
    neighbours, not a relative one."""
    if not a.numel():
        return 0.0
    floor = 1e-3 * float(b.abs().max())
    mag = torch.clamp(b.abs(), min=max(floor, 1e-30))
    ulp = torch.pow(2.0, torch.floor(torch.log2(mag)) - 23)
    return float((torch.clamp((a - b).abs() - slack, min=0.0) / ulp).max())


def _check_close(mine_w, ref_w, lr, what):
    err = (mine_w - ref_w).abs()
    bad = err > torch.maximum(2e-6 * ref_w.abs(), torch.full_like(ref_w, 1e-3 * lr))
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements off, worst {float(err.max()):.3e}"


def _check_state(opt, ref_opt, params, ref_params, lr, dt16, l2=0.0, steps=10):
    """``l2``: Adam's L2 weight decay feeds the master into the gradient (g + wd * w), so the masters' last-bit differences (inside
    their own bar) reach the moments: at most steps * wd * max|dw| on top of the 2 ulp."""
    for i, (p, r) in enumerate(zip(params, ref_params)):
        w = p.master if hasattr(p, "master") else p.data
        _check_close(w, r.detach(), lr, f"master {i} (n={w.numel()})")
        slack = steps * l2 * float((w - r.detach()).abs().max()) if w.numel() else 0.0
        st, rs = opt.state[p], ref_opt.state[r]
        for k in ("exp_avg", "exp_avg_sq"):
            u = _ulps(st[k], rs[k], slack * (1.0 if k == "exp_avg" else 2.0 * float(rs["exp_avg"].abs().max()) if w.numel() else 0.0))
            assert u <= 2, (i, k, u)
        if hasattr(p, "master"):
            assert torch.equal(p.data, p.master.to(dt16)), f"working copy {i} != round(master)"


def _make(sizes, mode, seed=0):
    """(ours, torch's): ``mode`` "f32": plain fp32 parameters; "bf16" / "f16": every other tensor a 16-bit working copy with its fp32
    master (the others plain fp32, like BN parameters), 16-bit gradients for the 16-bit copies."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    dt16 = {"f32": None, "bf16": torch.bfloat16, "f16": torch.float16}[mode]
    mine, ref = [], []
    for i, n in enumerate(sizes):
        w = torch.randn(n, device=DEV, generator=g)
        if dt16 is not None and i % 2 == 0:
            p = torch.nn.Parameter(w.to(dt16))
            p.master = w.clone()
        else:
            p = torch.nn.Parameter(w.clone())
        mine.append(p)
        ref.append(torch.nn.Parameter(w.clone()))
    return mine, ref, dt16


def _grads(params, seed):
    g = torch.Generator(device=DEV).manual_seed(1000 + seed)
    out = []
    for p in params:
        x = torch.randn(p.shape, device=DEV, generator=g) * 0.1
        out.append(x.to(p.dtype))              # (16-bit copies take 16-bit gradients: the reference gets them promoted exactly)
    return out


@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("kind,wd", [("adam", 0.0), ("adam", 0.05), ("adamw", 0.0), ("adamw", 0.1)])
def test_step_equals_torch_elementwise(mode, kind, wd):
    from pytorch_retinanet_amd.optim import MasterAdam, MasterAdamW
    mine, ref, dt16 = _make(SIZES, mode)
    cls, tcls = (MasterAdam, torch.optim.Adam) if kind == "adam" else (MasterAdamW, torch.optim.AdamW)
    opt = cls(mine, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    ropt = tcls(ref, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd, foreach=False)
    for s in range(10):
        lr = 1e-3 * (1.0 + 0.5 * math.sin(s))                        # a new lr every step
        for o in (opt, ropt):
            o.param_groups[0]["lr"] = lr
        for p, r, g in zip(mine, ref, _grads(mine, s)):
            p.grad, r.grad = g, g.float()
        opt.step()
        ropt.step()
    torch.cuda.synchronize()
    _check_state(opt, ropt, mine, ref, lr, dt16, l2=wd if kind == "adam" else 0.0)
    assert opt.group_steps() == [10.0]


def test_captured_step_follows_a_per_step_schedule():
    """opt.step() alone in a torch.cuda.graph, replayed with a LambdaLR stepping and sync_device_hparams() between replays: the
    trajectory is torch's eager one.  A step count or lr baked into the graph fails this."""
    from pytorch_retinanet_amd.optim import MasterAdamW
    mine, ref, dt16 = _make(SIZES[:12], "bf16", seed=3)
    opt = MasterAdamW(mine, lr=2e-3, weight_decay=0.05)
    ropt = torch.optim.AdamW(ref, lr=2e-3, weight_decay=0.05, foreach=False)
    lam = lambda s: (s + 1) / 4 if s < 4 else 0.5 ** (s - 3)
    sch, rsch = torch.optim.lr_scheduler.LambdaLR(opt, lam), torch.optim.lr_scheduler.LambdaLR(ropt, lam)
    static = [torch.zeros_like(p) for p in mine]
    for p, g in zip(mine, static):
        p.grad = g
    graph = None
    for s in range(10):
        gs = _grads(mine, s)
        for g, x, r in zip(static, gs, ref):
            g.copy_(x)
            r.grad = x.float()
        if s == 0:
            opt.step()                                                 # (creates the moments and the device block)
        else:
            if graph is None:
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    opt.step()                                         # (recorded, not run)
            opt.sync_device_hparams()
            graph.replay()
        ropt.step()
        sch.step()
        rsch.step()
    torch.cuda.synchronize()
    _check_state(opt, ropt, mine, ref, ropt.param_groups[0]["lr"], dt16)
    assert opt.group_steps() == [10.0]


def test_grad_scaler_skip_then_torch_trajectory():
    """fp16 copies under torch.amp.GradScaler: a step with an inf gradient changes no master, moment, working copy or step
    counter; the whole trajectory equals torch.optim.AdamW's under its own GradScaler."""
    from pytorch_retinanet_amd.optim import MasterAdamW
    mine, ref, dt16 = _make(SIZES[:10], "f16", seed=5)
    opt = MasterAdamW(mine, lr=1e-3, weight_decay=0.01)
    ropt = torch.optim.AdamW(ref, lr=1e-3, weight_decay=0.01, foreach=False)
    sc, rsc = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10), torch.amp.GradScaler("cuda", init_scale=2.0 ** 10)
    gen = torch.Generator(device=DEV).manual_seed(8)
    for s in range(6):
        # loss = sum(p * c): the gradient is scale * c, exact in fp16 (c is fp16-representable, the scale a power of two)
        cs = [(torch.randn(p.shape, device=DEV, generator=gen) * 0.1).half().float() for p in mine]
        if s == 2:
            cs[3][0] = float("inf")
            snap = [((p.master if hasattr(p, "master") else p.data).clone(), p.data.clone(), opt.state[p]["exp_avg"].clone(),
                     opt.state[p]["exp_avg_sq"].clone()) for p in mine]
        for o, ps, scaler in ((opt, mine, sc), (ropt, ref, rsc)):
            o.zero_grad(set_to_none=True)
            loss = sum((p.float() * c).sum() for p, c in zip(ps, cs))
            scaler.scale(loss).backward()
            scaler.step(o)
            scaler.update()
        if s == 2:
            torch.cuda.synchronize()
            assert opt.group_steps() == [2.0]
            for p, (w, c16, m, v) in zip(mine, snap):
                assert torch.equal(p.master if hasattr(p, "master") else p.data, w) and torch.equal(p.data, c16)
                assert torch.equal(opt.state[p]["exp_avg"], m) and torch.equal(opt.state[p]["exp_avg_sq"], v)
    torch.cuda.synchronize()
    assert float(sc.get_scale()) == float(rsc.get_scale()) and opt.group_steps() == [5.0]
    _check_state(opt, ropt, mine, ref, 1e-3, dt16)


def test_master_adamw_follows_torch_adamw_under_autocast():
    """fp32 masters + bf16 conv weights + MasterAdamW == fp32 parameters + autocast + torch.optim.AdamW (the bars of
    test_master_sgd_follows_torch_sgd_under_autocast)."""
    from pytorch_retinanet_amd.norm import FusedBatchNorm2d
    from pytorch_retinanet_amd.optim import MasterAdamW, master_state_dict, use_bf16_conv_weights

    def make():
        torch.manual_seed(11)
        m = torch.nn.Sequential(torch.nn.Conv2d(8, 16, 3, padding=1), FusedBatchNorm2d(16), torch.nn.ReLU(),
                                torch.nn.Conv2d(16, 8, 1, bias=False)).to(DEV).to(memory_format=torch.channels_last)
        return m.train()
    a, b = make(), make()
    kw = dict(lr=1e-3, weight_decay=1e-2)
    oa = torch.optim.AdamW(a.parameters(), foreach=False, **kw)
    assert use_bf16_conv_weights(b) == 2
    ob = MasterAdamW(b.parameters(), **kw)
    x = torch.randn(4, 8, 12, 10, device=DEV).contiguous(memory_format=torch.channels_last)
    for _ in range(4):
        for m, o in ((a, oa), (b, ob)):
            o.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = (m(x).float() ** 2).mean()
            loss.backward()
            o.step()
    sa, sb = a.state_dict(), master_state_dict(b)
    assert b[0].weight.dtype == torch.bfloat16 and sb["0.weight"].dtype == torch.float32
    for k in sa:
        torch.testing.assert_close(sb[k].float(), sa[k].float(), rtol=2e-5, atol=1e-6, msg=k)
    assert torch.equal(b[0].weight.float(), sb["0.weight"].to(torch.bfloat16).float())      # working copy == bf16(master)


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
    return {n: (p.master if hasattr(p, "master") else p.data).detach().float().cpu() for n, p in net.named_parameters()}


def test_bucketed_ddp_world1_with_master_adamw_equals_plain_step():
    """BucketedGradAllReduce at world size 1 + MasterAdamW.step(grads=grad_views()) == the plain MasterAdamW step (R18, K = 5).
    lr 1e-4: Adam moves an element by at most ~lr per step whatever its gradient, so the atomics noise of MIOpen's weight
    gradients stays inside the bar of the MasterSGD twin of this test."""
    import pytorch_retinanet_amd as P
    from pytorch_retinanet_amd.optim import MasterAdamW, use_bf16_conv_weights
    data = _batches(2)

    def run(use_ddp):
        net = _r18()
        use_bf16_conv_weights(net)
        opt = MasterAdamW(net.parameters(), lr=1e-4, weight_decay=1e-2)
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
        return _params(net)

    a, b = run(True), run(False)
    for k in a:
        torch.testing.assert_close(a[k], b[k], rtol=0, atol=5e-4, msg=k)


def test_captured_train_step_replays_with_a_per_step_schedule():
    """CapturedTrainStep + MasterAdamW + a per-step LambdaLR on R18, 8 batches: 1 capture, 6 replays (torch's AdamW: 0), and the
    parameters within test_graph_gpu.py's bars of the eager run."""
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from pytorch_retinanet_amd.optim import MasterAdamW, use_bf16_conv_weights
    data = _batches(8, seed=5)
    res = {}
    for captured in (False, True):
        net = _r18(seed=11)
        use_bf16_conv_weights(net)
        opt = MasterAdamW(net.parameters(), lr=2e-4, weight_decay=1e-2)
        sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: (s + 1) / 8)
        initial = _params(net)
        step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=2, enabled=captured)
        losses = []
        for im, tg in data:
            losses.append(float(step(im, tg)["loss"]))
            sch.step()
        torch.cuda.synchronize()
        res[captured] = (losses, _params(net), step.replays, step.captures, opt.group_steps())
    assert res[False][2] == 0 and res[True][2] == len(data) - 2 and res[True][3] == 1
    assert res[True][4] == res[False][4] == [8.0]
    assert np.all(np.isfinite(res[True][0]))
    np.testing.assert_allclose(res[True][0], res[False][0], rtol=2e-2)
    for k, a in res[False][1].items():
        torch.testing.assert_close(res[True][1][k], a, rtol=0, atol=2e-3, msg=k)
    moved = sum(float((res[True][1][k] - initial[k]).abs().max()) > 0 for k in initial)
    assert moved > len(initial) // 2


def test_simple_trainer_captures_master_adamw_with_a_step_scheduler():
    import pytorch_retinanet_amd as P
    torch.manual_seed(7)
    conf = P.load_hparams()
    conf.model.update(backbone_kind="resnet18", pretrained=False, num_classes=5, min_size=128, max_size=160)
    conf.dataset.kind = "synthetic"
    conf.dataset.update(length=12, height=128, width=160, boxes_per_image=3)
    conf.dataloader.train_bs = 2
    conf.dataloader.valid_bs = 2
    conf.dataloader.args.pin_memory = False
    conf.optimizer.class_name = "pytorch_retinanet_amd.optim.MasterAdamW"
    conf.optimizer.params = {"lr": 1e-4, "weight_decay": 1e-2}
    conf.scheduler.class_name = "torch.optim.lr_scheduler.LambdaLR"
    conf.scheduler.params = {"lr_lambda": lambda s: min(1.0, (s + 1) / 4)}
    conf.scheduler.interval, conf.scheduler.monitor = "step", None
    model = P.RetinaNetModel(conf)
    model.prepare_data()
    model.val_ds = None
    trainer = P.SimpleTrainer(max_epochs=1, device=DEV)
    losses = []
    import logging
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
    assert steps == 6 and trainer.captured_steps > 0, (steps, trainer.captured_steps)
    assert model.net.retinanet_head.classification_head.class_subnet[0].weight.dtype == torch.bfloat16
    assert len(losses) == 6 and all(math.isfinite(v) for v in losses), losses
    assert model.optimizer.param_groups[0]["lr"] == pytest.approx(1e-4)          # the schedule ran through the replays


def _saved(sd):
    "A state_dict through a checkpoint file (state_dict() hands out the live moment tensors)."
    import io
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    return torch.load(buf)


def test_checkpoint_moves_both_ways_between_master_adamw_and_torch_adamw():
    """3 steps, swap the optimizers' state_dicts (MasterAdamW -> torch.optim.AdamW and back, weights via master_state_dict), 3 more
    steps: each resumed run stays on the trajectory of the run it was taken from (the bars of the elementwise test)."""
    from pytorch_retinanet_amd.optim import MasterAdamW
    mine, ref, dt16 = _make(SIZES[:10], "bf16", seed=7)
    kw = dict(lr=1e-3, betas=(0.9, 0.99), weight_decay=0.02)
    opt, ropt = MasterAdamW(mine, **kw), torch.optim.AdamW(ref, foreach=False, **kw)

    def step(o, ps, s, lr):
        o.param_groups[0]["lr"] = lr
        for p, g in zip(ps, _grads(mine, s)):
            p.grad = g if p.dtype == g.dtype else g.float()
        o.step()
    for s in range(3):
        step(opt, mine, s, 1e-3)
        step(ropt, ref, s, 1e-3)
    # MasterAdamW's checkpoint into a fresh torch AdamW on fp32 copies of the masters; torch's into a fresh MasterAdamW
    ref2 = [torch.nn.Parameter((p.master if hasattr(p, "master") else p.data).clone()) for p in mine]
    ropt2 = torch.optim.AdamW(ref2, foreach=False, lr=5.0)
    ropt2.load_state_dict(_saved(opt.state_dict()))
    mine2, _, _ = _make(SIZES[:10], "bf16", seed=99)
    with torch.no_grad():
        for p, r in zip(mine2, ref):
            (p.master if hasattr(p, "master") else p.data).copy_(r)
            p.data.copy_(r)
    opt2 = MasterAdamW(mine2, lr=5.0)
    opt2.load_state_dict(_saved(ropt.state_dict()))
    assert opt2.param_groups[0]["lr"] == 1e-3 and opt2.param_groups[0]["betas"] == (0.9, 0.99) and opt2.group_steps() == [3.0]
    assert float(ropt2.state[ref2[0]]["step"]) == 3.0
    for s in range(3, 6):
        lr = 1e-3 * (1 + 0.2 * s)
        step(opt, mine, s, lr)
        step(ropt2, ref2, s, lr)
        step(opt2, mine2, s, lr)
        step(ropt, ref, s, lr)
    torch.cuda.synchronize()
    _check_state(opt, ropt2, mine, ref2, lr, dt16)           # ours, continued == torch, resumed from ours
    _check_state(opt2, ropt, mine2, ref, lr, dt16)           # ours, resumed from torch == torch, continued


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_adam_step_stays_inside_its_operands(dt):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "guard_probe.py"), "adam", dt], capture_output=True, text=True,
                       env=env, timeout=300, cwd=ROOT)
    tail = (r.stdout + r.stderr)[-1500:]
    assert r.returncode == 0, f"probe adam died (GPU memory access fault?):\n{tail}"
    assert "ok adam" in r.stdout, tail
