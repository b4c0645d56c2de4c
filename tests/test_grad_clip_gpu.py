"""GPU: global-norm gradient clipping for the master optimizers (``optim.GradClip``, ``rn_grad_norm_clip`` in csrc/clip.hip, and the
``_clip`` forms of the SGD / Adam steps): the norm against float64, its determinism, the coefficient against its fp32 restatement,
the clipped update against torch's optimizers fed ``g * coef``, under ``torch.amp.GradScaler``, captured alone and as the whole train
step, through the exchange's ``grads=`` views and ``SimpleTrainer``, and inside the out-of-bounds guard.

Bars: the norm within twice the error of torch's own fp32 ``clip_grad_norm_`` norm against float64 (floor: 16 fp32 ulp); the update
with the coefficient READ BACK from the block, so the step's arithmetic is judged at test_master_adam_gpu.py's bars (Adam) and at the
bars of MasterSGD's fp32 / bf16 (rtol 2e-5, atol 1e-6) and fp16 (rtol 2e-4, atol 2e-5) tests."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_master_adam_gpu import SIZES, _batches, _check_state, _grads, _make, _params, _r18

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 2_500_003                                  # 153 chunks, a tail of 3 elements
MODES = ["f32", "bf16", "f16"]


def _norm_call(clip, grads, scale=None):
    "One rn_grad_norm_clip call over ``grads`` (16-bit tensors are 16-bit gradients); returns (total_norm, clip_coef) as Python floats."
    from pytorch_retinanet_amd._lib import RN_BF16, RN_F16
    is16 = [g.dtype != torch.float32 for g in grads]
    f16 = any(g.dtype == torch.float16 for g in grads)
    clip.compute([g.data_ptr() for g in grads], [g.data_ptr() if h else 0 for g, h in zip(grads, is16)], [g.numel() for g in grads],
                 RN_F16 if f16 else RN_BF16, scale, grads[0].device)
    blk = clip._block.view(torch.float32)[:3].cpu()
    return float(blk[1]), float(blk[2])


def _ulp(x: float) -> float:
    return 2.0 ** (math.floor(math.log2(abs(x))) - 23)


@pytest.mark.parametrize("mode", MODES)
def test_norm_against_float64(mode):
    from pytorch_retinanet_amd.optim import GradClip
    mine, _, _ = _make(SIZES + [BIG], mode, seed=2)
    grads = _grads(mine, 4)
    ref = float(torch.linalg.vector_norm(torch.cat([g.double().flatten() for g in grads])))
    ps = [torch.nn.Parameter(torch.zeros(g.shape, device=DEV)) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = g.float()
    torch_norm = float(torch.nn.utils.clip_grad_norm_(ps, 1e30))
    total, coef = _norm_call(GradClip(1e30), grads)
    err_t, err_k = abs(torch_norm - ref), abs(total - ref)
    bar = max(2.0 * err_t, 16.0 * _ulp(ref))
    print(f"norm[{mode}] float64 {ref!r}: torch fp32 error {err_t:.3e}, kernel error {err_k:.3e}, bar {bar:.3e} (ulp {_ulp(ref):.3e})")
    assert err_k <= bar, (mode, ref, torch_norm, total)
    assert coef == 1.0


@pytest.mark.parametrize("mode", MODES)
def test_norm_and_coefficient_are_bit_equal_over_ten_calls(mode):
    from pytorch_retinanet_amd.optim import GradClip
    mine, _, _ = _make(SIZES + [BIG], mode, seed=3)
    grads = _grads(mine, 6)
    clip = GradClip(0.5)
    a = torch.randn(512, 512, device=DEV)
    seen = set()
    for i in range(10):
        b = a @ a                                                      # (other work on the stream between the calls)
        if i % 3 == 0:
            b = b.relu().sum()
        _norm_call(clip, grads)
        seen.add(clip._block.view(torch.int32)[1:3].cpu().numpy().tobytes())
    assert len(seen) == 1
    assert clip.stats() == {"calls": 10, "clipped": 10, "nonfinite": 0}


@pytest.mark.parametrize("mode", MODES)
def test_coefficient_equals_its_restatement_and_the_scale_divides_out(mode):
    from pytorch_retinanet_amd.optim import GradClip
    mine, _, _ = _make(SIZES + [BIG], mode, seed=4)
    grads = _grads(mine, 8)                                             # |g| < 1: 1024 g is exact in bf16 / fp16 / fp32, no overflow
    clip = GradClip(1.0)
    totals = []
    for max_norm in (1.0, 1e-3, 157.0, 158.5, 1e4, 0.3333):
        clip.max_norm = max_norm
        total, coef = _norm_call(clip, grads)
        totals.append(total)
        assert np.float32(coef).tobytes() == np.float32(GradClip.coef(total, max_norm)).tobytes(), (max_norm, total, coef)
    assert len(set(totals)) == 1
    assert any(GradClip.coef(totals[0], m) == 1.0 for m in (1e4,)) and GradClip.coef(totals[0], 1e-3) < 1.0
    scale = torch.full((1,), 1024.0, device=DEV)
    scaled = [g * 1024.0 for g in grads]
    assert all(torch.equal(s.double(), g.double() * 1024.0) for s, g in zip(scaled, grads))
    total_s, coef_s = _norm_call(clip, scaled, scale)
    assert abs(total_s - totals[0]) <= 2.0 * _ulp(totals[0]), (total_s, totals[0])
    assert np.float32(coef_s).tobytes() == np.float32(GradClip.coef(total_s, 0.3333)).tobytes()


def _build(kind, mine, ref, lrs, clip_norm):
    """(ours, torch's) on two parameter groups with different learning rates (even / odd tensors)."""
    from pytorch_retinanet_amd.optim import MasterAdam, MasterAdamW, MasterSGD
    groups = lambda ps: [{"params": ps[0::2], "lr": lrs[0]}, {"params": ps[1::2], "lr": lrs[1]}]
    if kind == "sgd":
        kw = dict(momentum=0.9, weight_decay=1e-2)
        return MasterSGD(groups(mine), lr=lrs[0], max_grad_norm=clip_norm, **kw), torch.optim.SGD(groups(ref), lr=lrs[0], foreach=False, **kw)
    cls, tcls, wd = (MasterAdam, torch.optim.Adam, 0.05) if kind == "adam" else (MasterAdamW, torch.optim.AdamW, 0.1)
    return cls(groups(mine), lr=lrs[0], weight_decay=wd, max_grad_norm=clip_norm), tcls(groups(ref), lr=lrs[0], weight_decay=wd, foreach=False)


def _check_update(kind, mode, opt, ropt, dt16):
    for g, rg in zip(opt.param_groups, ropt.param_groups):
        if kind == "sgd":
            rtol, atol = (2e-4, 2e-5) if mode == "f16" else (2e-5, 1e-6)
            for p, r in zip(g["params"], rg["params"]):
                w = p.master if hasattr(p, "master") else p.data
                torch.testing.assert_close(w, r.detach(), rtol=rtol, atol=atol)
                if hasattr(p, "master"):
                    assert torch.equal(p.data, p.master.to(dt16))
        else:
            _check_state(opt, ropt, g["params"], rg["params"], g["lr"], dt16, l2=0.05 if kind == "adam" else 0.0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["sgd", "adam", "adamw"])
@pytest.mark.parametrize("max_norm", [1e9, 0.5])
def test_clipped_step_equals_torch_fed_the_clipped_gradients(mode, kind, max_norm):
    """Ten steps, two groups with different lr, one global norm.  torch's optimizer gets g.float() * coef with coef read back from the
    block after the step.  max_norm 1e9: coef == 1 and the result is bit-equal to the same optimizer without a clip; 0.5: the norm
    of ~20 k elements of N(0, 0.1) is ~14, every step clips."""
    lrs = (0.05, 0.02) if kind == "sgd" else (1e-3, 3e-4)
    mine, ref, dt16 = _make(SIZES, mode)
    opt, ropt = _build(kind, mine, ref, lrs, max_norm)
    plain_p, _, _ = _make(SIZES, mode)
    plain, _ = _build(kind, plain_p, [torch.nn.Parameter(torch.zeros(1, device=DEV)) for _ in SIZES], lrs, None)
    clip = opt.grad_clip
    coefs = []
    for s in range(10):
        gs = _grads(mine, s)
        for p, q, g in zip(mine, plain_p, gs):
            p.grad, q.grad = g, g.clone()
        opt.step()
        if max_norm > 1e8:
            plain.step()
        coef = clip.clip_coef.clone()
        coefs.append(float(coef))
        for r, g in zip(ref, gs):
            r.grad = g.float() * coef
        ropt.step()
    torch.cuda.synchronize()
    st = clip.stats()
    if max_norm > 1e8:
        assert coefs == [1.0] * 10 and st == {"calls": 10, "clipped": 0, "nonfinite": 0}
        for p, q in zip(mine, plain_p):
            assert torch.equal(p.master if hasattr(p, "master") else p.data, q.master if hasattr(q, "master") else q.data)
            assert torch.equal(p.data, q.data)
    else:
        assert all(0.0 < c < 0.1 for c in coefs) and st == {"calls": 10, "clipped": 10, "nonfinite": 0}
    _check_update(kind, mode, opt, ropt, dt16)
    if kind != "sgd":
        assert opt.group_steps() == [10.0, 10.0]


def _scaler_run():
    """Six fp16 steps of MasterAdamW with a clip under torch.amp.GradScaler (nobody calls unscale_: the kernels divide by the scale)
    next to torch.optim.AdamW on fp32 copies under scaler.unscale_ + clip_grad_norm_ + step; step 2 carries one Inf gradient."""
    from pytorch_retinanet_amd.optim import GradClip, MasterAdamW
    max_norm = 0.25
    mine, ref, dt16 = _make(SIZES[:10], "f16", seed=5)
    opt = MasterAdamW(mine, lr=1e-3, weight_decay=0.01, max_grad_norm=max_norm)
    ropt = torch.optim.AdamW(ref, lr=1e-3, weight_decay=0.01, foreach=False)
    sc, rsc = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10), torch.amp.GradScaler("cuda", init_scale=2.0 ** 10)
    gen = torch.Generator(device=DEV).manual_seed(8)
    for s in range(6):
        cs = [(torch.randn(p.shape, device=DEV, generator=gen) * 0.1).half().float() for p in mine]
        if s == 2:
            cs[3][0] = float("inf")
            snap = [((p.master if hasattr(p, "master") else p.data).clone(), p.data.clone(), opt.state[p]["exp_avg"].clone(),
                     opt.state[p]["exp_avg_sq"].clone()) for p in mine]
        opt.zero_grad(set_to_none=True)
        sc.scale(sum((p.float() * c).sum() for p, c in zip(mine, cs))).backward()
        sc.step(opt)
        sc.update()
        ropt.zero_grad(set_to_none=True)
        rsc.scale(sum((p.float() * c).sum() for p, c in zip(ref, cs))).backward()
        rsc.unscale_(ropt)
        t_64 = float(torch.linalg.vector_norm(torch.cat([r.grad.double().flatten() for r in ref])))
        t_total = float(torch.nn.utils.clip_grad_norm_(ref, max_norm))
        rsc.step(ropt)
        rsc.update()
        k_total, k_coef = float(opt.grad_clip.total_norm), float(opt.grad_clip.clip_coef)
        print(f"step {s}: norm float64 {t_64!r} kernel {k_total!r} torch {t_total!r}; coef kernel {k_coef!r} torch {GradClip.coef(t_total, max_norm)!r}")
        if s == 2:
            torch.cuda.synchronize()
            assert opt.group_steps() == [2.0] and opt.grad_clip.stats()["nonfinite"] == 1
            for p, (w, c16, m, v) in zip(mine, snap):
                assert torch.equal(p.master if hasattr(p, "master") else p.data, w) and torch.equal(p.data, c16)
                assert torch.equal(opt.state[p]["exp_avg"], m) and torch.equal(opt.state[p]["exp_avg_sq"], v)
    torch.cuda.synchronize()
    st = opt.grad_clip.stats()
    assert st == {"calls": 6, "clipped": 6, "nonfinite": 1}            # (the Inf step's coefficient is 0: it counts as clipped too)
    assert float(sc.get_scale()) == float(rsc.get_scale()) and opt.group_steps() == [5.0]
    return opt, ropt, mine, ref, dt16


def test_grad_scaler_skips_the_inf_step_and_counts_it():
    """fp16 copies under torch.amp.GradScaler with a clip: a step with one Inf gradient changes no master, moment, working copy or step
    counter and counts as non-finite in the block; afterwards the masters follow torch's unscale_ + clip_grad_norm_ + step run on fp32
    copies at test_master_adam_gpu.py's bar for the masters (2e-6 relative or 1e-3 * lr)."""
    from test_master_adam_gpu import _check_close
    opt, ropt, mine, ref, dt16 = _scaler_run()
    for i, (p, r) in enumerate(zip(mine, ref)):
        _check_close(p.master if hasattr(p, "master") else p.data, r.detach(), 1e-3, f"master {i}")
        if hasattr(p, "master"):
            assert torch.equal(p.data, p.master.to(dt16))


def test_grad_scaler_trajectory_follows_torch_unscale_clip_step():
    """The same run, masters AND moments at test_master_adam_gpu.py's bars (2 ulp on the moments) against torch's scaler.unscale_ +
    clip_grad_norm_ + step.  The two coefficients have to agree to the bit at every step for this: one ulp between them moves every
    clipped gradient of that step, and a moment element that nearly cancels carries it as an absolute error far above 2 ulp (205 was
    measured with fp32 lane sums in the norm kernel: at step 5 the exact norm 9.8905548830 lies 0.02 ulp below the middle of two fp32
    numbers, torch's norm took the nearer one and the kernel the farther).  With the squares summed in double from the first addition
    the kernel's fp32 norm is the correctly rounded one; _scaler_run prints float64's, the kernel's and torch's at every step."""
    opt, ropt, mine, ref, dt16 = _scaler_run()
    _check_state(opt, ropt, mine, ref, 1e-3, dt16)


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_captured_step_follows_max_norm_written_between_replays(kind):
    """opt.step() alone in a torch.cuda.graph, replayed with new gradients and clip.max_norm rewritten between replays, equals the
    eager sequence bit for bit (one capture: a max_norm baked into the graph fails this)."""
    lrs = (0.05, 0.02) if kind == "sgd" else (1e-3, 3e-4)
    a_p, _, _ = _make(SIZES[:12], "bf16", seed=3)
    b_p, _, _ = _make(SIZES[:12], "bf16", seed=3)
    dummy = lambda: [torch.nn.Parameter(torch.zeros(1, device=DEV)) for _ in range(12)]
    a, _ = _build(kind, a_p, dummy(), lrs, 1.0)
    b, _ = _build(kind, b_p, dummy(), lrs, 1.0)
    static = [torch.zeros_like(p) for p in a_p]
    for p, g in zip(a_p, static):
        p.grad = g
    norms = [1.0, 1.0, 0.05, 0.05, 1e6, 0.3, 2.0, 1e-3]
    graph, coefs = None, []
    for s, mn in enumerate(norms):
        gs = _grads(a_p, s)
        for g, x, q in zip(static, gs, b_p):
            g.copy_(x)
            q.grad = x
        a.grad_clip.max_norm = mn
        b.grad_clip.max_norm = mn
        if s == 0:
            a.step()                                                   # (creates the state and the clip's block)
        else:
            if graph is None:
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    a.step()                                           # (recorded, not run)
            if kind != "sgd":
                a.sync_device_hparams()
            graph.replay()
        b.step()
        coefs.append((float(a.grad_clip.clip_coef), float(b.grad_clip.clip_coef)))
    torch.cuda.synchronize()
    assert all(x == y for x, y in coefs), coefs
    assert coefs[4][0] == 1.0 and coefs[7][0] < coefs[5][0] < 1.0
    assert a.grad_clip.stats() == b.grad_clip.stats() and a.grad_clip.stats()["calls"] == len(norms)
    for p, q in zip(a_p, b_p):
        assert torch.equal(p.master if hasattr(p, "master") else p.data, q.master if hasattr(q, "master") else q.data)
        assert torch.equal(p.data, q.data)


def test_first_block_cannot_be_created_inside_a_capture():
    from pytorch_retinanet_amd.optim import MasterSGD
    p = torch.nn.Parameter(torch.randn(256, device=DEV))
    p.grad = torch.randn(256, device=DEV)
    opt = MasterSGD([p], lr=0.1, max_grad_norm=1.0)
    before = p.detach().clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="before capturing"):
        with torch.cuda.graph(graph):
            opt.step()
    torch.cuda.synchronize()
    assert torch.equal(p.detach(), before) and opt.grad_clip.stats()["calls"] == 0
    opt.step()                                                         # eagerly it works, and the device is usable
    torch.cuda.synchronize()
    assert opt.grad_clip.stats()["calls"] == 1 and not torch.equal(p.detach(), before)


def test_captured_train_step_with_a_clip_replays_one_graph():
    """CapturedTrainStep + MasterAdamW + GradClip + the per-step LambdaLR of test_master_adam_gpu.py's twin on R18, 8 batches: 1 capture, 6 replays, every step clipped, losses and weights
    within test_master_adam_gpu.py's bars of the eager run (MIOpen's atomically accumulated weight gradients: rtol 2e-2 / atol 2e-3)."""
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from pytorch_retinanet_amd.optim import MasterAdamW, use_bf16_conv_weights
    data = _batches(8, seed=5)
    res = {}
    for captured in (False, True):
        net = _r18(seed=11)
        use_bf16_conv_weights(net)
        opt = MasterAdamW(net.parameters(), lr=2e-4, weight_decay=1e-2, max_grad_norm=0.05)
        # (that test's warm-up schedule: Adam's update does not shrink with the clipped gradient, and at a constant 2e-4 this random-init
        # net's loss runs away from step 6 on -- 3.0 -> 12 -> 30 --, where the eager and the replayed run drift apart by more than
        # MIOpen's noise in either)
        sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: (s + 1) / 8)
        initial = _params(net)
        step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=2, enabled=captured)
        losses = []
        for im, tg in data:
            losses.append(float(step(im, tg)["loss"]))
            sch.step()
        torch.cuda.synchronize()
        res[captured] = (losses, _params(net), step.replays, step.captures, opt.group_steps(), opt.grad_clip.stats())
    assert res[False][2] == 0 and res[True][2] == len(data) - 2 and res[True][3] == 1
    assert res[True][2] >= 3 and res[True][4] == res[False][4] == [8.0]
    assert res[True][5] == res[False][5] == {"calls": 8, "clipped": 8, "nonfinite": 0}
    assert np.all(np.isfinite(res[True][0]))
    np.testing.assert_allclose(res[True][0], res[False][0], rtol=2e-2)
    for k, a in res[False][1].items():
        torch.testing.assert_close(res[True][1][k], a, rtol=0, atol=2e-3, msg=k)
    moved = sum(float((res[True][1][k] - initial[k]).abs().max()) > 0 for k in initial)
    assert moved > len(initial) // 2


@pytest.mark.parametrize("amp", ["bf16", "f16"])
def test_bucketed_ddp_world1_with_a_clip_equals_the_plain_clipped_step(amp):
    """BucketedGradAllReduce at world size 1 + MasterAdamW with a clip (the norm of the exchanged fp32 bucket views) == the plain
    clipped step; fp16: parallel.ExchangeGradScaler's step_exchanged against torch.amp.GradScaler.step (the bar of
    test_bucketed_ddp_world1_with_master_adamw_equals_plain_step)."""
    import pytorch_retinanet_amd as P
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from pytorch_retinanet_amd.optim import MasterAdamW, use_16bit_conv_weights
    dt = torch.bfloat16 if amp == "bf16" else torch.float16
    data = _batches(2)

    def run(use_ddp):
        net = _r18()
        use_16bit_conv_weights(net, dt)
        opt = MasterAdamW(net.parameters(), lr=1e-4, weight_decay=1e-2, max_grad_norm=0.05)
        ddp = P.BucketedGradAllReduce(net, bucket_mb=8.0) if use_ddp else None
        scaler = None
        if amp == "f16":
            scaler = P.ExchangeGradScaler("cuda", init_scale=256.0) if use_ddp else torch.amp.GradScaler("cuda", init_scale=256.0)
        step = CapturedTrainStep(net, opt, ddp, amp_dtype=dt, enabled=False, scaler=scaler)
        for images, targets in data:
            step(images, targets)
        torch.cuda.synchronize()
        return _params(net), opt.grad_clip.stats(), float(opt.grad_clip.total_norm)

    (a, sa, na), (b, sb, nb) = run(True), run(False)
    assert sa == sb == {"calls": 2, "clipped": 2, "nonfinite": 0}
    assert na == pytest.approx(nb, rel=2e-2)
    for k in a:
        torch.testing.assert_close(a[k], b[k], rtol=0, atol=5e-4, msg=k)


def _trainer_conf(opt_name, params):
    import pytorch_retinanet_amd as P
    torch.manual_seed(7)
    conf = P.load_hparams()
    conf.model.update(backbone_kind="resnet18", pretrained=False, num_classes=5, min_size=128, max_size=160)
    conf.dataset.kind = "synthetic"
    conf.dataset.update(length=12, height=128, width=160, boxes_per_image=3)
    conf.dataloader.train_bs = 2
    conf.dataloader.valid_bs = 2
    conf.dataloader.args.pin_memory = False
    conf.optimizer.class_name = opt_name
    conf.optimizer.params = params
    conf.scheduler.class_name = None
    model = P.RetinaNetModel(conf)
    model.prepare_data()
    model.val_ds = None
    return model


@pytest.mark.parametrize("name,params", [("MasterSGD", {"lr": 1e-3, "momentum": 0.9, "weight_decay": 1e-3}),
                                         ("MasterAdamW", {"lr": 1e-4, "weight_decay": 1e-2})])
def test_simple_trainer_clips_inside_the_captured_step(name, params):
    import logging
    import pytorch_retinanet_amd as P
    from pytorch_retinanet_amd.optim import GradClip
    model = _trainer_conf("pytorch_retinanet_amd.optim." + name, params)
    trainer = P.SimpleTrainer(max_epochs=1, device=DEV, gradient_clip_val=1e-3, log_every=1)
    lines = []
    handler = logging.Handler()
    handler.emit = lambda rec: lines.append(rec.getMessage())
    trainer.log.addHandler(handler)
    old = trainer.log.level
    trainer.log.setLevel(logging.INFO)
    try:
        steps = trainer.fit(model)
    finally:
        trainer.log.removeHandler(handler)
        trainer.log.setLevel(old)
    assert steps == 6 and trainer.captured_steps > 0, (steps, trainer.captured_steps)
    assert isinstance(trainer.grad_clip, GradClip) and trainer.grad_clip is model.optimizer.grad_clip
    assert trainer.grad_clip.max_norm == 1e-3
    assert trainer.grad_clip.stats() == {"calls": steps, "clipped": steps, "nonfinite": 0}
    step_lines = [l for l in lines if "grad_norm" in l and "loss" in l]
    assert len(step_lines) == steps, lines
    assert all(math.isfinite(float(l.split("grad_norm")[1].split()[0])) for l in step_lines)


def test_simple_trainer_falls_back_to_torch_clipping_for_other_optimizers():
    import pytorch_retinanet_amd as P
    weights = {}
    for clip_val in (0.0, 1e-3):
        model = _trainer_conf("torch.optim.SGD", {"lr": 1e-2, "momentum": 0.9})
        trainer = P.SimpleTrainer(max_epochs=1, device=DEV, gradient_clip_val=clip_val)
        steps = trainer.fit(model)
        assert steps == 6 and trainer.grad_clip is None
        if clip_val:
            assert trainer.captured_steps == 0                         # the torch fallback runs eagerly
        weights[clip_val] = _params(model.net)
    first = {k: float((weights[0.0][k] - weights[1e-3][k]).abs().max()) for k in weights[0.0]}
    assert sum(v > 0 for v in first.values()) > len(first) // 2
    assert all(torch.isfinite(v).all() for v in weights[1e-3].values())


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_norm_and_clipped_steps_stay_inside_their_operands(dt):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "guard_probe.py"), "clip", dt], capture_output=True, text=True,
                       env=env, timeout=300, cwd=ROOT)
    tail = (r.stdout + r.stderr)[-1500:]
    assert r.returncode == 0, f"probe clip died (GPU memory access fault?):\n{tail}"
    assert "ok clip" in r.stdout, tail
