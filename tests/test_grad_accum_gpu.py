"""GPU: gradient accumulation into fp32 accumulators -- ``rn_grad_accumulate`` (csrc/accum.hip) against its torch restatement bit
for bit, found_inf over a window under a loss scaler, the three master optimizers stepping on the accumulators, the precision of
the fp32 sum against autograd's 16-bit ``.grad +=``, ``graph.CapturedTrainStep(accumulate=)`` against its eager self, the
accumulated ``MasterSGD`` trajectory against torch's ``(loss / N).backward()``, ``SimpleTrainer(accumulate_grad_batches=)``, and
the out-of-bounds guard.

Bars: everything that only re-orders nothing is bit-equal (the kernel's arithmetic is fixed: ``acc = (pos == 0 ? 0 : acc) +
float(g) * float(1 / N)``, two roundings); captured against eager at tests/test_graph_gpu.py's bars (losses rtol 2e-2, weights atol
2e-3: MIOpen's atomically accumulated weight gradients); against torch at the bar of
``test_master_sgd_follows_torch_sgd_under_autocast`` (rtol 2e-5, atol 1e-6)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import synth
from test_master_adam_gpu import SIZES, _make, _params, _r18

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 16384
MODES = ["bf16", "f16"]


def _mixed_params(mode, seed=0):
    """Flat tensors of 1, 7, 4097 and CHUNK + 1 elements (twice each: a 16-bit working copy with its fp32 master and 16-bit gradients,
    and a plain fp32 parameter) plus two channels-last 4-D conv weights, 16-bit."""
    dt = torch.bfloat16 if mode == "bf16" else torch.float16
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = []
    for n in (1, 7, 4097, CHUNK + 1):
        w = torch.randn(n, device=DEV, generator=g)
        p = torch.nn.Parameter(w.to(dt))
        p.master = w.clone()
        out += [p, torch.nn.Parameter(w.clone())]
    for shape in ((16, 8, 3, 3), (5, 3, 1, 1)):
        w = torch.randn(shape, device=DEV, generator=g).contiguous(memory_format=torch.channels_last)
        p = torch.nn.Parameter(w.to(dt))
        p.master = w.clone()
        out.append(p)
    return out


def _rand_grads(params, seed, scale=0.1):
    g = torch.Generator(device=DEV).manual_seed(2000 + seed)
    return [(torch.randn(p.shape, device=DEV, generator=g) * scale).to(p.dtype).contiguous(
        memory_format=torch.channels_last if p.dim() == 4 else torch.contiguous_format) for p in params]


def _restated(grad_sets, n):
    "acc = acc + g.float() * float32(1 / n), from zero, in torch"
    w = torch.tensor(1.0 / n, dtype=torch.float32, device=DEV)
    acc = [torch.zeros(g.shape, dtype=torch.float32, device=DEV) for g in grad_sets[0]]
    for gs in grad_sets:
        acc = [a + g.float() * w for a, g in zip(acc, gs)]
    return acc


def _window(acc, params, grad_sets):
    for k, gs in enumerate(grad_sets):
        for p, g in zip(params, gs):
            p.grad = g
        assert acc.accumulate(params) == len(params)
        acc.advance(k == len(grad_sets) - 1)


# ---- 1. the kernel against its restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [2, 3, 8])
def test_kernel_equals_its_restatement_bit_for_bit_over_ten_windows(mode, n):
    from pytorch_retinanet_amd.optim import GradAccumulator
    params = _mixed_params(mode)
    grad_sets = [_rand_grads(params, k) for k in range(n)]
    want = _restated(grad_sets, n)
    acc = GradAccumulator(n)
    _window(acc, params, grad_sets)                      # (creates the accumulators and the block)
    views = acc.grad_views()
    assert set(views) == set(params)
    for p in params:
        a = views[p]
        assert a.dtype == torch.float32 and a.stride() == (p.master if hasattr(p, "master") else p.data).stride()
    first = None
    for rep in range(10):
        for a in views.values():
            a.fill_(float("nan"))                        # pos == 0 overwrites: nothing of this survives
        _window(acc, params, grad_sets)
        torch.cuda.synchronize()
        got = [views[p].clone() for p in params]
        for i, (a, r) in enumerate(zip(got, want)):
            assert torch.equal(a, r), (rep, i, float((a - r).abs().max()))
        if first is None:
            first = got
        assert all(torch.equal(a, b) for a, b in zip(got, first))
    assert acc.position == 0 and float(acc.found_inf()) == 0.0
    assert acc.stats() == {"windows": 11, "nonfinite": 0, "micro_batches": 11 * n}


def test_position_follows_and_n_is_rewritten_between_windows_only():
    from pytorch_retinanet_amd.optim import GradAccumulator
    params = _mixed_params("bf16", seed=2)
    acc = GradAccumulator(3)
    gs = [_rand_grads(params, k) for k in range(3)]
    for p, g in zip(params, gs[0]):
        p.grad = g
    acc.accumulate(params)
    acc.advance(False)
    assert acc.position == 1 and not acc.next_is_final()
    with pytest.raises(RuntimeError, match="mid-window"):
        acc.n = 2
    acc.accumulate(params)
    acc.advance(True)                                    # a short window (the end of an epoch): still weighted 1 / 3
    torch.cuda.synchronize()
    w3 = torch.tensor(1.0 / 3, dtype=torch.float32, device=DEV)
    for p, g in zip(params, gs[0]):
        assert torch.equal(acc.grad_views()[p], (torch.zeros_like(g, dtype=torch.float32) + g.float() * w3) + g.float() * w3)
    acc.n = 2                                            # one tiny launch; the next window is weighted 1 / 2
    _window(acc, params, gs[:2])
    torch.cuda.synchronize()
    for a, r in zip([acc.grad_views()[p] for p in params], _restated(gs[:2], 2)):
        assert torch.equal(a, r)
    assert acc.stats() == {"windows": 2, "nonfinite": 0, "micro_batches": 4}


def test_first_accumulate_cannot_happen_inside_a_capture():
    from pytorch_retinanet_amd.optim import GradAccumulator
    p = torch.nn.Parameter(torch.randn(256, device=DEV))
    p.grad = torch.randn(256, device=DEV)
    acc = GradAccumulator(2)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="before capturing"):
        with torch.cuda.graph(graph):
            acc.accumulate([p])
    torch.cuda.synchronize()
    assert acc.stats()["micro_batches"] == 0
    assert acc.accumulate([p]) == 1                      # eagerly it works, and the device is usable
    acc.advance(False)
    torch.cuda.synchronize()
    assert acc.position == 1


# ---- 2. found_inf over a window -------------------------------------------------------------------------------------------------------
def test_found_inf_survives_to_the_final_step_and_is_cleared_by_the_next_window():
    from pytorch_retinanet_amd.optim import GradAccumulator, MasterSGD
    from pytorch_retinanet_amd.parallel import ExchangeGradScaler
    params, _, dt16 = _make(SIZES[:10], "f16", seed=4)
    opt = MasterSGD(params, lr=0.05, momentum=0.9)
    scaler = ExchangeGradScaler("cuda", init_scale=2.0 ** 10, growth_interval=1000)
    scaler.scale(torch.ones(1, device=DEV))              # (creates the scale tensor, as the first scaled loss does)
    acc = GradAccumulator(4)

    def window(inf_at):
        seen = []
        for k in range(4):
            for p, g in zip(params, _rand_grads(params, 10 + k)):
                p.grad = (g.float() * 2.0 ** 10).to(p.dtype)
            if k == inf_at:
                params[3].grad[0] = float("inf")
            acc.accumulate(params)
            seen.append(float(acc.found_inf()))
            if k == 3:
                scaler.step_exchanged(opt, acc)
                scaler.update()
            acc.advance(k == 3)
        torch.cuda.synchronize()
        return seen

    snap = [((p.master if hasattr(p, "master") else p.data).clone(), p.data.clone()) for p in params]
    assert window(inf_at=1) == [0.0, 1.0, 1.0, 1.0]      # micro-batch 2 of 4 sets it; it survives micro-batches 3 and 4
    for p, (w, c) in zip(params, snap):                  # the optimizer changed nothing ...
        assert torch.equal(p.master if hasattr(p, "master") else p.data, w) and torch.equal(p.data, c)
    assert float(scaler.get_scale()) == 2.0 ** 9         # ... and the scaler backed off, once
    assert float(acc.found_inf()) == 0.0 and acc.position == 0
    assert acc.stats() == {"windows": 1, "nonfinite": 1, "micro_batches": 4}
    assert window(inf_at=None) == [0.0, 0.0, 0.0, 0.0]   # cleared by the next window's start
    moved = sum(not torch.equal(p.master if hasattr(p, "master") else p.data, w) for p, (w, _) in zip(params, snap))
    assert moved == len(params) and float(scaler.get_scale()) == 2.0 ** 9
    assert acc.stats() == {"windows": 2, "nonfinite": 1, "micro_batches": 8}
    for p in params:
        if hasattr(p, "master"):
            assert torch.equal(p.data, p.master.to(dt16)) and bool(torch.isfinite(p.master).all())


# ---- 3. the optimizers on grad_views() ------------------------------------------------------------------------------------------------
class _Restated:
    "What step_exchanged takes in place of the accumulator: the restated sums and a clean found_inf."

    def __init__(self, views):
        self.views = views

    def grad_views(self):
        return self.views

    def found_inf(self):
        return torch.zeros((), dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("clip", [None, 0.05])
@pytest.mark.parametrize("kind", ["sgd", "adam", "adamw"])
def test_step_on_the_accumulators_equals_the_step_on_the_restated_sum(kind, clip, mode):
    """Two windows of N = 3: the optimizer stepping on grad_views() (fp16: through ExchangeGradScaler.step_exchanged) against the same
    optimizer stepping with grads= the restated fp32 sums -- masters, 16-bit copies and optimizer state bit-equal."""
    from pytorch_retinanet_amd.optim import GradAccumulator, MasterAdam, MasterAdamW, MasterSGD
    from pytorch_retinanet_amd.parallel import ExchangeGradScaler
    n, S = 3, 256.0
    a_p, _, _ = _make(SIZES[:12], mode, seed=6)
    b_p, _, _ = _make(SIZES[:12], mode, seed=6)

    def build(ps):
        if kind == "sgd":
            return MasterSGD(ps, lr=0.05, momentum=0.9, weight_decay=1e-2, max_grad_norm=clip)
        return (MasterAdam if kind == "adam" else MasterAdamW)(ps, lr=1e-3, weight_decay=0.01, max_grad_norm=clip)
    a, b = build(a_p), build(b_p)
    scalers = None
    if mode == "f16":
        scalers = [ExchangeGradScaler("cuda", init_scale=S, growth_interval=1000) for _ in range(2)]
        for sc in scalers:
            sc.scale(torch.ones(1, device=DEV))
    acc = GradAccumulator(n)
    for win in range(2):
        grad_sets = [_rand_grads(a_p, 10 * win + k) for k in range(n)]
        if mode == "f16":
            grad_sets = [[(g.float() * S).to(g.dtype) for g in gs] for gs in grad_sets]       # (scaled by the GradScaler's 256: exact)
        for k, gs in enumerate(grad_sets):
            for p, g in zip(a_p, gs):
                p.grad = g
            acc.accumulate(a_p)
            if k == n - 1:
                if scalers:
                    scalers[0].step_exchanged(a, acc)
                    scalers[0].update()
                else:
                    a.step(grads=acc.grad_views())
            acc.advance(k == n - 1)
        want = dict(zip(b_p, _restated(grad_sets, n)))
        if scalers:
            scalers[1].step_exchanged(b, _Restated(want))
            scalers[1].update()
        else:
            b.step(grads=want)
    torch.cuda.synchronize()
    if clip is not None:
        assert a.grad_clip.stats() == b.grad_clip.stats() and a.grad_clip.stats()["calls"] == 2      # the norm of the sum, once per window
        assert float(a.grad_clip.total_norm) == float(b.grad_clip.total_norm)
    for p, q in zip(a_p, b_p):
        assert torch.equal(p.master if hasattr(p, "master") else p.data, q.master if hasattr(q, "master") else q.data)
        assert torch.equal(p.data, q.data)
        for key in ("momentum_buffer", "exp_avg", "exp_avg_sq"):
            if key in a.state[p]:
                assert torch.equal(a.state[p][key], b.state[q][key]), key
    moved, _, _ = _make(SIZES[:12], mode, seed=6)
    master = lambda p: p.master if hasattr(p, "master") else p.data
    assert all(not torch.equal(master(p), master(m)) for p, m in zip(a_p, moved))            # (and the two windows really stepped)


# ---- 4. the precision claim -------------------------------------------------------------------------------------------------------------
def test_fp32_accumulator_is_closer_to_float64_than_the_bf16_grad_sum():
    """N = 8, the same eight bf16 gradients: the fp32 accumulator (times 8: exact) and autograd's bf16 ``.grad +=`` running sum, each
    against the float64 sum.  An ordering, not a tuned bar."""
    from pytorch_retinanet_amd.optim import GradAccumulator
    g = torch.Generator(device=DEV).manual_seed(21)
    w = torch.randn(64, 32, 3, 3, device=DEV, generator=g).contiguous(memory_format=torch.channels_last)
    p = torch.nn.Parameter(w.to(torch.bfloat16))
    p.master = w
    grads = [(torch.randn(w.shape, device=DEV, generator=g) * 0.1).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
             for _ in range(8)]
    acc = GradAccumulator(8)
    _window(acc, [p], [[x] for x in grads])
    exact = sum(x.double() for x in grads)
    running = grads[0].clone()
    for x in grads[1:]:
        running += x                                     # what .grad += does: a bf16 add per micro-batch
    torch.cuda.synchronize()
    err_acc = float((acc.grad_views()[p].double() * 8.0 - exact).abs().max())
    err_16 = float((running.double() - exact).abs().max())
    print(f"N=8 max abs error against float64: fp32 accumulator {err_acc:.3e}, bf16 .grad += {err_16:.3e}")
    assert err_acc < err_16


# ---- 5. captured = eager ----------------------------------------------------------------------------------------------------------------
def _batches_with_counts(counts, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    for T in counts:
        images = [torch.from_numpy(rng.random((3, 128, 160), dtype=np.float32)).to(DEV) for _ in range(2)]
        targets = []
        for _ in range(2):
            b, l = synth.gt_boxes(rng, T, 128, 160, num_classes=5, wh_lo=20.0, wh_hi=90.0)
            targets.append({"boxes": torch.from_numpy(b).to(DEV), "labels": torch.from_numpy(l).to(DEV)})
        out.append((images, targets))
    return out


def test_captured_accumulating_step_equals_the_eager_one():
    """R18, B = 2, N = 3, 7 batches = two windows and a leftover stepped as the end of an epoch, GT counts of two capacity classes
    (3 boxes: class 8; 12 boxes: class 32) under gt_capacity="auto"; then n = 2 written between windows and one more window."""
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from pytorch_retinanet_amd.optim import GradAccumulator, MasterSGD, use_bf16_conv_weights
    counts = [3, 3, 3, 12, 12, 12, 3, 3, 3]
    finals = [False, False, True, False, False, True, True, False, True]      # batch 7: the leftover; 8-9: the window at n = 2
    data = _batches_with_counts(counts)
    res = {}
    for captured in (False, True):
        net = _r18(seed=11)
        use_bf16_conv_weights(net)
        opt = MasterSGD(net.parameters(), lr=1e-2, momentum=0.9, weight_decay=1e-3, max_grad_norm=10.0)
        acc = GradAccumulator(3)
        initial = _params(net)
        step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=1, enabled=captured, gt_capacity="auto", accumulate=acc)
        losses = []
        for i, ((im, tg), final) in enumerate(zip(data, finals)):
            if i == 7:
                before = step.captures
                acc.n = 2                                # between windows: one tiny launch, no capture
            # batches 1-6 and 8-9 by the accumulator's own count, the leftover by the caller
            losses.append(float(step(im, tg, final=True if i == 6 else None)["loss"]))
            if i == 6:
                seven = (step.replays, step.captures, len(step._entries))
        torch.cuda.synchronize()
        res[captured] = (losses, _params(net), seven, step.replays, step.captures - before, acc.stats(), opt.grad_clip.stats())
    # eager warm-ups: one per (signature, kind) met -- (A, micro), (A, final), (B, micro), (B, final): batches 1, 3, 4, 6
    replays7, captures7, signatures = res[True][2]
    assert res[False][3] == 0 and replays7 >= 7 - 4 and signatures == 2 and captures7 <= 2 * signatures
    assert res[True][4] == 0 and res[True][3] == replays7 + 2          # n = 2: both batches replayed, nothing re-captured
    assert res[True][5] == res[False][5] == {"windows": 4, "nonfinite": 0, "micro_batches": 9}
    assert res[True][6] == res[False][6] and res[True][6]["calls"] == 4      # the clip saw the accumulated gradients, once per window
    la, lb = np.array(res[False][0]), np.array(res[True][0])
    assert np.all(np.isfinite(lb))
    np.testing.assert_allclose(lb, la, rtol=2e-2)                      # tests/test_graph_gpu.py's comparison of captured and eager
    for k, a in res[False][1].items():
        torch.testing.assert_close(res[True][1][k], a, rtol=0, atol=2e-3, msg=k)
    moved = sum(float((res[True][1][k] - initial[k]).abs().max()) > 0 for k in initial)
    assert moved > len(initial) // 2


# ---- 6. against torch's semantics -------------------------------------------------------------------------------------------------------
def test_accumulated_master_sgd_follows_torch_sgd_with_loss_over_n():
    """The toy model, optimizer settings and bar of test_master_sgd_follows_torch_sgd_under_autocast (tests/test_model_gpu.py), N = 4
    with four different inputs per window, three windows: torch accumulates (loss / 4).backward() into fp32 .grad, MasterSGD steps on
    the accumulator.  1 / 4 is an exact scaling, so only the fp32 summation order differs."""
    from pytorch_retinanet_amd.norm import FusedBatchNorm2d
    from pytorch_retinanet_amd.optim import GradAccumulator, MasterSGD, master_state_dict, use_bf16_conv_weights

    def make():
        torch.manual_seed(11)
        m = torch.nn.Sequential(torch.nn.Conv2d(8, 16, 3, padding=1), FusedBatchNorm2d(16), torch.nn.ReLU(),
                                torch.nn.Conv2d(16, 8, 1, bias=False)).to(DEV).to(memory_format=torch.channels_last)
        return m.train()
    a, b = make(), make()
    kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-2)
    oa = torch.optim.SGD(a.parameters(), **kw)
    assert use_bf16_conv_weights(b) == 2
    ob = MasterSGD(b.parameters(), **kw)
    acc = GradAccumulator(4)
    g = torch.Generator(device=DEV).manual_seed(3)
    for _ in range(3):
        oa.zero_grad(set_to_none=True)
        for k in range(4):
            x = torch.randn(4, 8, 12, 10, device=DEV, generator=g).contiguous(memory_format=torch.channels_last)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = (a(x).float() ** 2).mean()
            (loss / 4).backward()
            ob.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = (b(x).float() ** 2).mean()
            loss.backward()
            acc.accumulate(b.parameters())
            if k == 3:
                ob.step(grads=acc.grad_views())
            acc.advance(k == 3)
        oa.step()
    sa, sb = a.state_dict(), master_state_dict(b)
    for k in sa:
        torch.testing.assert_close(sb[k].float(), sa[k].float(), rtol=2e-5, atol=1e-6, msg=k)
    assert torch.equal(b[0].weight.float(), sb["0.weight"].to(torch.bfloat16).float())
    assert acc.stats() == {"windows": 3, "nonfinite": 0, "micro_batches": 12}


# ---- 7. the trainer ---------------------------------------------------------------------------------------------------------------------
def _trainer_conf(opt_name, params, length=18):
    import pytorch_retinanet_amd as P
    torch.manual_seed(7)
    conf = P.load_hparams()
    conf.model.update(backbone_kind="resnet18", pretrained=False, num_classes=5, min_size=128, max_size=160)
    conf.dataset.kind = "synthetic"
    conf.dataset.update(length=length, height=128, width=160, boxes_per_image=3)
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
                                         ("MasterAdam", {"lr": 1e-4}),
                                         ("MasterAdamW", {"lr": 1e-4, "weight_decay": 1e-2})])
def test_simple_trainer_accumulates_inside_the_captured_step(name, params):
    import pytorch_retinanet_amd as P
    from pytorch_retinanet_amd.optim import GradAccumulator
    model = _trainer_conf("pytorch_retinanet_amd.optim." + name, params)          # 9 batches per epoch
    before = _params(model.net)
    trainer = P.SimpleTrainer(max_epochs=2, device=DEV, accumulate_grad_batches=4)
    steps = trainer.fit(model)
    per_epoch = math.ceil(9 / 4)
    assert steps == 2 * per_epoch and trainer.captured_steps > 0, (steps, trainer.captured_steps)
    acc = trainer.grad_accumulator
    assert isinstance(acc, GradAccumulator) and acc.n == 4 and acc.position == 0
    assert acc.stats() == {"windows": 2 * per_epoch, "nonfinite": 0, "micro_batches": 18}
    if name != "MasterSGD":
        assert model.optimizer.group_steps() == [float(2 * per_epoch)]            # the optimizer's own device counter
    after = _params(model.net)
    assert all(bool(torch.isfinite(v).all()) for v in after.values())
    assert sum(float((after[k] - before[k]).abs().max()) > 0 for k in after) > len(after) // 2


def test_simple_trainer_accumulates_under_fp16_with_the_exchange_scaler():
    import pytorch_retinanet_amd as P
    model = _trainer_conf("pytorch_retinanet_amd.optim.MasterSGD", {"lr": 1e-3, "momentum": 0.9}, length=16)
    trainer = P.SimpleTrainer(max_epochs=1, device=DEV, precision="16", accumulate_grad_batches=4)
    assert trainer.fit(model) == 2
    st = trainer.grad_accumulator.stats()
    assert st["windows"] == 2 and st["micro_batches"] == 8


def test_simple_trainer_falls_back_to_eager_accumulation_for_other_optimizers():
    import pytorch_retinanet_amd as P
    weights = {}
    for n in (1, 4):
        model = _trainer_conf("torch.optim.SGD", {"lr": 1e-2, "momentum": 0.9})
        trainer = P.SimpleTrainer(max_epochs=1, device=DEV, accumulate_grad_batches=n)
        steps = trainer.fit(model)
        assert steps == math.ceil(9 / n) and trainer.grad_accumulator is None
        if n > 1:
            assert trainer.captured_steps == 0                                     # the plain thing, eagerly
        weights[n] = _params(model.net)
    diff = {k: float((weights[1][k] - weights[4][k]).abs().max()) for k in weights[1]}
    assert sum(v > 0 for v in diff.values()) > len(diff) // 2
    assert all(bool(torch.isfinite(v).all()) for v in weights[4].values())


def test_simple_trainer_refuses_accumulation_under_torch_distributed(tmp_path):
    import torch.distributed as dist
    import pytorch_retinanet_amd as P
    model = _trainer_conf("pytorch_retinanet_amd.optim.MasterSGD", {"lr": 1e-3, "momentum": 0.9})
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'rendezvous'}", rank=0, world_size=1)
    try:
        with pytest.raises(ValueError, match="single-process"):
            P.SimpleTrainer(max_epochs=1, device=DEV, accumulate_grad_batches=4).fit(model)
    finally:
        dist.destroy_process_group()


# ---- 8. the guard -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_accumulate_stays_inside_its_operands(dt):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "guard_probe.py"), "accum", dt], capture_output=True, text=True,
                       env=env, timeout=300, cwd=ROOT)
    tail = (r.stdout + r.stderr)[-1500:]
    assert r.returncode == 0, f"probe accum died (GPU memory access fault?):\n{tail}"
    assert "ok accum" in r.stdout, tail
