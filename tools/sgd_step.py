#!/usr/bin/env python3
"""MasterSGD with its hyperparameters in a device block (capturable=True, rn_sgd_master_step_dev) against the by-value step.

  (a) the optimizer step alone on R50-FPN's parameter set (conv weights bf16 with fp32 masters, bf16 gradients; BN / biases fp32):
      each form captured in a graph of its own, replayed as interleaved pairs (by value, device block, by value, ...), ``--pairs``
      pairs of ``--opt-iters`` replays each: us per step of both, and the pair-to-pair spread of each;
  (b) bench.py's step -- R50-FPN, bf16 autocast, B = 8 at 3 x 800 x 1333, graph.CapturedTrainStep -- under a per-step LambdaLR
      warm-up, with capturable=True (one graph, replayed) and with capturable=False (every new lr is a new graph key: run eagerly,
      as SimpleTrainer does): ms per step, host ms per step, captures and replays.
Prints one JSON line (and writes it to ``--out`` when given).

usage: sgd_step.py [--steps 20] [--warmup 4] [--rounds 2] [--pairs 7] [--opt-iters 100] [--skip-train] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import synth                                                        # noqa: E402
import pytorch_retinanet_amd as P                                   # noqa: E402
from pytorch_retinanet_amd import tuning                            # noqa: E402
from pytorch_retinanet_amd.graph import CapturedTrainStep           # noqa: E402
from pytorch_retinanet_amd.optim import MasterSGD, use_16bit_conv_weights   # noqa: E402

B, H, W = 8, 800, 1333
KW = dict(lr=1e-3, momentum=0.9, weight_decay=1e-4)


def r50(dev):
    torch.manual_seed(0)
    net = P.Retinanet(num_classes=90, backbone_kind="resnet50", pretrained=False, min_size=800, max_size=1333)
    net = net.to(dev).to(memory_format=torch.channels_last).train()
    use_16bit_conv_weights(net, torch.bfloat16)
    return net


def captured_optimizer(net, capturable):
    "One MasterSGD on copies of the net's parameters with random gradients, one eager step, then its step captured alone."
    g = torch.Generator(device=next(net.parameters()).device).manual_seed(1)
    params = []                                                     # (copies: random gradients would wreck the model's weights)
    for p in net.parameters():
        q = torch.nn.Parameter(p.detach().clone(memory_format=torch.preserve_format))
        if hasattr(p, "master"):
            q.master = p.master.detach().clone(memory_format=torch.preserve_format)
        x = (torch.randn(p.shape, device=p.device, generator=g) * 1e-3).to(p.dtype)
        q.grad = x.contiguous(memory_format=torch.channels_last) if p.dim() == 4 else x
        params.append(q)
    opt = MasterSGD(params, capturable=capturable, **KW)
    opt.step()                                                      # (state)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    return graph, opt, params


def replay_us(graph, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        graph.replay()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e3


def timed(name, stepper, images, batches, sched):
    torch.cuda.synchronize()
    host = 0.0
    t0 = time.perf_counter()
    for tg in batches:
        h0 = time.perf_counter()
        out = stepper(images, tg)
        sched.step()
        host += time.perf_counter() - h0
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    assert np.isfinite(float(out["loss"])), f"{name}: non-finite loss"
    return wall / len(batches) * 1e3, host / len(batches) * 1e3


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--opt-iters", type=int, default=100)
    ap.add_argument("--skip-train", action="store_true", help="only (a), the optimizer step alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    tuning.use_shipped_miopen_db(0)
    tuning.enable_conv_autotune()
    net = r50(dev)
    n_params = sum(p.numel() for p in net.parameters())
    n_tensors = sum(1 for _ in net.parameters())

    # (a) the optimizer step alone, interleaved pairs
    forms = {"by_value": captured_optimizer(net, False), "device_block": captured_optimizer(net, True)}
    us = {k: [] for k in forms}
    for _ in range(args.pairs):
        for k, (graph, _, _) in forms.items():
            us[k].append(replay_us(graph, args.opt_iters))
    alone = {k: {"us_per_step_median": round(float(np.median(v)), 2), "us_per_step_min": round(min(v), 2), "us_per_step_max": round(max(v), 2),
                 "per_pair_us": [round(x, 2) for x in v]} for k, v in us.items()}
    diffs = [d - b for b, d in zip(us["by_value"], us["device_block"])]
    line = {"tool": "sgd_step", "optimizer_alone": alone, "pairs": args.pairs, "opt_iters": args.opt_iters,
            "device_block_minus_by_value_us": {"median": round(float(np.median(diffs)), 2), "min": round(min(diffs), 2), "max": round(max(diffs), 2)},
            "by_value_pair_to_pair_spread_us": round(max(us["by_value"]) - min(us["by_value"]), 2),
            "workload": f"R50-FPN parameter set: {n_tensors} tensors, {n_params} elements; train step B={B} at 3x{H}x{W}, bf16, T=8"}
    del forms

    # (b) the scheduled train step: capturable (replayed) against by value (eager)
    if not args.skip_train:
        g = torch.Generator().manual_seed(0)
        images = [torch.rand(3, H, W, generator=g).to(dev) for _ in range(B)]
        rng = np.random.default_rng(7)
        tg = []
        for _ in range(B):
            b, l = synth.gt_boxes(rng, 8, H, W)
            tg.append({"boxes": torch.from_numpy(b).to(dev), "labels": torch.from_numpy(l).to(dev)})
        batches = [tg] * (args.warmup + args.steps)
        phases = {}
        for name, capturable in (("capturable_lambdalr", True), ("by_value_lambdalr_eager", False)):
            opt = MasterSGD(net.parameters(), capturable=capturable, **KW)
            sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: min(1.0, (s + 1) / 1000))
            phases[name] = (CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=2, enabled=capturable), sched, opt)
        res = {k: [] for k in phases}
        for _ in range(args.rounds):
            for k, (st, sc, _) in phases.items():
                for b in batches[:args.warmup]:
                    st(images, b)
                    sc.step()
                res[k].append(timed(k, st, images, batches[args.warmup:], sc))
        line.update({"steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
                     "train_ms_per_step": {k: round(float(np.mean([v[0] for v in res[k]])), 3) for k in res},
                     "host_ms_per_step": {k: round(float(np.mean([v[1] for v in res[k]])), 3) for k in res},
                     "per_round_ms": {k: [round(v[0], 3) for v in res[k]] for k in res},
                     "captures": {k: phases[k][0].captures for k in phases}, "replays": {k: phases[k][0].replays for k in phases},
                     "final_lr": {k: phases[k][2].param_groups[0]["lr"] for k in phases},
                     "device_steps": phases["capturable_lambdalr"][2].group_steps()})
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
