#!/usr/bin/env python3
"""Adam / AdamW on fp32 masters (optim.MasterAdamW, csrc/adam.hip) against MasterSGD, alone and inside the train step.

  (a) the optimizer step alone on R50-FPN's parameter set (conv weights bf16 with fp32 masters, bf16 gradients; BN / biases fp32),
      captured in a graph and replayed: us per step, bytes moved (SGD with momentum 20 B, Adam 28 B per element), fraction of
      the 6.29 TB/s copy ceiling;
  (b) bench.py's step -- R50-FPN, bf16 autocast, B = 8 at 3 x 800 x 1333, graph.CapturedTrainStep -- with MasterSGD, with MasterAdamW,
      and with MasterAdamW under a per-step LambdaLR (warmup): ms per step, host ms per step, captures and replays;
  (c) the same step with fp32 parameters and torch.optim.AdamW (its step cannot be captured: every step runs eagerly).
The train-step phases run interleaved for ``--rounds`` rounds; ms/step is wall time over ``--steps`` steps with the device drained
at both ends, host ms/step the time the calls take to return.  Prints one JSON line (and writes it to ``--out`` when given).

usage: adam_step.py [--steps 20] [--warmup 4] [--rounds 2] [--opt-iters 200] [--out FILE]"""
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
from pytorch_retinanet_amd.optim import MasterAdamW, MasterSGD, use_16bit_conv_weights   # noqa: E402

B, H, W = 8, 800, 1333
CEILING_TBS = 6.29


def r50(dev, convert: bool):
    torch.manual_seed(0)
    net = P.Retinanet(num_classes=90, backbone_kind="resnet50", pretrained=False, min_size=800, max_size=1333)
    net = net.to(dev).to(memory_format=torch.channels_last).train()
    if convert:
        use_16bit_conv_weights(net, torch.bfloat16)
    return net


def optimizer_alone(net, make_opt, per_elem_bytes, iters):
    "One optimizer's step, captured alone and replayed ``iters`` times: (us per step, bytes per step)."
    g = torch.Generator(device=net.parameters().__next__().device).manual_seed(1)
    params = []                                                     # (copies: random gradients would wreck the model's weights)
    for p in net.parameters():
        q = torch.nn.Parameter(p.detach().clone(memory_format=torch.preserve_format))
        if hasattr(p, "master"):
            q.master = p.master.detach().clone(memory_format=torch.preserve_format)
        params.append(q)
    for p in params:
        p.grad = (torch.randn(p.shape, device=p.device, generator=g) * 1e-3).to(p.dtype).contiguous(memory_format=torch.channels_last) \
            if p.dim() == 4 else (torch.randn(p.shape, device=p.device, generator=g) * 1e-3).to(p.dtype)
    opt = make_opt(params)
    opt.step()                                                      # (state)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        graph.replay()
    t1.record()
    torch.cuda.synchronize()
    us = t0.elapsed_time(t1) / iters * 1e3
    nbytes = sum(p.numel() for p in params) * per_elem_bytes
    del graph, params, opt
    return us, nbytes


def timed(name, stepper, images, batches, sched=None):
    torch.cuda.synchronize()
    host = 0.0
    t0 = time.perf_counter()
    for tg in batches:
        h0 = time.perf_counter()
        out = stepper(images, tg)
        if sched is not None:
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
    ap.add_argument("--opt-iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    tuning.use_shipped_miopen_db(0)
    tuning.enable_conv_autotune()
    net = r50(dev, True)
    n_params = sum(p.numel() for p in net.parameters())
    n_tensors = sum(1 for _ in net.parameters())

    # (a) the optimizer step alone
    alone = {}
    for name, make, nb in (("sgd", lambda ps: MasterSGD(ps, lr=1e-3, momentum=0.9, weight_decay=1e-4), 20),
                           ("adamw", lambda ps: MasterAdamW(ps, lr=1e-4, weight_decay=1e-2), 28)):
        us, nbytes = optimizer_alone(net, make, nb, args.opt_iters)
        alone[name] = {"us_per_step": round(us, 2), "bytes_per_step": nbytes,
                       "tb_per_s": round(nbytes / us / 1e6, 3), "fraction_of_copy_ceiling": round(nbytes / us / 1e6 / CEILING_TBS, 3)}

    # (b), (c) the train step
    g = torch.Generator().manual_seed(0)
    images = [torch.rand(3, H, W, generator=g).to(dev) for _ in range(B)]
    rng = np.random.default_rng(7)
    tg = []
    for _ in range(B):
        b, l = synth.gt_boxes(rng, 8, H, W)
        tg.append({"boxes": torch.from_numpy(b).to(dev), "labels": torch.from_numpy(l).to(dev)})
    n = args.warmup + args.steps
    batches = [tg] * n
    sgd = MasterSGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    adamw = MasterAdamW(net.parameters(), lr=1e-5, weight_decay=1e-2)
    adamw_s = MasterAdamW(net.parameters(), lr=1e-5, weight_decay=1e-2)
    warm = 1000
    sched = torch.optim.lr_scheduler.LambdaLR(adamw_s, lambda s: min(1.0, (s + 1) / warm))
    net32 = r50(dev, False)
    torch_adamw = torch.optim.AdamW(net32.parameters(), lr=1e-5, weight_decay=1e-2)
    phases = {"sgd": (CapturedTrainStep(net, sgd, amp_dtype=torch.bfloat16, eager_steps=2), None, net),
              "adamw": (CapturedTrainStep(net, adamw, amp_dtype=torch.bfloat16, eager_steps=2), None, net),
              "adamw_lambdalr": (CapturedTrainStep(net, adamw_s, amp_dtype=torch.bfloat16, eager_steps=2), sched, net),
              "torch_adamw_fp32": (CapturedTrainStep(net32, torch_adamw, amp_dtype=torch.bfloat16, eager_steps=2), None, net32)}
    res = {k: [] for k in phases}
    for r in range(args.rounds):
        for k, (st, sc, _) in phases.items():
            for b in batches[:args.warmup]:
                st(images, b)
                if sc is not None:
                    sc.step()
            res[k].append(timed(k, st, images, batches[args.warmup:], sc))
    ms = {k: float(np.mean([v[0] for v in res[k]])) for k in res}
    host = {k: float(np.mean([v[1] for v in res[k]])) for k in res}
    line = {"tool": "adam_step", "workload": f"R50-FPN bf16 train step, B={B} at 3x{H}x{W}, T=8; optimizer alone on its "
                                             f"{n_tensors} parameter tensors ({n_params} elements)",
            "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "opt_iters": args.opt_iters,
            "optimizer_alone": alone, "adamw_vs_sgd_alone": round(alone["adamw"]["us_per_step"] / alone["sgd"]["us_per_step"], 3),
            "target_adamw_us": 250, "target_fraction": 0.75,
            "train_ms_per_step": {k: round(v, 3) for k, v in ms.items()},
            "host_ms_per_step": {k: round(v, 3) for k, v in host.items()},
            "per_round_ms": {k: [round(v[0], 3) for v in res[k]] for k in res},
            "captures": {k: phases[k][0].captures for k in phases}, "replays": {k: phases[k][0].replays for k in phases},
            "lambdalr_final_lr": adamw_s.param_groups[0]["lr"],
            "images_per_s": {k: round(B / ms[k] * 1e3, 1) for k in ms}}
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
