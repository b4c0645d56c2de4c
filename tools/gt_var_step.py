#!/usr/bin/env python3
"""The train step on batches whose GT counts change from step to step (graph.CapturedTrainStep's GT capacity mode).

R50-FPN, bf16 autocast, B = 8 at 3 x 800 x 1333, optim.MasterSGD -- bench.py's headline step -- timed three ways:
  (a) constant T = 8 boxes per image, exact-shape keying: one capture, then replays (bench.py's line);
  (b) T ~ U{1..16} per image per step (seed-fixed), gt_capacity="auto": one capture per capacity class hit, then replays;
  (c) the same batches with the capacity mode off: every batch is a new signature -> eager steps (real training before this mode).
The phases run interleaved for ``--rounds`` rounds on one model (each keeps its own CapturedTrainStep); ms/step is wall time over
``--steps`` steps with the device drained at both ends, host ms/step the time the calls take to return (no sync inside).
Prints one JSON line (and writes it to ``--out`` when given).

usage: gt_var_step.py [--steps 20] [--warmup 4] [--rounds 2] [--out FILE]"""
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
from pytorch_retinanet_amd.graph import GT_CAPACITY_CLASSES, CapturedTrainStep, gt_capacity_class   # noqa: E402
from pytorch_retinanet_amd.optim import MasterSGD, use_16bit_conv_weights                        # noqa: E402

B, H, W = 8, 800, 1333


def gt_batches(rng, n, counts_fn, dev):
    out = []
    for _ in range(n):
        tg = []
        for c in counts_fn():
            b, l = synth.gt_boxes(rng, int(c), H, W)
            tg.append({"boxes": torch.from_numpy(b).to(dev), "labels": torch.from_numpy(l).to(dev)})
        out.append(tg)
    return out


def timed(stepper, images, batches):
    torch.cuda.synchronize()
    host = 0.0
    t0 = time.perf_counter()
    for tg in batches:
        h0 = time.perf_counter()
        out = stepper(images, tg)
        host += time.perf_counter() - h0
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    assert np.isfinite(float(out["loss"])), "non-finite loss"
    return wall / len(batches) * 1e3, host / len(batches) * 1e3


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    tuning.use_shipped_miopen_db(0)
    tuning.enable_conv_autotune()
    torch.manual_seed(0)
    net = P.Retinanet(num_classes=90, backbone_kind="resnet50", pretrained=False, min_size=800, max_size=1333)
    net = net.to(dev).to(memory_format=torch.channels_last).train()
    use_16bit_conv_weights(net, torch.bfloat16)
    opt = MasterSGD(net.parameters(), lr=1e-3, weight_decay=1e-3, momentum=0.9)
    g = torch.Generator().manual_seed(0)
    images = [torch.rand(3, H, W, generator=g).to(dev) for _ in range(B)]
    rng = np.random.default_rng(7)
    n = args.warmup + args.steps
    const = gt_batches(rng, 1, lambda: [8] * B, dev) * n
    var_counts = []

    def var():
        c = rng.integers(1, 17, size=B)
        var_counts.append(c)
        return c
    var_all = gt_batches(rng, n * args.rounds, var, dev)
    classes = sorted({gt_capacity_class(c, GT_CAPACITY_CLASSES) for c in var_counts})
    steppers = {"a": CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=2),
                "b": CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=2, gt_capacity="auto"),
                "c": CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=2)}
    res = {k: [] for k in steppers}
    for r in range(args.rounds):
        for k, st in steppers.items():
            data = const if k == "a" else var_all[r * n:(r + 1) * n]
            for tg in data[:args.warmup]:
                st(images, tg)
            res[k].append(timed(st, images, data[args.warmup:]))
    ms = {k: float(np.mean([v[0] for v in res[k]])) for k in res}
    host = {k: float(np.mean([v[1] for v in res[k]])) for k in res}
    line = {"tool": "gt_var_step", "workload": f"R50-FPN bf16 train step, B={B} at 3x{H}x{W}, T~U{{1..16}} per image (b, c) / T=8 (a)",
            "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
            "a_const_T8_replay_ms_per_step": round(ms["a"], 3), "b_var_T_capacity_ms_per_step": round(ms["b"], 3),
            "c_var_T_eager_ms_per_step": round(ms["c"], 3),
            "b_vs_a": round(ms["b"] / ms["a"], 4), "b_vs_c": round(ms["b"] / ms["c"], 4),
            "host_ms_per_step": {k: round(v, 3) for k, v in host.items()},
            "per_round_ms": {k: [round(v[0], 3) for v in res[k]] for k in res},
            "b_replays": steppers["b"].replays, "b_captures": steppers["b"].captures, "classes_hit": classes,
            "a_replays": steppers["a"].replays, "c_replays": steppers["c"].replays,
            "images_per_s": {k: round(B / ms[k] * 1e3, 1) for k in ms}}
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
