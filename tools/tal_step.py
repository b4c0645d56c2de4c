#!/usr/bin/env python3
"""What the task-aligned matcher costs next to K2 and ATSS: the matcher call alone, and the replayed train step.

(1) The matcher call alone at the train shape -- B = 8 images of 3 x 800 x 1333 (padded 800 x 1344: A = 201 600 anchors on five
    levels), K = 90, bf16 head outputs (logits around the prior, deltas of 0.1), T = 8 and T = 500 boxes per image -- as the loss issues
    it (flag words, FLAGGED_ONLY): ``ops.iou_match`` (K2), ``ops.atss_match`` and ``ops.tal_match`` (four launches each; TAL with the grid
    widths, as the model calls it, and walking every level whole), each captured once in a hipGraph and timed as ``--iters`` replays between two events, with the
    device drained at both ends; the median of ``--rounds`` interleaved rounds and their spread.
(2) R50-FPN, bf16 autocast, B = 8, T = 8, optim.MasterSGD -- bench.py's headline step -- through graph.CapturedTrainStep with
    ``matcher="iou"`` and with ``matcher="tal"`` on ONE model and the same batches, as interleaved pairs for ``--rounds`` rounds (each
    kind keeps its own CapturedTrainStep); ms/step is wall time over ``--steps`` steps with the device drained at both ends.  The
    pair-to-pair spread of each side stands next to the difference.  ``--no-step`` skips this part.
Prints one JSON line (and writes it to ``--out`` when given).

usage: tal_step.py [--steps 20] [--warmup 4] [--rounds 3] [--iters 50] [--no-step] [--out FILE]"""
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
from pytorch_retinanet_amd import ops, tuning                       # noqa: E402
from pytorch_retinanet_amd.anchors import AnchorGenerator           # noqa: E402
from pytorch_retinanet_amd.config import IOU_THRESHOLDS_BACKGROUND, IOU_THRESHOLDS_FOREGROUND   # noqa: E402
from pytorch_retinanet_amd.graph import CapturedTrainStep           # noqa: E402
from pytorch_retinanet_amd.optim import MasterSGD, use_16bit_conv_weights   # noqa: E402

B, H, W, T, K = 8, 800, 1333, 8, 90
HP, WP = 800, 1344


def _gt(rng, t, dev):
    boxes, labels = [], []
    for _ in range(B):
        b, l = synth.gt_boxes(rng, t, H, W)
        boxes.append(torch.from_numpy(b).to(dev))
        labels.append(torch.from_numpy(l).to(dev))
    return boxes, labels


def _replay_us(fn, iters):
    "``fn`` captured once; microseconds per replay over ``iters`` replays between two events."
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()                                                        # (fills the caches a capture must not allocate: workspace, offsets)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def matcher_alone(dev, rounds, iters):
    levels = synth.levels_for(HP, WP)
    anc = ops.anchors_emit(levels, list(AnchorGenerator().to(dev).cell_anchors), 0.0)
    sizes = [h * w * 9 for h, w, _ in levels]
    widths = [w for _, w, _ in levels]
    out = {"A": int(anc.shape[0]), "level_sizes": sizes, "K": K, "dtype": "bf16"}
    g = torch.Generator(device=dev).manual_seed(1)
    cls = [(torch.randn((B, s, K), device=dev, generator=g) * 0.5 - 4.6).to(torch.bfloat16) for s in sizes]
    box = [(torch.randn((B, s, 4), device=dev, generator=g) * 0.1).to(torch.bfloat16) for s in sizes]
    for t in (8, 500):
        boxes, labels = _gt(np.random.default_rng(t), t, dev)
        gt, lab = torch.cat(boxes), torch.cat(labels).to(torch.int64)
        off = ops.gt_offsets([t] * B, dev)
        bufs = ops.iou_match_outputs(B, int(anc.shape[0]), dev)
        ws = {}

        def k2():
            ops.iou_match(anc, gt, off, B, IOU_THRESHOLDS_FOREGROUND, IOU_THRESHOLDS_BACKGROUND, out=bufs, flagged_only=True)

        def atss():
            with ops.use_atss_workspaces(ws):
                ops.atss_match(anc, gt, off, B, sizes, 9, 9, out=bufs, flagged_only=True)

        def tal(level_w=widths):
            with ops.use_atss_workspaces(ws):
                ops.tal_match(cls, box, anc, gt, lab, off, B, sizes, 9, out=bufs, flagged_only=True, level_w=level_w)

        fns = {"k2": k2, "atss": atss, "tal": tal, "tal_whole_levels": lambda: tal(None)}
        res = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                res[k].append(_replay_us(fn, iters))
        tal()
        torch.cuda.synchronize()
        out[f"T{t}"] = {**{f"{k}_us": round(float(np.median(v)), 2) for k, v in res.items()},
                        **{f"{k}_spread_us": round(float(max(v) - min(v)), 2) for k, v in res.items()},
                        "per_round_us": {k: [round(v, 2) for v in vs] for k, vs in res.items()},
                        "tal_num_fg_per_image": [int(v) for v in bufs[1].tolist()]}
    return out


def timed(stepper, images, targets, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = stepper(images, targets)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    assert np.isfinite(float(out["loss"])), "non-finite loss"
    return wall / steps * 1e3


def step_pairs(dev, args):
    tuning.use_shipped_miopen_db(0)
    tuning.enable_conv_autotune()
    torch.manual_seed(0)
    net = P.Retinanet(num_classes=90, backbone_kind="resnet50", pretrained=False, min_size=800, max_size=1333)
    net = net.to(dev).to(memory_format=torch.channels_last).train()
    use_16bit_conv_weights(net, torch.bfloat16)
    opt = MasterSGD(net.parameters(), lr=1e-3, weight_decay=1e-3, momentum=0.9)
    g = torch.Generator().manual_seed(0)
    images = [torch.rand(3, H, W, generator=g).to(dev) for _ in range(B)]
    boxes, labels = _gt(np.random.default_rng(7), T, dev)
    targets = [{"boxes": b, "labels": l} for b, l in zip(boxes, labels)]
    crit = net.retinanet_head.losses
    steppers = {"iou": CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=2),
                "tal": CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=2)}
    res = {k: [] for k in steppers}
    for _ in range(args.rounds):
        for k, st in steppers.items():
            crit.matcher = k
            for _ in range(args.warmup):
                st(images, targets)
            res[k].append(timed(st, images, targets, args.steps))
    crit.matcher = "iou"
    ms = {k: float(np.median(v)) for k, v in res.items()}
    return {"workload": f"R50-FPN bf16 train step, B={B} at 3x{H}x{W}, T={T}, MasterSGD", "steps": args.steps, "warmup": args.warmup,
            "iou_replayed_ms_per_step": round(ms["iou"], 3), "tal_replayed_ms_per_step": round(ms["tal"], 3),
            "tal_minus_iou_ms": round(ms["tal"] - ms["iou"], 3), "tal_vs_iou": round(ms["tal"] / ms["iou"], 4),
            "spread_ms": {k: round(float(max(v) - min(v)), 3) for k, v in res.items()},
            "per_round_ms": {k: [round(v, 3) for v in res[k]] for k in res},
            "replays": {k: st.replays for k, st in steppers.items()}, "captures": {k: st.captures for k, st in steppers.items()}}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    line = {"tool": "tal_step", "rounds": args.rounds, "iters": args.iters, "matcher_alone": matcher_alone(dev, args.rounds, args.iters)}
    if not args.no_step:
        line["step"] = step_pairs(dev, args)
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
