#!/usr/bin/env python3
"""What Quality Focal Loss costs next to K3's focal loss: the loss call alone, and the replayed train step.

(1) The loss call alone at the train shape -- B = 8 images of 3 x 800 x 1333 (padded 800 x 1344: A = 201 600 anchors on five
    levels), K = 90, bf16 head outputs, T = 8 and T = 500 boxes per image, K2's flagged-only buffers -- as the loss Function issues
    it: ``ops.loss_fwd_bwd_levels`` (K3) with the focal parameters alone against K3 with ``alpha = 1, gamma = beta`` followed by
    ``ops.quality_focal_loss`` (two more launches), each captured once in a hipGraph and timed as ``--iters`` replays between two
    events, with the device drained at both ends; the median of ``--rounds`` interleaved rounds and their spread.
(2) R50-FPN, bf16 autocast, B = 8, T = 8, optim.MasterSGD -- bench.py's headline step -- through graph.CapturedTrainStep with
    ``cls_loss="focal"`` and with ``cls_loss="qfl"`` on ONE model and the same batches, as interleaved pairs for ``--rounds``
    rounds (each kind keeps its own CapturedTrainStep); ms/step is wall time over ``--steps`` steps with the device drained at both
    ends.  The pair-to-pair spread of each side stands next to the difference.  ``--no-step`` skips this part.
Prints one JSON line (and writes it to ``--out`` when given).

usage: qfl_step.py [--steps 20] [--warmup 4] [--rounds 3] [--iters 50] [--beta 2.0] [--no-step] [--out FILE]"""
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
from pytorch_retinanet_amd import losses, ops, tuning               # noqa: E402
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
        fn()                                                        # (fills the caches a capture must not allocate: state words, offsets)
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


def loss_alone(dev, rounds, iters, beta):
    levels = synth.levels_for(HP, WP)
    anc = ops.anchors_emit(levels, list(AnchorGenerator().to(dev).cell_anchors), 0.0)
    sizes = [h * w * 9 for h, w, _ in levels]
    gen = torch.Generator(device=dev).manual_seed(0)
    cls = [(torch.randn((B, s, K), device=dev, generator=gen) - 4.6).to(torch.bfloat16) for s in sizes]
    box = [(torch.randn((B, s, 4), device=dev, generator=gen) * 0.1).to(torch.bfloat16) for s in sizes]
    params = losses.RetinaNetLosses(K)._params()
    qparams = losses.RetinaNetLosses(K, cls_loss="qfl", qfl_beta=beta)._params()
    out = {"A": int(anc.shape[0]), "K": K, "dtype": "bf16", "beta": beta}
    for t in (8, 500):
        boxes, labels = _gt(np.random.default_rng(t), t, dev)
        gt, lab = torch.cat(boxes), torch.cat(labels)
        off = ops.gt_offsets([t] * B, dev)
        matches, num_fg, special = ops.iou_match(anc, gt, off, B, IOU_THRESHOLDS_FOREGROUND, IOU_THRESHOLDS_BACKGROUND, want_special=True,
                                                 flagged_only=True)
        form = losses.k3_form(int(gt.shape[0]), B)

        def k3(p=params):
            return ops.loss_fwd_bwd_levels(cls, box, anc, gt, lab, off, matches, num_fg, p, True, special=special,
                                           in_kernel_finalize=losses.IN_KERNEL_FINALIZE, form=form)

        def k3_qfl():
            loss, gcls, _ = k3(qparams)
            ops.quality_focal_loss(cls, box, anc, gt, lab, off, matches, num_fg, special, loss, gcls, beta=beta,
                                   reg_w=tuple(qparams.reg_w), logit_shift=qparams.logit_shift)
        res = {"focal": [], "qfl": []}
        for _ in range(rounds):
            res["focal"].append(_replay_us(k3, iters))
            res["qfl"].append(_replay_us(k3_qfl, iters))
        med = {k: float(np.median(v)) for k, v in res.items()}
        out[f"T{t}"] = {"focal_us": round(med["focal"], 2), "qfl_us": round(med["qfl"], 2),
                        "added_us": round(med["qfl"] - med["focal"], 2),
                        "spread_us": {k: round(float(max(v) - min(v)), 2) for k, v in res.items()},
                        "per_round_us": {k: [round(v, 2) for v in vs] for k, vs in res.items()},
                        "matched_rows": int(num_fg.sum())}
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
    net = P.Retinanet(num_classes=K, backbone_kind="resnet50", pretrained=False, min_size=800, max_size=1333)
    net = net.to(dev).to(memory_format=torch.channels_last).train()
    use_16bit_conv_weights(net, torch.bfloat16)
    opt = MasterSGD(net.parameters(), lr=1e-3, weight_decay=1e-3, momentum=0.9)
    g = torch.Generator().manual_seed(0)
    images = [torch.rand(3, H, W, generator=g).to(dev) for _ in range(B)]
    boxes, labels = _gt(np.random.default_rng(7), T, dev)
    targets = [{"boxes": b, "labels": l} for b, l in zip(boxes, labels)]
    crit = net.retinanet_head.losses
    kinds = ("focal", "qfl")
    crit.qfl_beta = float(args.beta)
    steppers = {k: CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=2) for k in kinds}
    res = {k: [] for k in kinds}
    for _ in range(args.rounds):
        for k, st in steppers.items():
            crit.cls_loss = k
            for _ in range(args.warmup):
                st(images, targets)
            res[k].append(timed(st, images, targets, args.steps))
    crit.cls_loss = "focal"
    ms = {k: float(np.median(v)) for k, v in res.items()}
    return {"workload": f"R50-FPN bf16 train step, B={B} at 3x{H}x{W}, T={T}, MasterSGD", "steps": args.steps, "warmup": args.warmup,
            "replayed_ms_per_step": {k: round(v, 3) for k, v in ms.items()},
            "added_ms": round(ms["qfl"] - ms["focal"], 3), "ratio": round(ms["qfl"] / ms["focal"], 4),
            "spread_ms": {k: round(float(max(v) - min(v)), 3) for k, v in res.items()},
            "per_round_ms": {k: [round(v, 3) for v in res[k]] for k in res},
            "replays": {k: st.replays for k, st in steppers.items()}, "captures": {k: st.captures for k, st in steppers.items()}}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--beta", type=float, default=2.0)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    line = {"tool": "qfl_step", "rounds": args.rounds, "iters": args.iters, "loss_alone": loss_alone(dev, args.rounds, args.iters, args.beta)}
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
