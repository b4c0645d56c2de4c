#!/usr/bin/env python3
"""The train step on batches whose IMAGE SIZES change from step to step (graph.CapturedTrainStep's image capacity mode).

R50-FPN, bf16 autocast, B = 8, min_size 800 / max_size 1333, optim.MasterSGD; every image's raw size is drawn per step from a seed-fixed
list of COCO-like landscape shapes that share one pixel class (2**19) and one canvas class (800 x 1344), T ~ U{1..16} boxes per image.
Timed three ways:
  (a) the varying batches, gt_capacity="auto" + image_capacity="auto": one capture per (canvas, pixel, GT) class hit, then replays;
  (b) the same batches with the image mode off (gt_capacity="auto" alone): nearly every batch is a new signature -> eager steps;
  (c) a constant-size batch (8 x 3 x 480 x 800 -> 799 x 1333: its own canvas IS the class canvas), gt_capacity="auto": replays -- the
      yardstick (a) is held against.
The phases run interleaved for ``--rounds`` rounds on one model (each keeps its own CapturedTrainStep); ms/step is wall time over
``--steps`` steps with the device drained at both ends, host ms/step the time the calls take to return (no sync inside).  The staging
launch (``ops.image_stage`` of one batch) is timed on its own with device events.  Prints one JSON line (and writes it to ``--out``).

How to read the numbers: the three phases train the SAME net and optimizer one after the other, so the weights and MIOpen's autotune state
carry over from phase to phase and round to round -- the phases compare step TIME, not training results.  ``image_stage_ms`` is 50 launches
back to back over one batch with no cache flush between them: an upper bound on a hot-cache copy (source and arena stay in the Infinity
Cache), not the launch's cost inside a step, where the images come from HBM.

usage: image_var_step.py [--steps 20] [--warmup 4] [--rounds 2] [--out FILE]"""
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
from pytorch_retinanet_amd.graph import CapturedTrainStep, image_pixel_class    # noqa: E402
from pytorch_retinanet_amd.optim import MasterSGD, use_16bit_conv_weights       # noqa: E402

B = 8
# COCO-like landscape shapes, all within the pixel class 2**19 (262144 < h * w <= 524288 for the largest) and the canvas 800 x 1344
SHAPES = [(480, 640), (427, 640), (426, 640), (428, 640), (640, 640), (500, 640), (375, 500), (333, 500), (480, 600), (512, 640),
          (424, 640), (360, 640), (457, 640), (640, 800), (600, 800), (534, 800)]

CONST_SHAPE = (480, 800)            # resizes to 799 x 1333: the natural canvas is 800 x 1344, pixel class 2**19


def batches(rng, n, shapes_fn, dev):
    out = []
    for _ in range(n):
        ims, tg = [], []
        for h, w in shapes_fn():
            ims.append(torch.from_numpy(rng.random((3, h, w), dtype=np.float32)).to(dev))
            b, l = synth.gt_boxes(rng, int(rng.integers(1, 17)), h, w)
            tg.append({"boxes": torch.from_numpy(b).to(dev), "labels": torch.from_numpy(l).to(dev)})
        out.append((ims, tg))
    return out


def timed(stepper, data):
    torch.cuda.synchronize()
    host = 0.0
    t0 = time.perf_counter()
    for ims, tg in data:
        h0 = time.perf_counter()
        out = stepper(ims, tg)
        host += time.perf_counter() - h0
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    assert np.isfinite(float(out["loss"])), "non-finite loss"
    return wall / len(data) * 1e3, host / len(data) * 1e3


def stage_ms(ims, dev, reps=50):
    staged = ops.new_image_arena(len(ims), image_pixel_class([im.shape[1:] for im in ims]), dev)
    for _ in range(5):
        ops.image_stage(ims, staged)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        ops.image_stage(ims, staged)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


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
    rng = np.random.default_rng(7)
    n = args.warmup + args.steps
    assert image_pixel_class(SHAPES) == 2 ** 19
    # every batch holds the largest shape's pixel class: one image of >= 2**18 pixels keeps the batch in class 2**19
    big = [s for s in SHAPES if s[0] * s[1] > 2 ** 18]

    def var_shapes():
        pick = [SHAPES[int(i)] for i in rng.integers(0, len(SHAPES), size=B - 1)]
        return [big[int(rng.integers(0, len(big)))]] + pick
    var_all = batches(rng, n * args.rounds, var_shapes, dev)
    const_all = batches(rng, n * args.rounds, lambda: [CONST_SHAPE] * B, dev)
    const_ims = const_all[0][0]
    const_all = [(const_ims, tg) for _, tg in const_all]             # the same eight images at every step: the sizes are what matters
    kw = dict(amp_dtype=torch.bfloat16, eager_steps=2, gt_capacity="auto")
    steppers = {"a": CapturedTrainStep(net, opt, image_capacity="auto", max_graphs=8, **kw), "b": CapturedTrainStep(net, opt, **kw),
                "c": CapturedTrainStep(net, opt, **kw)}
    res = {k: [] for k in steppers}
    for r in range(args.rounds):
        for k, st in steppers.items():
            data = (const_all if k == "c" else var_all)[r * n:(r + 1) * n]
            for ims, tg in data[:args.warmup]:
                st(ims, tg)
            res[k].append(timed(st, data[args.warmup:]))
    ms = {k: float(np.mean([v[0] for v in res[k]])) for k in res}
    host = {k: float(np.mean([v[1] for v in res[k]])) for k in res}
    keys = sorted({(k[0][2], k[0][3], k[1][1]) for k in steppers["a"]._entries if k[0][0] == "img_cap"})
    line = {"tool": "image_var_step",
            "workload": f"R50-FPN bf16 train step, B={B}, raw sizes from {len(SHAPES)} COCO-like shapes per image and step, T~U{{1..16}}, min 800 / max 1333",
            "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
            "a_var_size_image_capacity_ms_per_step": round(ms["a"], 3), "b_var_size_mode_off_ms_per_step": round(ms["b"], 3),
            "c_const_size_same_canvas_replay_ms_per_step": round(ms["c"], 3),
            "a_vs_c": round(ms["a"] / ms["c"], 4), "a_vs_b": round(ms["a"] / ms["b"], 4),
            "host_ms_per_step": {k: round(v, 3) for k, v in host.items()},
            "per_round_ms": {k: [round(v[0], 3) for v in res[k]] for k in res},
            "a_replays": steppers["a"].replays, "a_captures": steppers["a"].captures, "a_classes_hit": [list(map(str, k)) for k in keys],
            "b_replays": steppers["b"].replays, "b_captures": steppers["b"].captures,
            "c_replays": steppers["c"].replays, "c_captures": steppers["c"].captures,
            "image_stage_ms": round(stage_ms(var_all[0][0], dev), 4),
            "images_per_s": {k: round(B / ms[k] * 1e3, 1) for k in ms}}
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
