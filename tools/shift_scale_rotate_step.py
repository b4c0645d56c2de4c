#!/usr/bin/env python3
"""The train step with and without shift / scale / rotate drawn and applied on the device (augment.ShiftScaleRotate).

R50-FPN, bf16 autocast, B = 8 at 3 x 800 x 1333, T = 8 boxes per image, optim.MasterSGD, gt_capacity="auto" + image_capacity="auto"
(the staged path) -- two ways on one model and the same batches, both replayed through graph.CapturedTrainStep on the same canvas
class (800 x 1344):
  (a) nothing installed: this commit's staged step with the augmentation off, which launches what the parent commit's staged step
      launches;
  (b) net.transform.shift_scale_rotate = ShiftScaleRotate(p=1.0): the draw (two launches of one wave per image + the counter's
      launch) and the warp of every image into a second arena (four 4-byte taps per channel and pixel, one dense store), all inside
      the graph.
The two run as interleaved pairs for ``--rounds`` rounds (each keeps its own CapturedTrainStep); ms/step is wall time over ``--steps``
steps with the device drained at both ends.  ``warp_stage_ms`` times the warp launch alone with device events, ``--reps`` launches back
to back over the staged batch with its last coefficients and no cache flush between them (a hot-cache figure); ``warp_stage_GBps`` =
the bytes of the images read once and written once over that time (the taps' re-reads are served by the caches and not counted).  For
the kernel's time inside a step run the tool under ``rocprofv3 --kernel-trace --stats`` in a run of its own and read
``image_warp_stage_kernel``.  Prints one JSON line (and writes it to ``--out``).

usage: shift_scale_rotate_step.py [--steps 20] [--warmup 4] [--rounds 3] [--reps 20] [--out FILE]"""
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
from pytorch_retinanet_amd.augment import ShiftScaleRotate          # noqa: E402
from pytorch_retinanet_amd.graph import CapturedTrainStep, image_pixel_class    # noqa: E402
from pytorch_retinanet_amd.optim import MasterSGD, use_16bit_conv_weights       # noqa: E402

B, H, W, T = 8, 800, 1333, 8


def timed(stepper, images, targets, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = stepper(images, targets)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    assert np.isfinite(float(out["loss"])), "non-finite loss"
    return wall / steps * 1e3


def warp_stage_ms(images, coef, dev, reps):
    "-> (ms per warp launch, bytes of the images read once + written once) for the staged batch and ``coef`` (rn_affine_coef on the device)."
    staged = ops.image_stage(images, ops.new_image_arena(len(images), image_pixel_class([im.shape[1:] for im in images]), dev))
    out = ops.StagedImages(torch.empty_like(staged.arena), torch.empty_like(staged.in_hw))
    for _ in range(3):
        ops.image_warp_stage(staged, coef, out=out)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        ops.image_warp_stage(staged, coef, out=out)
    e1.record()
    torch.cuda.synchronize()
    moved = sum(2 * 4 * 3 * int(im.shape[1]) * int(im.shape[2]) for im in images)
    return e0.elapsed_time(e1) / reps, moved


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
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
    targets = []
    for _ in range(B):
        b, l = synth.gt_boxes(rng, T, H, W)
        targets.append({"boxes": torch.from_numpy(b).to(dev), "labels": torch.from_numpy(l).to(dev)})
    ssr = ShiftScaleRotate(p=1.0, seed=0)
    kw = dict(amp_dtype=torch.bfloat16, eager_steps=2, gt_capacity="auto", image_capacity="auto")
    steppers = {"a": CapturedTrainStep(net, opt, **kw), "b": CapturedTrainStep(net, opt, **kw)}
    res = {k: [] for k in steppers}
    for r in range(args.rounds):
        for k, st in steppers.items():
            net.transform.shift_scale_rotate = ssr if k == "b" else None
            for _ in range(args.warmup):
                st(images, targets)
            res[k].append(timed(st, images, targets, args.steps))
    net.transform.shift_scale_rotate = None
    ms = {k: float(np.median(v)) for k, v in res.items()}
    coef = ssr.coef.clone()
    m, _, applied, kept = ops.affine_coef_views(coef)
    warp_ms, moved = warp_stage_ms(images, coef, dev, args.reps)
    classes = sorted({(str(k[0][2]), k[0][3]) for st in steppers.values() for k in st._entries if k[0][0] == "img_cap"})
    line = {"tool": "shift_scale_rotate_step",
            "workload": f"R50-FPN bf16 train step, B={B} at 3x{H}x{W}, T={T}, MasterSGD, gt_capacity + image_capacity auto",
            "shift_scale_rotate": repr(ssr), "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
            "a_off_replayed_ms_per_step": round(ms["a"], 3), "b_on_replayed_ms_per_step": round(ms["b"], 3),
            "b_minus_a_ms": round(ms["b"] - ms["a"], 3), "b_vs_a": round(ms["b"] / ms["a"], 4),
            "per_round_ms": {k: [round(v, 3) for v in res[k]] for k in res},
            "replays": {k: st.replays for k, st in steppers.items()}, "captures": {k: st.captures for k, st in steppers.items()},
            "classes_hit": classes, "b_batches_drawn": ssr.counter, "last_applied": applied.tolist(), "last_kept": kept.tolist(),
            "last_m": [[round(float(v), 5) for v in row] for row in m.tolist()],
            "warp_stage_ms": round(warp_ms, 4), "warp_stage_bytes": moved, "warp_stage_GBps": round(moved / warp_ms / 1e6, 1),
            "warp_stage_reps": args.reps}
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
