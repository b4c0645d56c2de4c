#!/usr/bin/env python3
"""The train step with and without brightness / contrast drawn and applied on the device (augment.RandomBrightnessContrast).

R50-FPN, bf16 autocast, B = 8 at 3 x 800 x 1333, T = 8 boxes per image, optim.MasterSGD -- bench.py's headline step -- three ways on one
model and the same batches, all replayed through graph.CapturedTrainStep:
  (a) nothing installed: this commit's step with the feature off, which launches what the parent commit's step launches;
  (b) net.transform.brightness_contrast = RandomBrightnessContrast(p=0.5): by-max -- one single-wave draw and, in the transform kernel,
      the COLOR instantiation with one multiply, one add and a clamp per channel value; no further pass over the images;
  (c) the same with brightness_by_max=False: by-mean -- one more read of the source images for the mean (two launches).
The three run interleaved for ``--rounds`` rounds (each keeps its own CapturedTrainStep); ms/step is wall time over ``--steps`` steps
with the device drained at both ends.  The yardstick is leg (a) of the same run.  Prints one JSON line (and writes it to ``--out``
when given).

usage: brightness_contrast_step.py [--steps 20] [--warmup 4] [--rounds 3] [--out FILE]"""
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
from pytorch_retinanet_amd.augment import RandomBrightnessContrast  # noqa: E402
from pytorch_retinanet_amd.graph import CapturedTrainStep           # noqa: E402
from pytorch_retinanet_amd.optim import MasterSGD, use_16bit_conv_weights   # noqa: E402

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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
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
    installed = {"a": None, "b": RandomBrightnessContrast(p=0.5, seed=0), "c": RandomBrightnessContrast(brightness_by_max=False, p=0.5, seed=0)}
    steppers = {k: CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=2) for k in installed}
    res = {k: [] for k in steppers}
    for r in range(args.rounds):
        for k, st in steppers.items():
            net.transform.brightness_contrast = installed[k]
            for _ in range(args.warmup):
                st(images, targets)
            res[k].append(timed(st, images, targets, args.steps))
    net.transform.brightness_contrast = None
    ms = {k: float(np.median(v)) for k, v in res.items()}
    line = {"tool": "brightness_contrast_step", "workload": f"R50-FPN bf16 train step, B={B} at 3x{H}x{W}, T={T}, MasterSGD",
            "by_max": repr(installed["b"]), "by_mean": repr(installed["c"]), "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
            "a_off_replayed_ms_per_step": round(ms["a"], 3), "b_by_max_replayed_ms_per_step": round(ms["b"], 3),
            "c_by_mean_replayed_ms_per_step": round(ms["c"], 3),
            "b_minus_a_ms": round(ms["b"] - ms["a"], 3), "c_minus_a_ms": round(ms["c"] - ms["a"], 3),
            "b_vs_a": round(ms["b"] / ms["a"], 4), "c_vs_a": round(ms["c"] / ms["a"], 4),
            "per_round_ms": {k: [round(v, 3) for v in res[k]] for k in res},
            "replays": {k: st.replays for k, st in steppers.items()}, "captures": {k: st.captures for k, st in steppers.items()},
            "batches_drawn": {k: installed[k].counter for k in ("b", "c")}}
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
