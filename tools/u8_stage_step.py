#!/usr/bin/env python3
"""Staging uint8 images (rn_image_stage_u8) against staging fp32 images (rn_image_stage), B = 8 at 3 x 800 x 1333.

Three measurements on one box in one run, each as interleaved pairs for ``--rounds`` rounds after a warm-up (medians are reported, the
per-round values are kept):
  1. the staging launch alone, device events around ``--reps`` launches back to back: ``image_stage_u8`` on interleaved sources, on
     planar sources, and ``image_stage`` on the CPU-converted floats (the yardstick: this kernel is not touched).  Bytes moved per
     launch are computed from the shapes -- uint8: 3 read + 12 written per pixel, fp32: 12 + 12 -- and GB/s = bytes / time, next to the
     6.29 TB/s copy ceiling the project uses.  No cache flush between launches: a hot-cache figure, like ``image_stage_ms`` elsewhere.
  2. a batch from pinned host memory into the arena: the host-to-device copies plus the staging launch, host clock around ``--reps``
     batches with the device drained at both ends, uint8 (interleaved) against fp32.
  3. the replayed R50-FPN bf16 train step (optim.MasterSGD, gt_capacity + image_capacity "auto") fed the uint8 batch against fed the
     fp32 batch from device memory: ms/step is wall time over ``--steps`` steps with the device drained at both ends.  Both feed ONE
     graph (the key's dtype is the arena's); ``--no-step`` skips this part.
Before anything is timed the two arenas are compared bit for bit.  Prints one JSON line (and writes it to ``--out``).

usage: u8_stage_step.py [--steps 20] [--warmup 4] [--rounds 3] [--reps 50] [--no-step] [--out FILE]"""
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

B, H, W, T = 8, 800, 1333, 8
COPY_CEILING_GBPS = 6290.0


def launch_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def wall_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def timed(stepper, images, targets, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = stepper(images, targets)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    assert np.isfinite(float(out["loss"])), "non-finite loss"
    return wall / steps * 1e3


def interleaved(fns, rounds, warmup, measure):
    "-> {name: [one value per round]}: every round runs each candidate once, in turn, after its own warm-up."
    res = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            for _ in range(warmup):
                fn()
            res[k].append(measure(fn))
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "u8_stage_step.py measures on the GPU: no device, no number"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    hwc = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(B)]
    host_u8 = [torch.from_numpy(a).pin_memory() for a in hwc]                                   # [H, W, 3], as a decoder gives it
    host_f32 = [(t.permute(2, 0, 1).to(torch.float32) / 255).contiguous().pin_memory() for t in host_u8]
    u8_i = [t.to(dev).permute(2, 0, 1) for t in host_u8]                                       # interleaved: strides (1, 3 W, 3)
    u8_p = [t.contiguous() for t in u8_i]                                                      # planes
    f32 = [t.to(dev) for t in host_f32]
    pix = image_pixel_class([(H, W)] * B)
    arena = {k: ops.new_image_arena(B, pix, dev) for k in ("u8_interleaved", "u8_planar", "f32")}
    ops.image_stage_u8(u8_i, arena["u8_interleaved"]); ops.image_stage_u8(u8_p, arena["u8_planar"]); ops.image_stage(f32, arena["f32"])
    torch.cuda.synchronize()
    n = 3 * H * W
    same = all(torch.equal(arena[k].arena[:, :n].view(torch.int32), arena["f32"].arena[:, :n].view(torch.int32)) for k in arena)
    assert same, "the uint8 stage and the fp32 stage of the converted floats differ"

    # ---- 1. the launch alone ----
    fns = {"u8_interleaved": lambda: ops.image_stage_u8(u8_i, arena["u8_interleaved"]),
           "u8_planar": lambda: ops.image_stage_u8(u8_p, arena["u8_planar"]), "f32": lambda: ops.image_stage(f32, arena["f32"])}
    k_ms = interleaved(fns, args.rounds, args.warmup, lambda fn: launch_ms(fn, args.reps))
    moved = {"u8_interleaved": B * H * W * 15, "u8_planar": B * H * W * 15, "f32": B * H * W * 24}
    kernel = {}
    for k, v in k_ms.items():
        ms = float(np.median(v))
        gbps = moved[k] / ms / 1e6
        kernel[k] = {"ms": round(ms, 4), "per_round_ms": [round(x, 4) for x in v], "bytes": moved[k], "GBps": round(gbps, 1),
                     "share_of_copy_ceiling": round(gbps / COPY_CEILING_GBPS, 4)}

    # ---- 2. pinned host memory -> arena ----
    def feed_u8():
        ops.image_stage_u8([t.to(dev, non_blocking=True).permute(2, 0, 1) for t in host_u8], arena["u8_interleaved"])

    def feed_f32():
        ops.image_stage([t.to(dev, non_blocking=True) for t in host_f32], arena["f32"])
    h_ms = interleaved({"u8": feed_u8, "f32": feed_f32}, args.rounds, 2, lambda fn: wall_ms(fn, max(args.reps // 5, 4)))
    h2d = {k: {"ms": round(float(np.median(v)), 3), "per_round_ms": [round(x, 3) for x in v],
               "host_bytes": B * H * W * (3 if k == "u8" else 12)} for k, v in h_ms.items()}

    line = {"tool": "u8_stage_step", "workload": f"B={B} at 3x{H}x{W}", "reps": args.reps, "rounds": args.rounds, "warmup": args.warmup,
            "bits_equal": same, "copy_ceiling_GBps": COPY_CEILING_GBPS, "stage_launch": kernel,
            "u8_interleaved_vs_f32": round(kernel["u8_interleaved"]["ms"] / kernel["f32"]["ms"], 4),
            "u8_planar_vs_f32": round(kernel["u8_planar"]["ms"] / kernel["f32"]["ms"], 4), "pinned_h2d_plus_stage": h2d,
            "h2d_u8_vs_f32": round(h2d["u8"]["ms"] / h2d["f32"]["ms"], 4)}

    # ---- 3. the replayed train step ----
    if not args.no_step:
        tuning.use_shipped_miopen_db(0)
        tuning.enable_conv_autotune()
        torch.manual_seed(0)
        net = P.Retinanet(num_classes=90, backbone_kind="resnet50", pretrained=False, min_size=800, max_size=1333)
        net = net.to(dev).to(memory_format=torch.channels_last).train()
        use_16bit_conv_weights(net, torch.bfloat16)
        opt = MasterSGD(net.parameters(), lr=1e-3, weight_decay=1e-3, momentum=0.9)
        targets = []
        for _ in range(B):
            b, l = synth.gt_boxes(rng, T, H, W)
            targets.append({"boxes": torch.from_numpy(b).to(dev), "labels": torch.from_numpy(l).to(dev)})
        st = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=2, gt_capacity="auto", image_capacity="auto")
        feeds = {"u8": u8_i, "f32": f32}
        res = {k: [] for k in feeds}
        for _ in range(args.rounds):
            for k, ims in feeds.items():
                for _ in range(args.warmup):
                    st(ims, targets)
                res[k].append(timed(st, ims, targets, args.steps))
        ms = {k: float(np.median(v)) for k, v in res.items()}
        line["train_step"] = {"workload": f"R50-FPN bf16 train step, B={B} at 3x{H}x{W}, T={T}, MasterSGD, gt_capacity + image_capacity auto",
                              "steps": args.steps, "u8_ms_per_step": round(ms["u8"], 3), "f32_ms_per_step": round(ms["f32"], 3),
                              "u8_vs_f32": round(ms["u8"] / ms["f32"], 4), "per_round_ms": {k: [round(v, 3) for v in res[k]] for k in res},
                              "captures": st.captures, "replays": st.replays, "keys": len(st._entries)}
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
