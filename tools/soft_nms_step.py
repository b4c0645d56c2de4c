#!/usr/bin/env python3
"""What Soft-NMS costs next to hard NMS: the detect chain alone, and a replayed predict.

(1) The detect chain at BASELINE configs[3]'s shape -- B = 16 images, A = 338 454 anchors (1344 x 1344 padded input), K = 90, fp16
    head outputs, logits N(-7, 1.2) (SURVEY 8d's sparse regime, ~11 k candidates per image), bench.py's ``detect_chain_line`` inputs
    -- with ``nms="hard"`` and with each soft kind: each chain's launches captured once in a hipGraph and timed as ``--iters``
    replays between two events, the device drained at both ends; hard against each soft kind as interleaved pairs for ``--rounds``
    rounds, the median of each side and its pair-to-pair spread.  The hard side is the parent commit's launches: it is the yardstick
    of the same run.
(2) ``graph.CapturedPredict`` on R50-FPN, bf16 autocast, eval mode, B = 1 at min_size 800 / max_size 1333 over the class canvas
    800 x 1344 (the smallest R50 shape of tools/predict_var_step.py, calibrated as there to logits ~N(-7, 1.2)) on ONE model whose
    ``nms`` is flipped between the kinds: each kind keeps its own graph under the predictor's key; ms/call is wall time over
    ``--steps`` replayed calls, interleaved.  ``--no-predict`` skips this part.
A soft kind runs one block-wide argmin and one decay pass per survivor where hard NMS builds a suppression matrix once, so it is
expected to cost more on crowded classes; the figure is reported here, not tuned.  Prints one JSON line (and writes it to ``--out``
when given).

usage: soft_nms_step.py [--steps 20] [--warmup 4] [--rounds 3] [--iters 50] [--no-predict] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import synth                                                        # noqa: E402
import pytorch_retinanet_amd as P                                   # noqa: E402
from pytorch_retinanet_amd import ops, tuning                       # noqa: E402
from pytorch_retinanet_amd.anchors import AnchorGenerator           # noqa: E402
from pytorch_retinanet_amd.graph import CapturedPredict             # noqa: E402

KINDS = ops.NMS_KINDS
CANVAS = (800, 1344)
AMP = torch.bfloat16


def _replay_us(enqueue, iters):
    "``enqueue`` captured once; microseconds per replay over ``iters`` replays between two events."
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enqueue()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        enqueue()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def _sides(res, unit, digits):
    med = {k: float(np.median(v)) for k, v in res.items()}
    out = {f"{k}_{unit}": round(v, digits) for k, v in med.items()}
    for k in KINDS[1:]:
        out[f"added_{unit}_{k}"] = round(med[k] - med["hard"], digits)
        out[f"ratio_{k}"] = round(med[k] / med["hard"], 4)
    out[f"spread_{unit}"] = {k: round(float(max(v) - min(v)), digits) for k, v in res.items()}
    out[f"per_round_{unit}"] = {k: [round(x, digits) for x in v] for k, v in res.items()}
    return out


def chain_pairs(dev, rounds, iters):
    B, A, K = 16, 338454, 90
    anc = ops.anchors_emit(synth.levels_for(1344, 1344), list(AnchorGenerator().to(dev).cell_anchors), 0.0)
    g = torch.Generator(device=dev).manual_seed(1)
    cls = (torch.randn((B, A, K), device=dev, generator=g) * 1.2 - 7.0).to(torch.float16)
    box = (torch.randn((B, A, 4), device=dev, generator=g) * 0.1).to(torch.float16)
    hw = [(1333, 1333)] * B
    handles, moved = {}, {}
    for kind in KINDS:
        handles[kind] = []
        ops.detect_levels([cls], [box], anc, hw, 0.05, 1e-2, 0.5, 100, max_candidates=1 << 18, enqueue_only=handles[kind], nms=kind)
    res = {k: [] for k in KINDS}
    for _ in range(rounds):                                           # hard against each soft kind, as pairs
        for kind in KINDS[1:]:
            res["hard"].append(_replay_us(handles["hard"][0], iters))
            res[kind].append(_replay_us(handles[kind][0], iters))
    for kind in KINDS:                                                # (what the chains returned: the counts, and the scores' sums)
        meta = handles[kind][1][3].cpu()
        assert not bool(meta[1].any()), "candidate overflow at the default capacity"
        moved[kind] = (int(meta[0].sum()), float(handles[kind][1][1].double().sum()))
    out = {"B": B, "A": A, "K": K, "dtype": "fp16", "logits": "N(-7, 1.2)", "iters": iters,
           "detections": {k: v[0] for k, v in moved.items()}, "score_sum": {k: round(v[1], 3) for k, v in moved.items()}}
    out.update(_sides(res, "us", 2))
    return out


def predict_pairs(dev, args):
    from predict_var_step import SHAPES, calibrate
    tuning.use_shipped_miopen_db(0)
    tuning.enable_conv_autotune()
    torch.manual_seed(0)
    net = P.Retinanet(num_classes=90, backbone_kind="resnet50", pretrained=False, min_size=800, max_size=1333)
    net = net.to(dev).to(memory_format=torch.channels_last)
    rng = np.random.default_rng(7)
    calibrate(net, [torch.from_numpy(rng.random((3,) + SHAPES[i], dtype=np.float32)).to(dev) for i in (0, 1)])
    images = [torch.from_numpy(rng.random((3,) + SHAPES[0], dtype=np.float32)).to(dev)]
    pred = CapturedPredict(net, [CANVAS], amp_dtype=AMP)
    res, dets = {k: [] for k in KINDS}, {}
    for _ in range(args.rounds):
        for kind in KINDS:
            net.nms = kind
            for _ in range(args.warmup):
                pred(images)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                d = pred(images)
            torch.cuda.synchronize()
            res[kind].append((time.perf_counter() - t0) / args.steps * 1e3)
            dets[kind] = len(d[0]["scores"])
    net.nms = "hard"
    out = {"workload": f"R50-FPN bf16 eval CapturedPredict, B=1 of 3x{SHAPES[0][0]}x{SHAPES[0][1]}, min 800 / max 1333, canvas {CANVAS[0]} x {CANVAS[1]}",
           "steps": args.steps, "warmup": args.warmup, "detections": dets, "stats": dict(pred.stats)}
    out.update(_sides(res, "ms", 3))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--no-predict", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    line = {"tool": "soft_nms_step", "rounds": args.rounds, "detect_chain": chain_pairs(dev, args.rounds, args.iters)}
    if not args.no_predict:
        line["predict"] = predict_pairs(dev, args)
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
