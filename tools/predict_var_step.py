#!/usr/bin/env python3
"""Inference on batches whose IMAGE SIZES change from call to call (graph.CapturedPredict).

R50-FPN, bf16 autocast, eval mode, min_size 800 / max_size 1333; batches of B = 1 and B = 16 whose raw sizes are drawn per call from a
seed-fixed list of COCO-like landscape shapes that share one canvas class (800 x 1344).  A random-init net detects nothing, so the
BatchNorm statistics are set by one train-mode pass and the class head is rescaled until the eval logits are ~N(-7, 1.2): with A x K =
18 M (anchor, class) pairs per image that leaves ~1e4 candidates above the 0.05 score threshold, the regime of the ``e2e_full.npz``
fixture and well inside the detect chain's default capacity of 2**18 (at ``__graft_entry__.smoke``'s N(-3.5, 1.2) a third of the pairs
pass and every call of this size overflows).  Timed three ways per B, interleaved for ``--rounds`` rounds:
  (a) ``CapturedPredict`` on the varying batches: one capture per (B, canvas class, pixel class), then replays;
  (b) eager ``Retinanet.predict_staged`` on the same batches over the same class canvas, with the same staging and read-back -- the
      yardstick (a) is held against;
  (c) ``net.predict`` on the same batches, each over its OWN canvas (what a batch pays for its class canvas is (b) - (c)).
ms/call is wall time over ``--steps`` calls with the device drained at both ends; every call ends in its own wait for the result, so
host ms/call is measured apart: (a) ``CapturedPredict.host_seconds`` over the timed calls -- everything a whole ``__call__`` does on
the host (class and key arithmetic, the weights stamp, staging, the replay, the copy's enqueue, building the dicts) except its wait
for the device; (b) the time the eager enqueue of stage + ``predict_staged`` + copy takes to return, the wait left out (building the
dicts is not in it); (c) the whole call, ``detect_levels``' own read-back -- a wait -- included.  Before anything is timed (c) is run
once over every own canvas the data holds, so no timed call meets a shape for the first time (the vendor library searches its
algorithms then: hundreds of ms).  Prints one JSON line (and writes it to ``--out``).

usage: predict_var_step.py [--steps 20] [--warmup 4] [--rounds 2] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import pytorch_retinanet_amd as P                                   # noqa: E402
from pytorch_retinanet_amd import ops, tuning                       # noqa: E402
from pytorch_retinanet_amd.graph import CapturedPredict, image_pixel_class    # noqa: E402
from pytorch_retinanet_amd.norm import note_raw_write               # noqa: E402

# COCO-like landscape shapes: every one resizes into the canvas 800 x 1344
SHAPES = [(480, 640), (427, 640), (426, 640), (428, 640), (500, 640), (375, 500), (333, 500), (480, 600), (512, 640),
          (424, 640), (360, 640), (457, 640), (600, 800), (534, 800), (480, 800)]
CANVAS = (800, 1344)
AMP = torch.bfloat16


def calibrate(net, images):
    "Eval-mode BatchNorm statistics from one train-mode pass, then a class head whose eval logits are ~N(-7, 1.2)."
    with torch.no_grad(), torch.autocast("cuda", dtype=AMP):
        bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
        old = [m.momentum for m in bns]
        for m in bns:
            m.momentum = 1.0
        net.train()
        il, _ = net.transform(images, None)
        net._features(il.tensors)
        for m, mo in zip(bns, old):
            m.momentum = mo
    net.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=AMP):
        il, _ = net.transform(images, None)
        _, out = net._features(il.tensors)
        head = net.retinanet_head.classification_head.class_subnet_output
        raw = out["cls_preds"].float() - float(head.bias.float().mean())
        f = 1.2 / max(float(raw.std()), 1e-12)
        head.weight.mul_(f)
        head.bias.fill_(-7.0 - f * float(raw.mean()))
    note_raw_write()


def batches(rng, n, B, dev):
    return [[torch.from_numpy(rng.random((3,) + SHAPES[int(i)], dtype=np.float32)).to(dev) for i in rng.integers(0, len(SHAPES), size=B)]
            for _ in range(n)]


class StagedEager:
    "(b): what CapturedPredict does per call -- stage, the pass, one read-back -- without the graph."
    def __init__(self, net, B, dev):
        self.net, self.B = net, B
        self.staged = ops.new_image_arena(B, image_pixel_class(SHAPES), dev, CANVAS)
        self.host = torch.empty((ops.detect_result_layout(B, net.detections_per_img)["total"],), dtype=torch.uint8).pin_memory()

    def enqueue(self, images):
        ops.image_stage(images, self.staged)
        with torch.autocast("cuda", dtype=AMP, cache_enabled=False):
            block = self.net.predict_staged(self.staged)
        self.host.copy_(block, non_blocking=True)

    def __call__(self, images):
        self.enqueue(images)
        torch.cuda.current_stream().synchronize()
        return ops.detect_result_dicts(self.host.clone(), self.B, self.net.detections_per_img)


def plain(net):
    def call(images):
        with torch.autocast("cuda", dtype=AMP):
            return net.predict(images)
    return call


def timed(fn, data):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for images in data:
        n += sum(len(d["scores"]) for d in fn(images))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / len(data) * 1e3, n / len(data)


def host_ms(enqueue, data):
    "The time the calls take to return with the final wait left out (the device is drained before and after the loop)."
    torch.cuda.synchronize()
    host = 0.0
    for images in data:
        h0 = time.perf_counter()
        enqueue(images)
        host += time.perf_counter() - h0
    torch.cuda.synchronize()
    return host / len(data) * 1e3


def own_canvas(net, images):
    tr = net.transform
    return (len(images),) + tuple(tr._canvas(tr.staged_eval_bounds([(int(im.shape[1]), int(im.shape[2])) for im in images])))


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
    net = net.to(dev).to(memory_format=torch.channels_last)
    rng = np.random.default_rng(7)
    calibrate(net, batches(rng, 1, 2, dev)[0])
    n = args.warmup + args.steps
    line = {"tool": "predict_var_step",
            "workload": f"R50-FPN bf16 eval predict, raw sizes from {len(SHAPES)} COCO-like shapes per image and call, min 800 / max 1333, "
                        f"class canvas {CANVAS[0]} x {CANVAS[1]}",
            "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds}
    for B in (1, 16):
        data = batches(rng, n * args.rounds, B, dev)
        pred = CapturedPredict(net, [CANVAS], amp_dtype=AMP)
        eager = StagedEager(net, B, dev)
        fns = {"a": pred, "b": eager, "c": plain(net)}
        res = {k: [] for k in fns}
        host_a = []
        met = set()
        for images in data:                                          # (c): every own canvas once, before anything is timed
            if own_canvas(net, images) not in met:
                met.add(own_canvas(net, images))
                fns["c"](images)
        for r in range(args.rounds):
            for k, fn in fns.items():
                part = data[r * n:(r + 1) * n]
                for images in part[:args.warmup]:
                    fn(images)
                h0, c0 = pred.host_seconds, pred.host_calls
                res[k].append(timed(fn, part[args.warmup:]))
                if k == "a" and pred.host_calls > c0:
                    host_a.append((pred.host_seconds - h0) / (pred.host_calls - c0) * 1e3)
        ms = {k: float(np.mean([v[0] for v in res[k]])) for k in res}
        part = data[args.warmup:n]
        host = {"a": float(np.mean(host_a)), "b": host_ms(eager.enqueue, part), "c": host_ms(plain(net), part)}
        line[f"B{B}"] = {"a_captured_predict_ms_per_call": round(ms["a"], 3), "b_eager_staged_same_canvas_ms_per_call": round(ms["b"], 3),
                         "c_net_predict_own_canvas_ms_per_call": round(ms["c"], 3),
                         "a_vs_b": round(ms["a"] / ms["b"], 4), "class_canvas_cost_b_vs_c": round(ms["b"] / ms["c"], 4),
                         "own_canvases_in_data": len(met),
                         "host_ms_per_call": {k: round(v, 3) for k, v in host.items()},
                         "per_round_ms": {k: [round(v[0], 3) for v in res[k]] for k in res},
                         "detections_per_call": {k: round(float(np.mean([v[1] for v in res[k]])), 1) for k in res},
                         "a_stats": dict(pred.stats), "images_per_s": {k: round(B / ms[k] * 1e3, 1) for k in ms}}
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
