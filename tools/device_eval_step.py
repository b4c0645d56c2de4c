#!/usr/bin/env python3
"""COCO bbox AP of a test set on the host (coco_eval.BBoxEval, interpreted) and on the device (coco_eval.DeviceBBoxEval).

A seeded synthetic test set: ``--images`` images of 800 x 1333, about 7 ground-truth boxes each over 80 categories, and 100 detections
per image -- jittered copies of the ground truth (so matches occur at every IoU threshold) plus noise boxes -- in batches of
``--batch`` as ``test_step`` hands them to ``CocoEvaluator.update``.  Two ways over the same detections:
  (a) ``CocoEvaluator(gt, ["bbox"])``: the host path of the parent commit, detections as CPU tensors;
  (b) ``CocoEvaluator(gt, ["bbox"], device="cuda")``: detections as CUDA tensors (what ``net.predict`` returns), kept on the device;
      the matching and the precision / recall rows are the two kernels of csrc/eval.hip.
Each is timed over ``update`` for all batches plus ``accumulate``, wall clock, the device drained at both ends of (b); (b) runs
``--reps`` times after one warm-up and the median is reported.  ``kernels_ms`` are the two launches' own times from device events
(``ops.enable_timing``) in the last repetition.  ``predict_s`` = images / ``--predict-rate`` is what predicting the same images costs
at the recorded ``bench.py --mode predict`` rate: the expectation to confirm or refute is that (b) costs less than that.  The 12
statistics of the two paths must be equal, or the tool fails.  ``--skip-host`` leaves (a) out (at 5 000 images it takes minutes).
Prints one JSON line (and writes it to ``--out``).

usage: device_eval_step.py [--images 500] [--batch 8] [--reps 3] [--predict-rate 650] [--skip-host] [--out FILE]"""
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

from pytorch_retinanet_amd import ops                                                   # noqa: E402
from pytorch_retinanet_amd.coco_eval import CocoEvaluator                               # noqa: E402

H, W, CATS, DETS = 800, 1333, 80, 100


def test_set(n_images: int, seed: int = 0):
    "-> (gt rows, [per image {boxes xyxy f32, scores, labels}] as CPU tensors)"
    rng = np.random.default_rng(seed)
    gt, preds = [], []
    for img in range(n_images):
        k = int(rng.integers(3, 12))                                                    # about 7 per image
        wh = np.exp(rng.uniform(np.log(12), np.log(500), (k, 2)))                       # small, medium and large boxes
        xy = rng.uniform(0, 1, (k, 2)) * np.maximum(np.array([W, H]) - wh, 1.0)
        g = np.concatenate([xy, xy + wh], 1).astype(np.float32)
        cat = rng.integers(1, CATS + 1, k)
        crowd = rng.random(k) < 0.03
        for b, c, w in zip(g, cat, crowd):
            bw, bh = float(b[2] - b[0]), float(b[3] - b[1])
            gt.append({"image_id": img, "category_id": int(c), "bbox": [float(b[0]), float(b[1]), bw, bh], "area": bw * bh, "iscrowd": int(w)})
        n_jit = min(DETS, 4 * k)
        src = rng.integers(0, k, n_jit)
        size = np.concatenate([g[src, 2:] - g[src, :2]] * 2, 1)
        jit = g[src] + rng.normal(0, 0.06, (n_jit, 4)).astype(np.float32) * size       # IoU from ~0.5 to ~1 with the source
        noise_wh = np.exp(rng.uniform(np.log(12), np.log(500), (DETS - n_jit, 2)))
        noise_xy = rng.uniform(0, 1, (DETS - n_jit, 2)) * np.maximum(np.array([W, H]) - noise_wh, 1.0)
        boxes = np.concatenate([jit, np.concatenate([noise_xy, noise_xy + noise_wh], 1)]).astype(np.float32)
        boxes[:, 2:] = np.maximum(boxes[:, 2:], boxes[:, :2] + 1.0)
        labels = np.concatenate([np.where(rng.random(n_jit) < 0.9, cat[src], rng.integers(1, CATS + 1, n_jit)), rng.integers(1, CATS + 1, DETS - n_jit)])
        scores = np.concatenate([rng.uniform(0.2, 1.0, n_jit), rng.uniform(0.05, 0.6, DETS - n_jit)]).astype(np.float32)
        preds.append({"boxes": torch.from_numpy(boxes), "scores": torch.from_numpy(scores), "labels": torch.from_numpy(labels.astype(np.int64))})
    return gt, preds


def run(ev, preds, batch):
    for b in range(0, len(preds), batch):
        ev.update({b + j: p for j, p in enumerate(preds[b:b + batch])})
    ev.accumulate()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=500)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--predict-rate", type=float, default=650.0, help="images/s of bench.py --mode predict")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gt, preds = test_set(a.images)
    dev = torch.device("cuda:0")
    on_dev = [{k: v.to(dev) for k, v in p.items()} for p in preds]
    res = {"tool": "device_eval_step", "images": a.images, "ground_truth": len(gt), "detections": a.images * DETS, "categories": CATS,
           "batch": a.batch, "predict_rate_images_per_s": a.predict_rate, "predict_s": a.images / a.predict_rate}
    stats_host = None
    if not a.skip_host:
        ev = CocoEvaluator([dict(g) for g in gt], ["bbox"])
        t0 = time.perf_counter()
        run(ev, preds, a.batch)
        res["host_s"] = time.perf_counter() - t0
        ev.summarize(verbose=False)
        stats_host = ev.coco_eval["bbox"].stats
    times = []
    for rep in range(a.reps + 1):                                                       # the first is the warm-up
        ev = CocoEvaluator([dict(g) for g in gt], ["bbox"], device=dev)                 # (the ground-truth upload is the constructor's, as in test_dataloader)
        last = rep == a.reps
        ops.enable_timing(last)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(ev, on_dev, a.batch)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        if last:
            res["kernels_ms"] = {k: sum(e0.elapsed_time(e1) for e0, e1 in v) for k, v in ops.timing_events().items()}
            ops.enable_timing(False)
    ev.summarize(verbose=False)
    stats_dev = ev.coco_eval["bbox"].stats
    res["device_s"] = float(np.median(times[1:]))
    res["device_s_all"] = times[1:]
    res["device_first_s"] = times[0]
    res["stats"] = stats_dev.tolist()
    if stats_host is not None:
        res["stats_equal"] = bool(np.array_equal(stats_host, stats_dev))
        res["speedup"] = res["host_s"] / res["device_s"]
    res["device_cheaper_than_predict"] = bool(res["device_s"] < res["predict_s"])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if stats_host is not None and not res["stats_equal"]:
        sys.exit("the two paths disagree: " + str(stats_host.tolist()) + " vs " + str(stats_dev.tolist()))


if __name__ == "__main__":
    main()
