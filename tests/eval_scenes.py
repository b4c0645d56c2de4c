"""Shared inputs of the device-evaluator tests (``test_device_eval.py``, ``test_device_eval_gpu.py``): seeded scenes on an integer
grid, the hand-made matching cases, and the host references (``BBoxEval`` itself).  No GPU is touched here."""
import copy

import numpy as np
import torch

from pytorch_retinanet_amd.coco_eval import BBoxEval, CocoEvaluator

IMG_IDS = [41, 7, 19, 3, 88, 52, 11, 64]             # shuffled on purpose: the evaluator sorts them
CATS = [1, 2, 3, 4, 5]
DET_ONLY_CAT = 9                                     # a category that only detections name
SCENE_SEEDS = (0, 1, 2)
GRID = 8                                             # box corners are multiples of it, so IoU ties between rows occur


def _xyxy(rng, n, lo=1, hi=12):
    x, y = rng.integers(0, 20, n) * GRID, rng.integers(0, 20, n) * GRID
    w, h = rng.integers(lo, hi, n) * GRID, rng.integers(lo, hi, n) * GRID
    return np.stack([x, y, x + w, y + h], 1).astype(np.float32)


def random_scene(seed: int):
    """-> (gt rows, predictions {image id: {"boxes" xyxy f32, "scores" f32, "labels" i64}}).  8 images, 5 categories (+ one that only
    detections name), corners on a grid of 8, scores on a grid of 1/16 (equal scores occur), a few crowd rows, one pair of image
    IMG_IDS[0] / category 1 with 70 ground-truth rows (more than one strip of 64), IMG_IDS[1] without detections, IMG_IDS[2] without
    ground truth.  Detections are copies of ground truth, shifted copies and noise, so matches occur at every threshold."""
    rng = np.random.default_rng(seed)
    gt, preds = [], {}
    for n, img in enumerate(IMG_IDS):
        boxes, cats, crowd = [], [], []
        if n != 2:
            k = int(rng.integers(3, 9))
            boxes.append(_xyxy(rng, k))
            cats.append(rng.choice(CATS, k))
            crowd.append((rng.random(k) < 0.15).astype(np.int64))
        if n == 0:                                   # the dense pair: 70 small rows of category 1, many of them identical
            boxes.append(_xyxy(rng, 70, 1, 4))
            cats.append(np.full(70, 1))
            crowd.append((rng.random(70) < 0.05).astype(np.int64))
        gb = np.concatenate(boxes) if boxes else np.zeros((0, 4), np.float32)
        gc = np.concatenate(cats) if cats else np.zeros((0,), np.int64)
        gw = np.concatenate(crowd) if crowd else np.zeros((0,), np.int64)
        for b, c, w in zip(gb, gc, gw):
            x, y, bw, bh = float(b[0]), float(b[1]), float(b[2] - b[0]), float(b[3] - b[1])
            gt.append({"image_id": img, "category_id": int(c), "bbox": [x, y, bw, bh], "area": bw * bh, "iscrowd": int(w)})
        if n == 1:
            continue
        parts, labels = [], []
        if len(gb):
            take = rng.integers(0, len(gb), min(len(gb), 40))
            parts.append(gb[take])                                            # exact copies (IoU 1, and ties between identical rows)
            labels.append(gc[take])
            shift = gb[take].copy()
            shift[:, [0, 2]] += GRID * rng.integers(0, 2, len(take))[:, None].astype(np.float32)
            shift[:, 3] += GRID * rng.integers(0, 3, len(take)).astype(np.float32)
            parts.append(shift)                                               # partial overlaps: some thresholds only
            labels.append(np.where(rng.random(len(take)) < 0.2, rng.choice(CATS, len(take)), gc[take]))
        k = int(rng.integers(4, 12))
        parts.append(_xyxy(rng, k))                                           # noise
        labels.append(rng.choice(CATS + [DET_ONLY_CAT], k))
        db, dl = np.concatenate(parts), np.concatenate(labels)
        order = rng.permutation(len(db))
        scores = (rng.integers(1, 16, len(db)) / 16.0).astype(np.float32)
        preds[img] = {"boxes": torch.from_numpy(db[order]), "scores": torch.from_numpy(scores), "labels": torch.from_numpy(dl[order].astype(np.int64))}
    return gt, preds


def host_evaluator(gt, preds, batches=3):
    "``CocoEvaluator`` on the host, the predictions fed in ``batches`` updates -> the evaluator after ``accumulate`` and ``summarize``."
    ev = CocoEvaluator(copy.deepcopy(gt), ["bbox"])
    feed(ev, preds, batches)
    ev.accumulate()
    ev.summarize(verbose=False)
    return ev


def feed(ev, preds, batches=3, to=None):
    ids = list(preds)
    for b in range(batches):
        part = {i: ({k: (v if to is None else v.to(to)) for k, v in preds[i].items()}) for i in ids[b::batches]}
        if part:
            ev.update(part)


# ---- hand-made cases for the matching kernel: (name, ground truth rows [x, y, w, h, iscrowd], detections [x1, y1, x2, y2, score]) -----
def _row(x, y, w, h, crowd=0):
    return [float(x), float(y), float(w), float(h), crowd]


def match_cases():
    rng = np.random.default_rng(5)

    def many_gt(n):
        b = _xyxy(rng, n, 1, 5)
        return [_row(x1, y1, x2 - x1, y2 - y1, int(rng.random() < 0.1)) for x1, y1, x2, y2 in b.tolist()]

    def dets_on(rows, n):
        out = []
        for j in range(n):
            x, y, w, h, _ = rows[int(rng.integers(0, len(rows)))] if rows else _row(8, 8, 16, 16)
            dx = GRID * int(rng.integers(0, 2))
            out.append([x + dx, y, x + dx + w, y + h, int(rng.integers(1, 9)) / 8.0])
        return out

    cases = [("no ground truth", [], [[0, 0, 16, 16, 0.5], [8, 8, 24, 24, 0.25]]),
             ("no detections", [_row(0, 0, 16, 16), _row(8, 8, 16, 16, 1)], []),
             ("one ground truth", [_row(0, 0, 40, 40)], [[0, 0, 40, 40, 0.9], [0, 0, 40, 30, 0.8], [100, 100, 140, 140, 0.7]])]
    for n in (63, 64, 65, 130):                                               # the strip seam
        rows = many_gt(n)
        rows[-1] = list(rows[0])                                              # the LAST row repeats the first: a tie across the strips
        cases.append((f"{n} ground truth", rows, dets_on(rows, 24) + [rows[0][:2] + [rows[0][0] + rows[0][2], rows[0][1] + rows[0][3], 1.0]]))
    for n in (100, 103):                                                      # the cut at 100 detections
        rows = many_gt(12)
        cases.append((f"{n} detections", rows, dets_on(rows, n)))
    cases += [
        ("two identical ground truth: the tie goes to the later row", [_row(0, 0, 40, 40), _row(0, 0, 40, 40), _row(200, 200, 40, 40)],
         [[0, 0, 40, 40, 0.9], [0, 0, 40, 40, 0.8], [0, 0, 40, 40, 0.7]]),
        ("equal scores keep their order", [_row(0, 0, 40, 40)], [[0, 0, 40, 32, 0.5], [0, 0, 40, 40, 0.5], [0, 0, 40, 36, 0.5]]),
        ("one crowd region matched by three detections", [_row(100, 100, 200, 200, 1), _row(0, 0, 40, 40)],
         [[110, 110, 150, 150, 0.9], [120, 120, 170, 170, 0.8], [150, 150, 200, 200, 0.7], [0, 0, 40, 40, 0.6]]),
        # 20 x 20 = 400 px^2: cared-for in "all" and "small", ignored (not crowd) in "medium" and "large": matched once there, then gone
        ("an out-of-range ground truth is matched once", [_row(0, 0, 20, 20)], [[0, 0, 20, 20, 0.9], [0, 0, 20, 20, 0.8]]),
        # the detection overlaps a crowd row at IoU 1 (union = its own area) and a cared-for row at 0.64: the cared-for row wins
        ("a cared-for match at a lower IoU beats an ignored one", [_row(0, 0, 200, 200, 1), _row(0, 0, 50, 32)],
         [[0, 0, 50, 50, 0.9]]),
        ("IoU exactly 0.5", [_row(0, 0, 200, 200)], [[0, 0, 200, 100, 0.9]]),
        ("zero areas", [_row(10, 10, 0, 30), _row(0, 0, 40, 40)], [[10, 10, 10, 40, 0.9], [5, 5, 5, 5, 0.8], [0, 0, 40, 40, 0.7]]),
    ]
    return cases


def match_reference(rows, dets):
    """``BBoxEval._evaluate_img`` on one pair, per area range -> (matched uint64 [D], ignored uint64 [D], gt_ignored uint8 [G]) with the
    kernel's bit layout; detections in the kernel's input order (descending score, stable) and cut at 100."""
    ev = BBoxEval([])
    T = len(ev.iou_thrs)
    g = [{"bbox": r[:4], "_area": r[2] * r[3], "iscrowd": r[4]} for r in rows]
    order = sorted(range(len(dets)), key=lambda j: -dets[j][4])
    xyxy = np.array([dets[j][:4] for j in order], dtype=np.float32).reshape(-1, 4)
    d = [{"bbox": [float(b[0]), float(b[1]), float(b[2] - b[0]), float(b[3] - b[1])], "score": float(np.float32(dets[j][4]))} for b, j in zip(xyxy, order)]
    matched, ignored, gig = np.zeros(len(d), np.uint64), np.zeros(len(d), np.uint64), np.zeros(len(g), np.uint8)
    for a, rng in enumerate(ev.area_rng):
        e = ev._evaluate_img(g, d, rng)
        if e is None:
            continue
        ig_sorted = e["g_ig"]                                                  # (sorted cared-for first; the flags per original row:)
        flags = np.array([bool(x["iscrowd"]) or not (rng[0] <= x["_area"] <= rng[1]) for x in g], dtype=bool)
        assert sorted(flags.tolist()) == ig_sorted.tolist()
        gig |= (flags.astype(np.uint8) << a).astype(np.uint8)
        for t in range(T):
            n = e["dtm"].shape[1]
            matched[:n] |= e["dtm"][t].astype(np.uint64) << np.uint64(a * T + t)
            ignored[:n] |= e["dt_ig"][t].astype(np.uint64) << np.uint64(a * T + t)
    return xyxy, matched, ignored, gig


def scene_properties(gt, preds):
    """From ``BBoxEval`` alone: does the scene hold (a) a detection whose best IoU >= 0.5 is shared by two available rows of its pair
    (the tie rule decides), (b) a detection matched to an ignored row, (c) a pair with more than 64 ground-truth rows, (d) rows of
    ``recall`` at -1, (e) equal scores inside a pair?"""
    from collections import defaultdict
    from pytorch_retinanet_amd.coco_eval import _iou_xywh, prepare_for_coco_detection
    ev = BBoxEval(copy.deepcopy(gt), prepare_for_coco_detection(preds)).evaluate()
    gts, dts = defaultdict(list), defaultdict(list)
    for x in ev.gt:
        gts[x["image_id"], x["category_id"]].append(x)
    for x in ev.dt:
        dts[x["image_id"], x["category_id"]].append(x)
    ties = ignored_match = equal_scores = False
    for key in set(gts) & set(dts):
        g, d = gts[key], dts[key]
        ious = _iou_xywh(np.array([x["bbox"] for x in d], dtype=np.float64), np.array([x["bbox"] for x in g], dtype=np.float64),
                         np.array([bool(x["iscrowd"]) for x in g]))
        best = ious.max(1)
        ties |= bool((((ious == best[:, None]).sum(1) > 1) & (best >= 0.5)).any())
        equal_scores |= len({x["score"] for x in d}) < len(d)
        for rng in ev.area_rng:
            e = ev._evaluate_img(g, d, rng)
            ignored_match |= bool((e["dtm"] & e["dt_ig"]).any())
    return {"ties": ties, "ignored_match": ignored_match, "dense_pair": max(len(v) for v in gts.values()) > 64,
            "minus_one_rows": bool((ev.eval["recall"] == -1).any()) and bool((ev.eval["recall"] > 0).any()), "equal_scores": equal_scores}
