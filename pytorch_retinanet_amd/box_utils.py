"""Box helpers with the reference's names (``retinanet/box_utils.py:11-80``).

``matcher`` and ``activ_2_bbox`` are the HIP kernels K2 / K4.  ``bbox_2_activ`` and
the two ``convert_*`` helpers are small torch expressions kept for surface parity:
on the training path the encode step is fused into the loss kernel (K3) and never
runs as a separate op.
"""
from typing import Optional

import torch
from torch import Tensor

from . import ops
from .config import BBOX_REG_WEIGHTS, ENCODE_LOG_EPS, IOU_THRESHOLDS_BACKGROUND, IOU_THRESHOLDS_FOREGROUND, LOGIT_SHIFT
from .utilities import ifnone


def convert_xywh(boxes: Tensor) -> Tensor:
    "XYXY -> (cx, cy, w, h)  (box_utils.py:11-15)"
    return torch.cat([(boxes[:, :2] + boxes[:, 2:]) / 2, boxes[:, 2:] - boxes[:, :2]], 1)


def convert_x1y1x2y2(boxes: Tensor) -> Tensor:
    "(cx, cy, w, h) -> XYXY  (box_utils.py:18-22)"
    half = boxes[:, 2:] / 2
    return torch.cat([boxes[:, :2] - half, boxes[:, :2] + half], 1)


def bbox_2_activ(bboxes: Tensor, anchors: Tensor) -> Tensor:
    "Regression targets of `bboxes` w.r.t. `anchors`, both XYXY (box_utils.py:25-34)."
    b, a = convert_xywh(bboxes), convert_xywh(anchors)
    centers = (b[..., :2] - a[..., :2]) / a[..., 2:]
    sizes = torch.log(b[..., 2:] / a[..., 2:] + ENCODE_LOG_EPS)
    return torch.cat([centers, sizes], -1).mul_(b.new_tensor([BBOX_REG_WEIGHTS]))


def activ_2_bbox(activations: Tensor, anchors: Tensor, decode: str = "reference") -> Tensor:
    """Model activations -> XYXY boxes (box_utils.py:37-48), HIP kernel K4.

    ``decode="reference"`` keeps the reference's behaviour: sizes come from ``exp(activations[..., :2])``
    (SURVEY Q4); ``decode="standard"`` takes them from ``activations[..., 2:]`` (the inverse of ``bbox_2_activ``,
    ``decode_boxes_reference``).  Either way the activations are divided IN PLACE by ``BBOX_REG_WEIGHTS``
    (Q5; a value no-op with the default unit weights)."""
    if decode not in ops.BOX_DECODES:
        raise ValueError(f"decode must be one of {ops.BOX_DECODES}, got {decode!r}")
    if any(w != 1.0 for w in BBOX_REG_WEIGHTS):
        activations.div_(activations.new_tensor([BBOX_REG_WEIGHTS]))
    return ops.decode_clip(activations, anchors, None, decode=decode)


def decode_boxes_reference(deltas, anchors, reg_w=BBOX_REG_WEIGHTS, decode: str = "standard", image_hw=None):
    """K4's two decodes restated in numpy fp32, operation for operation (the tests' yardstick; CPU tensors or arrays).  ``deltas``
    [..., 4] (any float dtype: widened to fp32 first), ``anchors`` [A, 4] or ``deltas``' shape, ``reg_w`` four weights -> XYXY boxes,
    a torch tensor when ``deltas`` is one, else a numpy array.  The rule (include/retinanet_hip.h, K4):
      1. t[j] = d[j] / reg_w[j];
      2. acx = (x1 + x2) / 2, acy likewise, aw = x2 - x1, ah = y2 - y1;
      3. cx = aw * t0 + acx, cy = ah * t1 + acy;
      4. "standard": sw = t2 > CLIP ? CLIP : t2, sh likewise (a NaN stays NaN); "reference": sw = t0, sh = t1 (Q4), no clip;
      5. w = aw * exp(sw), h = ah * exp(sh);
      6. the box is (cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2);
    ``image_hw`` ([B, 2] rows of (h, w) for deltas [B, A, 4], or one (h, w)): then clipped to the image as K4 clips.  ``exp`` is
    numpy's fp32 one, which may differ from the device library's by an ulp: compare with the K4 bar, not bit for bit."""
    import numpy as np
    if decode not in ops.BOX_DECODES:
        raise ValueError(f"decode must be one of {ops.BOX_DECODES}, got {decode!r}")
    as_torch = isinstance(deltas, Tensor)
    d = deltas.detach().to(torch.float32).cpu().numpy() if as_torch else np.asarray(deltas, dtype=np.float32)
    a = anchors.detach().to(torch.float32).cpu().numpy() if isinstance(anchors, Tensor) else np.asarray(anchors, dtype=np.float32)
    rw = np.asarray([float(v) for v in reg_w], dtype=np.float32)
    if rw.shape != (4,):
        raise ValueError(f"reg_w must hold four weights, got {reg_w!r}")
    two = np.float32(2.0)
    with np.errstate(all="ignore"):
        t = d / rw
        acx, acy = (a[..., 0] + a[..., 2]) / two, (a[..., 1] + a[..., 3]) / two
        aw, ah = a[..., 2] - a[..., 0], a[..., 3] - a[..., 1]
        cx, cy = aw * t[..., 0] + acx, ah * t[..., 1] + acy
        if decode == "standard":
            clip = np.float32(ops.BOX_XFORM_CLIP)
            sw, sh = np.where(t[..., 2] > clip, clip, t[..., 2]), np.where(t[..., 3] > clip, clip, t[..., 3])
        else:
            sw, sh = t[..., 0], t[..., 1]
        w, h = aw * np.exp(sw), ah * np.exp(sh)
        out = np.stack([cx - w / two, cy - h / two, cx + w / two, cy + h / two], -1).astype(np.float32)
        if image_hw is not None:
            hw = np.asarray(image_hw, dtype=np.int64).astype(np.float32)
            hh, ww = (hw[..., 0], hw[..., 1]) if hw.ndim == 1 else (hw[:, 0][:, None], hw[:, 1][:, None])
            zero = np.float32(0.0)
            for j, hi in ((0, ww), (1, hh), (2, ww), (3, hh)):
                v = out[..., j]
                v = np.where(v < zero, zero, v)              # K4's clampf: a NaN fails both comparisons and stays
                out[..., j] = np.where(v > hi, hi, v)
    return torch.from_numpy(out) if as_torch else out


def soft_nms_reference(boxes, scores, iou_thr, method, sigma=0.5, min_score=1e-3, max_keep=None, on_pick=None):
    """Soft-NMS of ONE segment restated in numpy fp32, operation for operation (the rule next to K6 in include/retinanet_hip.h; the
    tests' yardstick; CPU tensors or arrays).  ``boxes`` [n, 4] XYXY, ``scores`` [n] (expected >= 0), payload = index:
      0. area = (x2 - x1) * (y2 - y1); inter = max(0, xx2 - xx1) * max(0, yy2 - yy1); iou = inter / ((area_i + area_j) - inter);
      1. pick the live entry with the smallest key (inv_ordered(current score) << 32) | index: the highest score, ties to the lower index;
      2. stop if there is none, its score is not > ``min_score``, or ``max_keep`` (None / <= 0: no cap) entries are kept;
      3. emit it with its current score; it is dead;
      4. every live entry with iou > 0 against it: "soft_linear": if iou > ``iou_thr``, s = s * (1 - iou); "soft_gaussian":
         s = s * float32(exp(-(float64(iou) * float64(iou)) / float64(float32(sigma)))).
    ``on_pick(i, scores, live)``: called at every step 3 with the picked index, the current scores and the live mask (the pick still
    live) -- for tests that look at how close the runner-up was.
    -> (kept indices int64 [m], their scores float32 [m]), in pick order.  ``exp`` is numpy's double one, which may differ from the
    device library's in the last place: a Gaussian weight may differ by one fp32 unit."""
    import numpy as np
    if method not in ops.NMS_KINDS[1:]:
        raise ValueError(f"method must be one of {ops.NMS_KINDS[1:]}, got {method!r}")
    b = boxes.detach().to(torch.float32).cpu().numpy() if isinstance(boxes, Tensor) else np.asarray(boxes, dtype=np.float32)
    s = scores.detach().to(torch.float32).cpu().numpy() if isinstance(scores, Tensor) else np.asarray(scores, dtype=np.float32)
    b, s = b.reshape(-1, 4), s.reshape(-1).copy()
    n = s.shape[0]
    thr, floor, one, zero = np.float32(iou_thr), np.float32(min_score), np.float32(1.0), np.float32(0.0)
    sig = np.float64(np.float32(sigma))
    cap = int(max_keep) if max_keep is not None and int(max_keep) > 0 else n
    idx = np.arange(n, dtype=np.uint64)

    def keys(v):                                             # rn::inv_ordered(score) << 32 | index
        u = v.view(np.uint32)
        u = u ^ np.where(u >> np.uint32(31), np.uint32(0xffffffff), np.uint32(0x80000000))
        return ((~u).astype(np.uint64) << np.uint64(32)) | idx

    live = np.ones(n, dtype=bool)
    keep, out = [], []
    with np.errstate(all="ignore"):
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        while len(keep) < cap and live.any():
            k = keys(s)
            k[~live] = np.uint64(0xffffffffffffffff)
            i = int(np.argmin(k))
            if not s[i] > floor:
                break
            if on_pick is not None:
                on_pick(i, s, live)
            keep.append(i)
            out.append(s[i])
            live[i] = False
            w = np.where(b[i, 2] < b[:, 2], b[i, 2], b[:, 2]) - np.where(b[i, 0] > b[:, 0], b[i, 0], b[:, 0])
            h = np.where(b[i, 3] < b[:, 3], b[i, 3], b[:, 3]) - np.where(b[i, 1] > b[:, 1], b[i, 1], b[:, 1])
            w, h = np.where(w > zero, w, zero), np.where(h > zero, h, zero)
            inter = w * h
            iou = inter / ((area[i] + area) - inter)
            if method == "soft_linear":
                hit = live & (iou > zero) & (iou > thr)
                s[hit] = s[hit] * (one - iou[hit])
            else:
                hit = live & (iou > zero)
                d = iou[hit].astype(np.float64)
                s[hit] = s[hit] * np.exp(-(d * d) / sig).astype(np.float32)
    return np.asarray(keep, dtype=np.int64), np.asarray(out, dtype=np.float32)


def _iou_pairs_f32(t, a):
    "K2's pair arithmetic (csrc/rn_match.hpp, iou_pair) of one GT box against anchors [n,4], operation for operation in numpy fp32."
    import numpy as np
    area_t = (t[2] - t[0]) * (t[3] - t[1])
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    w = np.minimum(t[2], a[:, 2]) - np.maximum(t[0], a[:, 0])
    h = np.minimum(t[3], a[:, 3]) - np.maximum(t[1], a[:, 1])
    w = np.where(w > 0, w, np.float32(0))
    h = np.where(h > 0, h, np.float32(0))
    inter = w * h
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / ((area_t + area_a) - inter)


def atss_candidates(anchors, target, level_sizes, cells, topk: int = 9):
    """Steps 1-2 of the ATSS rule for ONE GT box: the candidate list (anchor indices, levels in order, each ascending in
    (d2, index)) as a numpy int64 array.  ``anchors`` / ``target``: numpy fp32 [A,4] / [4]."""
    import numpy as np
    half = np.float32(0.5)
    acx, acy = (anchors[:, 0] + anchors[:, 2]) * half, (anchors[:, 1] + anchors[:, 3]) * half
    gcx, gcy = (target[0] + target[2]) * half, (target[1] + target[3]) * half
    dx, dy = acx - gcx, acy - gcy
    xx, yy = dx * dx, dy * dy
    d2 = xx + yy                                           # two products and one sum, each rounded to fp32
    cells = [int(cells)] * len(level_sizes) if isinstance(cells, int) else [int(c) for c in cells]
    out, lo = [], 0
    for size, c in zip(level_sizes, cells):
        k = min(int(topk) * c, int(size))
        order = np.argsort(d2[lo:lo + size], kind="stable")[:k]      # stable: ties in d2 go to the lower index
        out.append(order.astype(np.int64) + lo)
        lo += int(size)
    return np.concatenate(out) if out else np.zeros((0,), np.int64)


def atss_matcher(anchors: Tensor, targets: Tensor, level_sizes, cells, topk: int = 9) -> Tensor:
    """ATSS (Zhang et al., CVPR 2020): match `anchors` [A,4] to `targets` [T,4] -> i64 [A], -1 background, else the target index
    (there is no ignored band).  ``level_sizes``: anchors per pyramid level, in anchor order; ``cells``: anchors per grid location
    (an int or one per level).  CUDA tensors go to the HIP kernel (``ops.atss_match``); CPU tensors run this restatement of the
    numbered rule in include/retinanet_hip.h, operation for operation, in numpy fp32 and Python doubles:
      1. centres (x1 + x2) * 0.5f, d2 = dx * dx + dy * dy in fp32;
      2. per level the k_l = min(topk * cells, A_l) anchors smallest under (d2, index); the list is the levels in order;
      3. iou_c in K2's fp32 pair arithmetic, widened to double; mean and var = sum((iou_c - mean)^2) / (n - 1) (0 for n == 1) as
         two serial double sums in list order; no square root;
      4. positive iff dev = iou_c - mean has dev >= 0 and dev * dev >= var, and the anchor centre lies inside the box by more than
         0.01f on every side (fp32);
      5. an anchor positive for several targets takes the largest fp32 IoU, ties to the lowest target index."""
    targets = targets.reshape(-1, 4)
    level_sizes = [int(s) for s in level_sizes]
    if sum(level_sizes) != anchors.shape[0]:
        raise ValueError(f"level sizes {level_sizes} do not sum to the {anchors.shape[0]} anchors")
    if anchors.is_cuda:
        off = ops.gt_offsets([targets.shape[0]], anchors.device)
        matches, _ = ops.atss_match(anchors, targets, off, 1, level_sizes, cells, topk, want_num_fg=False)
        return matches[0]
    import numpy as np
    a = anchors.detach().to(torch.float32).contiguous().numpy()
    t = targets.detach().to(torch.float32).contiguous().numpy()
    half, margin = np.float32(0.5), np.float32(0.01)
    acx, acy = (a[:, 0] + a[:, 2]) * half, (a[:, 1] + a[:, 3]) * half
    matches = np.full((a.shape[0],), -1, np.int64)
    best = np.full((a.shape[0],), -1.0, np.float32)
    for g in range(t.shape[0]):
        cand = atss_candidates(a, t[g], level_sizes, cells, topk)
        n = len(cand)
        if n == 0:
            continue
        iou = _iou_pairs_f32(t[g], a[cand])
        vals = [float(v) for v in iou]                      # widened to double
        s = 0.0
        for v in vals:                                      # (a plain loop: the built-in sum() compensates its rounding)
            s += v
        mean = s / n
        ss = 0.0
        for v in vals:
            d = v - mean
            ss += d * d
        var = ss / (n - 1) if n > 1 else 0.0
        inside = np.minimum(np.minimum(acx[cand] - t[g, 0], acy[cand] - t[g, 1]), np.minimum(t[g, 2] - acx[cand], t[g, 3] - acy[cand]))
        for j in range(n):
            dev = vals[j] - mean
            if dev >= 0.0 and dev * dev >= var and inside[j] > margin:
                i = cand[j]
                if iou[j] > best[i]:                        # strict: an equal IoU keeps the lower target index
                    best[i], matches[i] = iou[j], g
    return torch.from_numpy(matches)


def _exp_f32(v):
    "exp of an fp32 array computed through double and rounded once (what the device library's expf gives, up to an ulp)."
    import numpy as np
    with np.errstate(all="ignore"):
        return np.exp(v.astype(np.float64)).astype(np.float32)


def task_aligned_metric(logits, deltas, anchors, target, alpha: int = 1, beta: int = 6, reg_w=BBOX_REG_WEIGHTS, logit_shift: float = LOGIT_SHIFT):
    """Step 2 of the task-aligned rule for ONE GT box against n anchors, every step one rounded numpy fp32 operation: ``logits`` [n]
    (the label's logit of every anchor), ``deltas`` [n,4], ``anchors`` [n,4], ``target`` [4], all numpy fp32 -> (m [n], u [n], s [n]):
    the metric, the IoU of the standard-decoded box and the score.  The two ``exp`` go through double and are rounded once."""
    import numpy as np
    one, two, zero = np.float32(1.0), np.float32(2.0), np.float32(0.0)
    with np.errstate(all="ignore"):
        z = logits + np.float32(logit_shift)
        e = _exp_f32(-np.abs(z))
        r = one / (one + e)
        s = np.where(z >= zero, r, e * r)
        rw = np.asarray([float(v) for v in reg_w], dtype=np.float32)
        t = deltas / rw
        acx, acy = (anchors[:, 0] + anchors[:, 2]) / two, (anchors[:, 1] + anchors[:, 3]) / two
        aw, ah = anchors[:, 2] - anchors[:, 0], anchors[:, 3] - anchors[:, 1]
        cx, cy = aw * t[:, 0] + acx, ah * t[:, 1] + acy
        clip = np.float32(ops.BOX_XFORM_CLIP)
        sw, sh = np.where(t[:, 2] > clip, clip, t[:, 2]), np.where(t[:, 3] > clip, clip, t[:, 3])
        w, h = aw * _exp_f32(sw), ah * _exp_f32(sh)
        hw, hh = w / two, h / two
        px1, py1, px2, py2 = cx - hw, cy - hh, cx + hw, cy + hh
        gx1, gy1, gx2, gy2 = target
        iw = np.where(px2 < gx2, px2, gx2) - np.where(px1 > gx1, px1, gx1)
        ih = np.where(py2 < gy2, py2, gy2) - np.where(py1 > gy1, py1, gy1)
        iw, ih = np.where(iw > zero, iw, zero), np.where(ih > zero, ih, zero)
        inter = iw * ih
        union = (w * h + (gx2 - gx1) * (gy2 - gy1)) - inter
        u = np.where(union > zero, inter / np.where(union > zero, union, one), zero).astype(np.float32)
        m = np.ones_like(s)
        for _ in range(int(alpha)):
            m = m * s
        for _ in range(int(beta)):
            m = m * u
    return m.astype(np.float32), u, s.astype(np.float32)


def task_aligned_candidates(cls, box, anchors, target, label: int, topk: int = 13, alpha: int = 1, beta: int = 6,
                            reg_w=BBOX_REG_WEIGHTS, logit_shift: float = LOGIT_SHIFT):
    """Steps 1-3 of the task-aligned rule for ONE GT row: (the selected anchors, best first; their u; ALL candidates in rank order;
    their m) as numpy arrays.  ``cls`` [A,K] / ``box`` [A,4] / ``anchors`` [A,4] / ``target`` [4]: numpy fp32; ``label`` in 1..K."""
    import numpy as np
    none = (np.zeros((0,), np.int64), np.zeros((0,), np.float32), np.zeros((0,), np.int64), np.zeros((0,), np.float32))
    K = cls.shape[1]
    if not (1 <= int(label) <= K) or not np.isfinite(target).all() or not (target[2] > target[0]) or not (target[3] > target[1]):
        return none
    half = np.float32(0.5)
    acx, acy = (anchors[:, 0] + anchors[:, 2]) * half, (anchors[:, 1] + anchors[:, 3]) * half
    cand = np.nonzero((acx > target[0]) & (acx < target[2]) & (acy > target[1]) & (acy < target[3]))[0]
    if cand.size == 0:
        return none
    m, u, _ = task_aligned_metric(cls[cand, int(label) - 1], box[cand], anchors[cand], target, alpha, beta, reg_w, logit_shift)
    with np.errstate(all="ignore"):
        keep = (m > 0) & (m < np.inf) & (u >= 0)
    cand, m, u = cand[keep], m[keep], u[keep]
    key = ((~m.view(np.uint32)).astype(np.uint64) << np.uint64(32)) | cand.astype(np.uint64)     # largest m first, ties to the lower index
    order = np.argsort(key, kind="stable")
    sel = order[:int(topk)]
    return cand[sel].astype(np.int64), u[sel], cand[order].astype(np.int64), m[order]


def task_aligned_matcher(cls: Tensor, box: Tensor, anchors: Tensor, targets: Tensor, labels: Tensor, topk: int = 13, alpha: int = 1,
                         beta: int = 6, reg_w=BBOX_REG_WEIGHTS, logit_shift: float = LOGIT_SHIFT, level_sizes=None, cells=9) -> Tensor:
    """Task-aligned assignment (TOOD, Feng et al., ICCV 2021) of ONE image: the head's outputs ``cls`` [A,K] / ``box`` [A,4] (any float
    dtype: widened to fp32), ``anchors`` [A,4], ``targets`` [T,4], ``labels`` [T] in 1..K -> i64 [A], -1 background, else the target
    index (there is no ignored band).  CUDA tensors go to the HIP kernel (``ops.tal_match``; ``level_sizes`` / ``cells`` are its level
    layout, default one level); CPU tensors run this restatement of the numbered rule in include/retinanet_hip.h, operation for
    operation in numpy fp32:
      1. candidates of a row: the anchors whose centre ((x1 + x2) * 0.5f, (y1 + y2) * 0.5f) lies strictly inside the box; none for a
         label outside 1..K or a non-finite / empty box;
      2. s = the sigmoid of the label's logit + logit_shift from e = exp(-|z|) (r = 1 / (1 + e), s = z >= 0 ? r : e * r); u = the IoU
         of the standard-decoded box (``rn_box_iou_loss``'s steps 1-2); m = 1 * s * ... * s * u * ... * u (``alpha`` then ``beta``
         factors, left to right); dropped unless m > 0, m < inf and u >= 0;
      3. the ``topk`` largest m of the row over all levels together, ties to the lower anchor index;
      4. an anchor selected for several rows takes the largest fp32 u, ties to the lower row.
    The predictions are constants: nothing is differentiated.  ``exp`` is computed through double and rounded once; the device's
    ``expf`` may differ by an ulp, so a near-tie can fall the other way (the tests assert a margin)."""
    alpha, beta, topk = ops.tal_exponent(alpha, "alpha"), ops.tal_exponent(beta, "beta"), ops.tal_topk(topk)
    targets = targets.reshape(-1, 4)
    labels = labels.reshape(-1)
    if labels.shape[0] != targets.shape[0]:
        raise ValueError(f"{labels.shape[0]} labels for {targets.shape[0]} boxes")
    if cls.shape[0] != anchors.shape[0] or box.shape[0] != anchors.shape[0]:
        raise ValueError(f"head outputs of {cls.shape[0]} / {box.shape[0]} rows for {anchors.shape[0]} anchors")
    if anchors.is_cuda:
        sizes = [int(anchors.shape[0])] if level_sizes is None else [int(s) for s in level_sizes]
        off = ops.gt_offsets([targets.shape[0]], anchors.device)
        lo, cl, bl = 0, [], []
        for s in sizes:
            cl.append(cls[None, lo:lo + s].contiguous())
            bl.append(box[None, lo:lo + s].contiguous())
            lo += s
        matches, _ = ops.tal_match(cl, bl, anchors, targets, labels, off, 1, sizes, cells, topk, alpha, beta, reg_w=reg_w,
                                   logit_shift=logit_shift, want_num_fg=False)
        return matches[0]
    import numpy as np
    c = cls.detach().to(torch.float32).contiguous().numpy()
    d = box.detach().to(torch.float32).contiguous().numpy()
    a = anchors.detach().to(torch.float32).contiguous().numpy()
    t = targets.detach().to(torch.float32).contiguous().numpy()
    lab = labels.detach().to(torch.int64).numpy()
    matches = np.full((a.shape[0],), -1, np.int64)
    best = np.full((a.shape[0],), -1.0, np.float32)
    for g in range(t.shape[0]):
        sel, u, _, _ = task_aligned_candidates(c, d, a, t[g], int(lab[g]), topk, alpha, beta, reg_w, logit_shift)
        for i, v in zip(sel, u):
            if v > best[i]:                                  # strict: an equal IoU keeps the lower target index
                best[i], matches[i] = v, g
    return torch.from_numpy(matches)


def matcher(anchors: Tensor, targets: Tensor, match_thr: Optional[float] = None, back_thr: Optional[float] = None) -> Tensor:
    """Match `anchors` [A,4] to `targets` [T,4]: -2 ignore, -1 background, else the
    target index (box_utils.py:51-80), HIP kernel K2 (fused IoU + arg-max + thresholds)."""
    match_thr = ifnone(match_thr, IOU_THRESHOLDS_FOREGROUND)
    back_thr = ifnone(back_thr, IOU_THRESHOLDS_BACKGROUND)
    assert match_thr > back_thr
    targets = targets.reshape(-1, 4)
    off = ops.gt_offsets([targets.shape[0]], anchors.device)
    matches, _ = ops.iou_match(anchors, targets, off, 1, match_thr, back_thr, want_num_fg=False)
    return matches[0]
