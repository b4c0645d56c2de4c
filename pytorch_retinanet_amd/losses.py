"""``RetinaNetLosses`` with the reference's surface (``retinanet/losses.py:11-145``).

``forward`` / ``calc_loss`` run as two HIP launches for the whole batch -- K2
``rn_iou_match`` and K3 ``rn_loss_fwd_bwd`` -- instead of the reference's per-image
Python loop of ~40 torch ops with 4 host syncs each (losses.py:126, :66-97).  K3
writes the gradients in the same pass that computes the loss values, so
``backward`` only has to apply the upstream scalar (a device-side no-op when it
is 1, the ``loss.backward()`` case).
"""
import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from . import ops
from .config import (BBOX_REG_WEIGHTS, ENCODE_LOG_EPS, FOCAL_LOSS_ALPHA, FOCAL_LOSS_GAMMA,
                     IOU_THRESHOLDS_BACKGROUND, IOU_THRESHOLDS_FOREGROUND, LOGIT_SHIFT, SMOOTH_L1_LOSS_BETA)


class _FusedDenseHeadLoss(torch.autograd.Function):
    """(cls [B,A,K], box [B,A,4]) -> f32[2] = (classification_loss, regression_loss)."""

    @staticmethod
    def forward(ctx, cls, box, anchors, gt_boxes, gt_labels, gt_off, params, fg_thr, bg_thr):
        B = cls.shape[0]
        matches, num_fg = ops.iou_match(anchors, gt_boxes, gt_off, B, fg_thr, bg_thr)
        want_grad = bool(ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        loss, gcls, gbox = ops.loss_fwd_bwd(cls, box, anchors, gt_boxes, gt_labels, gt_off, matches, num_fg,
                                            params, want_grad)
        ctx.gcls, ctx.gbox = gcls, gbox
        ctx.box_dtype, ctx.cls_shape, ctx.box_shape = box.dtype, cls.shape, box.shape
        return loss

    @staticmethod
    def backward(ctx, g):
        if ctx.gcls is None:
            raise RuntimeError("fused RetinaNet loss: backward called twice (or without gradients recorded); "
                               "re-run the forward pass instead of retain_graph=True")
        gcls, gbox = ctx.gcls, ctx.gbox
        ctx.gcls = ctx.gbox = None
        g = g.to(torch.float32)
        ops.scale_inplace(gcls, g[0:1])
        ops.scale_inplace(gbox, g[1:2])
        if gbox.dtype != ctx.box_dtype:
            gbox = gbox.to(ctx.box_dtype)
        return gcls.view(ctx.cls_shape), gbox.view(ctx.box_shape), None, None, None, None, None, None, None


class MatchAhead:
    """The one object between ``RetinaNetLosses`` and the loss Function: the anchors, the GT arrays as the library takes them (``B``
    images) and the matcher (``rule``: the ``ops`` call and its arguments behind B), in one of three states --
    launched ahead of the head convolutions on a side stream (``RetinaNetLosses.match_ahead``: the matcher needs only the anchors and
    the GT boxes, so it does not have to sit between the class-output conv and K3): ``matches`` / ``num_fg`` / ``special`` are its
    buffers and ``done`` the event the loss stream waits for;
    to launch on the loss's stream: ``matches`` is None, ``num_fg0`` a zeroed i32 [B] the matcher adds into (None: it clears its own);
    to try INSIDE the loss kernel first (``FUSE_MATCH``): as before, with ``max_gt`` the bound on the boxes per image (else None)."""
    __slots__ = ("anchors", "gt_boxes", "gt_labels", "gt_off", "B", "num_fg0", "max_gt", "rule", "matches", "num_fg", "special", "done")


_SIDE_STREAMS = {}
# K2 inside K3 (rn_loss_match_fwd_bwd_levels) is OPT-IN: bit-identical results, but measured SLOWER than the two launches on MI355X
# (B = 8, A = 201 600, T = 8, isolated: 201 us against 154 us for K2 + K3).  num_fg[b] normalises every gradient of image b, so the
# fused kernel needs a grid barrier between its matching prologue and the stream; ablations on one box: the barrier alone +23 us (it
# exposes the launch ramp of the 1 536 workgroups, which the plain kernel hides under the early workgroups' streaming), the matching
# pass alone +15 us when other waves' streaming covers it and ~45 us when everything waits behind the barrier.
FUSE_MATCH = os.environ.get("RN_FUSE_MATCH", "0") == "1"
# The two batch losses from the streaming kernel itself instead of a one-block finalize launch behind it (rn_loss_fwd_bwd_levels_fin:
# fixed-point partial sums through device-scope atomics, workgroup 0 waits for the last arrival): same bits, one dependent launch less
IN_KERNEL_FINALIZE = True
# How K3 repairs its special rows (``ops.LOSS_FORM_*``, rn_loss_fwd_bwd_levels_rp).  "auto": the chunk form at the train shape, the
# list form from K3_LIST_MIN_GT boxes per image on (same-box A/B on MI355X, round 6, isolated graph replays, one-launch forms: T = 8
# 116.8 us chunks / 119.0 list; T = 64 131.7 / 127.9; T = 500 fp16 149.3 / 143.2).  The two-launch form (a pure background stream + a
# repair kernel over K2's flag words, one special row per lane) is correct and slower -- 145 / 170 / 198 us at T = 8 / 64 / 500: the
# repair's dependent loads have nothing to hide under once they leave the streaming kernel -- and stays for A/B: K3_FORM = 1.
K3_FORM = "auto"
K3_LIST_MIN_GT = 32


def k3_form(total_gt: int, B: int) -> int:
    """The K3 form for ``total_gt`` GT rows over B images.  Packed GT (``ops.PackedGT``, the capture's GT capacity mode) passes its
    row count R = B x capacity class: the host knows no per-image count there, and any form is exact for any count (the form
    only decides how the special rows are repaired) -- the classes 8 / 32 / 128 / 512 of ``graph.GT_CAPACITY_CLASSES`` give the
    chunk form for class 8 and the list form from class 32 on, the rule the measurements above give for images at capacity."""
    if K3_FORM != "auto":
        return int(K3_FORM)
    return ops.LOSS_FORM_LIST if total_gt >= K3_LIST_MIN_GT * max(B, 1) else ops.LOSS_FORM_CHUNKS


# Gradient pre-scale (fp16 training): a device f32 scalar -- a torch.amp.GradScaler's ``_scale`` -- that K3 multiplies into every
# gradient BEFORE rounding it to fp16.  K3 writes d loss / d logits in the forward pass; a background element at the prior has
# 0.25 p^3 / (num_fg B) ~ 4e-10, below fp16's smallest subnormal (6e-8): stored unscaled it is zero whatever backward multiplies in
# later.  The reference's native-AMP run scales the fp32 loss first and keeps them (~2.6e-5 at a scale of 65 536).  backward then
# multiplies by upstream / prescale (exactly 1 under ``scaler.scale(loss).backward()``).
class grad_prescale(ops._Override):
    "``with grad_prescale(scaler_scale_tensor):`` -- fused loss calls inside the block pre-scale their gradients by it."


def scaler_prescale(scaler, dev) -> Optional[Tensor]:
    "The device scalar of a ``torch.amp.GradScaler`` (created on first use), or None when there is no enabled scaler."
    if scaler is None or not scaler.is_enabled():
        return None
    if getattr(scaler, "_scale", None) is None:
        scaler._lazy_init_scale_growth_tracker(torch.device(dev))
    return scaler._scale


def _side_stream(dev: torch.device) -> "torch.cuda.Stream":
    s = _SIDE_STREAMS.get(dev.index)
    if s is None:
        s = _SIDE_STREAMS[dev.index] = torch.cuda.Stream(device=dev)
    return s


class _FusedDenseHeadLossLevels(torch.autograd.Function):
    """Per-level head outputs (cls_0..cls_{L-1}, box_0..box_{L-1}) -> f32[2]; no concatenation."""

    @staticmethod
    def forward(ctx, h, params, L, box_loss, *levels):
        """``h``: the ``MatchAhead`` of the batch.  ``box_loss``: None (K3's smooth-L1 as it is) or (kind, weight): ``ops.box_iou_loss``
        then runs right behind K3, on the same stream and with the same gradient pre-scale, and replaces the regression loss and the
        matched rows' box gradients.  ``levels``: the L class and the L box outputs, optionally followed by ONE more argument, the
        class loss: None (K3's focal loss as it is) or ("qfl", beta) -- ``params`` then carries ``alpha = 1, gamma = beta`` and
        ``ops.quality_focal_loss`` runs behind K3 (and behind ``ops.box_iou_loss``) the same way, adding the matched label elements'
        soft-target terms to the classification loss and storing their gradients."""
        cls_levels, box_levels = levels[:L], levels[L:2 * L]
        cls_loss = levels[2 * L] if len(levels) > 2 * L else None
        ctx.extra = len(levels) - 2 * L
        if cls_loss is not None and h.matches is None and h.max_gt is not None:
            raise ValueError('cls_loss="qfl" reads the matcher\'s buffers and cannot run behind the fused match-and-loss kernel')
        dev = cls_levels[0].device
        want_grad = any(ctx.needs_input_grad[4:4 + 2 * L])
        fused = None
        if h.matches is None and h.max_gt is not None:
            # K2 runs INSIDE the loss kernel (one launch; box_utils.py:51-80 in the prologue of rn_loss_match_fwd_bwd_levels) unless
            # the library declines the shape
            fused = ops.loss_match_fwd_bwd_levels(cls_levels, box_levels, h.anchors, h.gt_boxes, h.gt_labels, h.gt_off, h.max_gt,
                                                  *h.rule[1:], params, want_grad)
        ctx.prescale = None
        if fused is not None:
            loss, gcls, gbox = fused[0], fused[1], fused[2]
        else:
            if h.matches is None:
                # (the "tal" rule is launched HERE whatever the caller did: it reads the outputs that have just arrived -- as
                # constants: a Function's forward records nothing -- and runs right in front of K3 on K3's stream)
                _launch_matcher(h, heads=(cls_levels, box_levels, params))
            elif h.done is not None:
                torch.cuda.current_stream(dev).wait_event(h.done)    # the matcher ran beside the head convolutions
            pre = grad_prescale.value
            if not (want_grad and pre is not None and pre.device == dev):
                pre = None
            loss, gcls, gbox = ops.loss_fwd_bwd_levels(cls_levels, box_levels, h.anchors, h.gt_boxes, h.gt_labels, h.gt_off, h.matches,
                                                       h.num_fg, params, want_grad, special=h.special, in_kernel_finalize=IN_KERNEL_FINALIZE,
                                                       grad_prescale=pre, form=k3_form(int(h.gt_boxes.shape[0]), h.B))
            ctx.prescale = pre
            if box_loss is not None:
                ops.box_iou_loss(box_levels, h.anchors, h.gt_boxes, h.gt_off, h.matches, h.num_fg, h.special, loss, gbox, box_loss[0],
                                 reg_w=tuple(params.reg_w), weight=box_loss[1], grad_prescale=pre)
            if cls_loss is not None:
                ops.quality_focal_loss(cls_levels, box_levels, h.anchors, h.gt_boxes, h.gt_labels, h.gt_off, h.matches, h.num_fg, h.special,
                                       loss, gcls, beta=cls_loss[1], reg_w=tuple(params.reg_w), logit_shift=params.logit_shift,
                                       grad_prescale=pre)
        ctx.grads = (gcls, gbox)
        ctx.meta = [(c.shape, c.dtype) for c in cls_levels] + [(b.shape, b.dtype) for b in box_levels]
        # two scalar outputs (views of the kernel's f32[2]): backward then receives the two upstream scalars directly, without
        # autograd's select-backward zeros / copies / add in front of the first gradient kernel
        return loss[0], loss[1]

    @staticmethod
    def backward(ctx, g0, g1):
        if ctx.grads is None or ctx.grads[0] is None:
            raise RuntimeError("fused RetinaNet loss: backward called twice (or without gradients recorded); "
                               "re-run the forward pass instead of retain_graph=True")
        gcls, gbox = ctx.grads
        ctx.grads = None
        dev = gcls[0].device
        g0 = torch.full((1,), 0.0, device=dev) if g0 is None else g0.reshape(1)
        g1 = torch.full((1,), 0.0, device=dev) if g1 is None else g1.reshape(1)
        pre = getattr(ctx, "prescale", None)
        if pre is not None:                 # the gradients already carry the pre-scale: what is left is upstream / prescale (1 under a GradScaler)
            g0, g1 = g0.float() / pre.reshape(1), g1.float() / pre.reshape(1)
        ops.scale_inplace_batched(list(gcls) + list(gbox), [g0] * len(gcls) + [g1] * len(gbox))      # one launch
        outs = [t.view(shape) if t.dtype == dt else t.to(dt).view(shape) for t, (shape, dt) in zip(list(gcls) + list(gbox), ctx.meta)]
        return (None,) * 4 + tuple(outs) + (None,) * ctx.extra


def _resolve_gt(targets, dev: Optional[torch.device]):
    """Targets -- the reference's list of dicts or an ``ops.PackedGT`` -- as (gt_boxes, gt_labels, gt_off, zeroed num_fg or None, B,
    bound on the GT boxes per image).  A list is packed by ``ops.gt_pack`` on ``dev`` (one launch; ``dev`` None: the two host figures
    only, the arrays None).  Packed GT: the staged arrays as they are, ``gt_stage``'s zeroed ``num_fg``, and every host-side figure an
    upper bound -- K2's kernel choice and K3's form (``k3_form``) see the R rows, the bound is the capacity per image; the kernels read
    each image's range from ``gt_off``."""
    if isinstance(targets, ops.PackedGT):
        return targets.gt_boxes, targets.gt_labels, targets.gt_off, targets.num_fg, targets.B, targets.cap_per_image
    boxes = [t["boxes"] for t in targets]
    arrays = (None,) * 4 if dev is None else ops.gt_pack(boxes, [t["labels"] for t in targets], dev)
    return arrays + (len(boxes), max([b.numel() // 4 for b in boxes] or [0]))


def _launch_matcher(h: MatchAhead, out: Optional[tuple] = None, heads: Optional[tuple] = None) -> None:
    """The matcher of ``h.rule`` on the CURRENT stream, into ``h.matches`` / ``h.num_fg`` / ``h.special``.  ``out``: buffers the caller
    allocated (``match_ahead``: they belong to its main stream), written in full.  Without it fresh ones, and ``matches`` written at the
    flagged rows only: it goes nowhere but into the loss kernel, which reads it through the flag words.  ``heads``: (cls_levels,
    box_levels, params) -- what the "tal" rule reads beside the anchors and the GT, so it can only be launched where they exist."""
    kw = dict(want_special=True, flagged_only=True) if out is None else dict(out=out)
    if h.rule[0] == "tal":
        if heads is None:
            raise ValueError('matcher="tal" reads the head\'s outputs and cannot be launched ahead of them')
        sizes, cells, topk, alpha, beta, level_w = h.rule[1:]
        h.matches, h.num_fg, h.special = ops.tal_match(heads[0], heads[1], h.anchors, h.gt_boxes, h.gt_labels, h.gt_off, h.B, sizes, cells,
                                                       topk, alpha, beta, reg_w=tuple(heads[2].reg_w), logit_shift=heads[2].logit_shift,
                                                       zeroed_num_fg=h.num_fg0, level_w=level_w, **kw)
        return
    match = ops.atss_match if h.rule[0] == "atss" else ops.iou_match
    h.matches, h.num_fg, h.special = match(h.anchors, h.gt_boxes, h.gt_off, h.B, *h.rule[1:], zeroed_num_fg=h.num_fg0, **kw)


def _stack_anchors(anchors) -> Tensor:
    """List of per-image [A,4] tensors -> one shared [A,4] (the usual case: the
    generator hands out the same cached tensor per image) or a stacked [B,A,4]."""
    if isinstance(anchors, Tensor):
        return anchors
    first = anchors[0]
    if all(a is first or a.data_ptr() == first.data_ptr() for a in anchors):
        return first
    return torch.stack(list(anchors))


def _check_matcher(matcher: str, atss_topk: int, tal: tuple = (13, 1, 6)) -> None:
    if matcher not in ops.MATCHERS:
        raise ValueError(f"matcher must be one of {ops.MATCHERS}, got {matcher!r}")
    if int(atss_topk) <= 0:
        raise ValueError(f"atss_topk must be a positive int, got {atss_topk!r}")
    ops.tal_topk(tal[0]), ops.tal_exponent(tal[1], "tal_alpha"), ops.tal_exponent(tal[2], "tal_beta")
    if matcher == "tal" and FUSE_MATCH:
        raise ValueError('RN_FUSE_MATCH=1 runs the max-IoU matcher inside the loss kernel and cannot be combined with matcher="tal": '
                         "the task-aligned matcher reads the head\'s outputs and fills the matcher\'s buffers; unset RN_FUSE_MATCH or use "
                         'matcher="iou"')
    if matcher == "atss" and FUSE_MATCH:
        raise ValueError('RN_FUSE_MATCH=1 runs the max-IoU matcher inside the loss kernel and cannot be combined with matcher="atss": '
                         "there is no ATSS form of the fused kernel; unset RN_FUSE_MATCH or use matcher=\"iou\"")


def _check_box_loss(box_loss: str, box_loss_weight: float) -> None:
    if box_loss not in ops.BOX_LOSSES:
        raise ValueError(f"box_loss must be one of {ops.BOX_LOSSES}, got {box_loss!r}")
    if not float(box_loss_weight) > 0.0:
        raise ValueError(f"box_loss_weight must be positive, got {box_loss_weight!r}")
    if box_loss != "smooth_l1" and FUSE_MATCH:
        raise ValueError(f'RN_FUSE_MATCH=1 keeps the match codes inside the loss kernel and cannot be combined with box_loss="{box_loss}": '
                         'the IoU box losses read the matcher\'s buffers; unset RN_FUSE_MATCH or use box_loss="smooth_l1"')


def _check_cls_loss(cls_loss: str, qfl_beta: float) -> None:
    if cls_loss not in ops.CLS_LOSSES:
        raise ValueError(f"cls_loss must be one of {ops.CLS_LOSSES}, got {cls_loss!r}")
    if not (float(qfl_beta) >= 0.0 and float(qfl_beta) < float("inf")):
        raise ValueError(f"qfl_beta must be finite and >= 0, got {qfl_beta!r}")
    if cls_loss != "focal" and FUSE_MATCH:
        raise ValueError(f'RN_FUSE_MATCH=1 keeps the match codes inside the loss kernel and cannot be combined with cls_loss="{cls_loss}": '
                         'Quality Focal Loss reads the matcher\'s buffers; unset RN_FUSE_MATCH or use cls_loss="focal"')


def _decode_iou(deltas: Tensor, anchors: Tensor, gt: Tensor, reg_w: Sequence[float]):
    """Steps 1 and 2 of ``rn_box_iou_loss``'s rule in ``deltas``' dtype, ONE copy for ``box_iou_loss_reference`` and
    ``box_quality_reference``: ((cx, cy), the decoded box (px1, py1, px2, py2), the GT coordinates, union, iou)."""
    dt = deltas.dtype
    an, g = anchors.to(dt), gt.to(dt)
    t = deltas / torch.tensor([float(v) for v in reg_w], dtype=dt, device=deltas.device)
    acx, acy, aw, ah = (an[:, 0] + an[:, 2]) / 2, (an[:, 1] + an[:, 3]) / 2, an[:, 2] - an[:, 0], an[:, 3] - an[:, 1]
    cx, cy = aw * t[:, 0] + acx, ah * t[:, 1] + acy
    clip = torch.full_like(t[:, 2], ops.BOX_XFORM_CLIP)
    sw, sh = torch.where(t[:, 2] > clip, clip, t[:, 2]), torch.where(t[:, 3] > clip, clip, t[:, 3])
    w, h = aw * torch.exp(sw), ah * torch.exp(sh)
    px1, py1, px2, py2 = cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2
    gx1, gy1, gx2, gy2 = g[:, 0], g[:, 1], g[:, 2], g[:, 3]
    zero = torch.zeros_like(px1)
    iw = torch.where(px2 < gx2, px2, gx2) - torch.where(px1 > gx1, px1, gx1)
    ih = torch.where(py2 < gy2, py2, gy2) - torch.where(py1 > gy1, py1, gy1)
    iw, ih = torch.where(iw > 0, iw, zero), torch.where(ih > 0, ih, zero)
    inter = iw * ih
    union = (w * h + (gx2 - gx1) * (gy2 - gy1)) - inter
    iou = torch.where(union > 0, inter / torch.where(union > 0, union, torch.ones_like(union)), zero)
    return (cx, cy), (px1, py1, px2, py2), (gx1, gy1, gx2, gy2), union, iou


def box_quality_reference(deltas: Tensor, anchors: Tensor, gt: Tensor, reg_w: Sequence[float] = BBOX_REG_WEIGHTS) -> Tensor:
    """Step 1 of ``rn_quality_focal_loss``'s rule (include/retinanet_hip.h) in ``deltas``' dtype: the quality q [N] of N matched rows,
    the IoU of the standard-decoded box with the GT box -- steps 1 and 2 of ``box_iou_loss_reference``, the same code.  Detached: the
    quality is a constant of the class loss, no gradient reaches the deltas through it."""
    return _decode_iou(deltas, anchors, gt, reg_w)[4].detach()


def quality_focal_loss_reference(logits: Tensor, quality: Tensor, beta: float = 2.0, logit_shift: float = LOGIT_SHIFT) -> Tensor:
    """Steps 2 and 3 of ``rn_quality_focal_loss``'s rule as differentiable torch code in ``logits``' dtype: the losses l [N] of N label
    elements ``logits`` [N] against their qualities ``quality`` [N] in [0, 1].  z = x + logit_shift; sigma from e = exp(-|z|) as the
    kernel forms it; l = w * bce with bce = (max(z, 0) - q z) + log1p(e) and w = |sigma - q|^beta DETACHED (the library's quirk Q3;
    mmdet differentiates through it), so autograd gives dl / dx = w * (sigma - q).  The per-image scale and the sum (steps 3-4)
    are the caller's."""
    q = quality.detach().to(logits.dtype)
    z = logits + logit_shift
    e = torch.exp(-z.abs())
    r = 1 / (1 + e)
    sigma = torch.where(z >= 0, r, e * r)
    bce = (torch.clamp(z, min=0) - q * z) + torch.log1p(e)
    d = (sigma - q).detach()
    w = d * d if beta == 2 else (torch.ones_like(d) if beta == 0 else d.abs().pow(beta))
    return w * bce


def box_iou_loss_reference(deltas: Tensor, anchors: Tensor, gt: Tensor, kind: str, reg_w: Sequence[float] = BBOX_REG_WEIGHTS) -> Tensor:
    """The rule of ``rn_box_iou_loss`` (include/retinanet_hip.h, steps 1-3) as differentiable torch code in ``deltas``' dtype: the row
    losses l [N] of N matched rows -- ``deltas`` [N,4] the head's outputs, ``anchors`` / ``gt`` [N,4] each row's anchor and GT box.
    Autograd through it is the gradient of step 4: every min / max is a ``torch.where`` on the strict comparison that selects the
    predicted coordinate, so a tie goes to the GT coordinate and carries no derivative; a slot above the clip has zero gradient.
    The per-image scale, the weight and the sum (steps 4-5) are the caller's."""
    if kind not in ops.BOX_LOSS_KINDS:
        raise ValueError(f"kind must be one of {tuple(ops.BOX_LOSS_KINDS)}, got {kind!r}")
    (cx, cy), (px1, py1, px2, py2), (gx1, gy1, gx2, gy2), union, iou = _decode_iou(deltas, anchors, gt, reg_w)
    zero = torch.zeros_like(px1)
    ew = torch.where(px2 > gx2, px2, gx2) - torch.where(px1 < gx1, px1, gx1)
    eh = torch.where(py2 > gy2, py2, gy2) - torch.where(py1 < gy1, py1, gy1)
    if kind == "giou":
        c = ew * eh
        pen = torch.where(c > 0, (c - union) / torch.where(c > 0, c, torch.ones_like(c)), zero)
    else:
        c2 = ew * ew + eh * eh
        dx, dy = cx - (gx1 + gx2) / 2, cy - (gy1 + gy2) / 2
        pen = torch.where(c2 > 0, (dx * dx + dy * dy) / torch.where(c2 > 0, c2, torch.ones_like(c2)), zero)
    return (1 - iou) + pen


class RetinaNetLosses(nn.Module):
    def __init__(self, num_classes: int, matcher: str = "iou", atss_topk: int = 9, cells=None, box_loss: str = "smooth_l1",
                 box_loss_weight: float = 1.0, cls_loss: str = "focal", qfl_beta: float = 2.0, tal_topk: int = 13, tal_alpha: int = 1,
                 tal_beta: int = 6) -> None:
        """``matcher``: "iou" (K2: the reference's max-IoU rule with its 0.5 / 0.4 thresholds) or "atss" (``ops.atss_match``: a
        per-object threshold from the IoU statistics of the ``atss_topk`` nearest locations of every pyramid level; no ignored band).
        ATSS applies to the per-level path (``forward_levels`` / ``match_ahead``, what ``Retinanet.forward`` runs; ``forward`` /
        ``calc_loss`` on concatenated outputs raise a ``ValueError`` with it); ``cells``: anchors
        per grid location (an int or one per level; ``Retinanet`` passes its anchor generator's), default 9.
        ``box_loss``: "smooth_l1" (the reference's encode-then-smooth-L1 inside K3; no further launch) or "giou" / "diou"
        (``ops.box_iou_loss`` behind K3: the loss of the decoded box against its GT box, times ``box_loss_weight``).  Like ATSS the IoU
        kinds apply to the per-level path and refuse ``RN_FUSE_MATCH=1``.  Inference is not affected by this argument: what decodes the
        detections is ``Retinanet(box_decode=...)``, whose "standard" kind is the decode these losses train.
        ``cls_loss``: "focal" (the reference's sigmoid focal loss against a 0 / 1 target inside K3; no further launch) or "qfl"
        (Quality Focal Loss, Li et al., NeurIPS 2020: K3 runs with ``alpha = 1, gamma = qfl_beta`` and ``ops.quality_focal_loss`` behind
        it gives every matched row's label element the IoU of its decoded box with its GT box as target; the weight stays detached
        and the normaliser ``num_fg``, see include/retinanet_hip.h).  Per-level path only, refuses ``RN_FUSE_MATCH=1``; composes with
        both matchers and all three box losses.  CPU tensors with "qfl" go through the torch restatement (``matcher="atss"`` only:
        the max-IoU matcher has no CPU form).
        ``matcher="tal"`` (``ops.tal_match``, TOOD's task-aligned assignment): per object the ``tal_topk`` anchors with the largest
        ``score^tal_alpha * IoU^tal_beta`` among those whose centre lies inside its box, the score and the IoU being what the head
        predicts NOW (read as constants; integer exponents in 0..8, the metric is a chain of fp32 products).  It needs the head's
        outputs, so it never runs ahead of the head: ``match_ahead`` only records the rule and the launch happens in
        ``forward_levels``, right in front of K3 on the same stream.  Per-level path only, refuses ``RN_FUSE_MATCH=1``; composes with
        every box and class loss.  ``matcher`` is a plain attribute read at every call: TOOD's schedule "ATSS for the first
        epochs, then TAL" is ``losses.matcher = "tal"`` between two epochs (a captured step re-captures once: the matcher is part
        of its key)."""
        super().__init__()
        _check_matcher(matcher, atss_topk, (tal_topk, tal_alpha, tal_beta))
        self.tal_topk, self.tal_alpha, self.tal_beta = int(tal_topk), int(tal_alpha), int(tal_beta)
        _check_box_loss(box_loss, box_loss_weight)
        _check_cls_loss(cls_loss, qfl_beta)
        self.cls_loss, self.qfl_beta = cls_loss, float(qfl_beta)
        self.box_loss, self.box_loss_weight = box_loss, float(box_loss_weight)
        self.matcher, self.atss_topk = matcher, int(atss_topk)
        self.cells = 9 if cells is None else cells
        self.n_c = num_classes
        self.alpha = FOCAL_LOSS_ALPHA
        self.gamma = FOCAL_LOSS_GAMMA
        self.beta = SMOOTH_L1_LOSS_BETA

    # -- stand-alone helpers (surface parity; the fused kernel does not call them) ----
    def smooth_l1_loss(self, input: Tensor, target: Tensor) -> Tensor:
        "Summed smooth-L1 with threshold `beta` (losses.py:19-27)."
        n = torch.abs(input - target)
        if self.beta < 1e-5:
            return n.sum()
        return torch.where(n < self.beta, 0.5 * n ** 2 / self.beta, n - 0.5 * self.beta).sum()

    def focal_loss(self, clas_pred: Tensor, clas_tgt: Tensor) -> Tensor:
        """Summed focal loss of logits vs {0,1} targets exactly as the reference
        defines it (losses.py:29-47): constant (detached) modulating weight, and
        alpha applied to the NEGATIVES' complement (positives get 1 - alpha)."""
        p = torch.sigmoid(clas_pred.detach())
        w = clas_tgt * (1 - p) + (1 - clas_tgt) * p
        a = (1 - clas_tgt) * self.alpha + clas_tgt * (1 - self.alpha)
        w = w.pow(self.gamma).mul(a)
        return F.binary_cross_entropy_with_logits(clas_pred, clas_tgt, w, reduction="sum")

    # -- fused path ----------------------------------------------------------------------
    def _params(self):
        if self.cls_loss == "qfl":
            # K3 as QFL's negative term: alpha = 1 weighs every background element sigma^beta * BCE(sigma, 0) and every matched label
            # element 1 - alpha = 0 (the contract rn_quality_focal_loss rests on)
            return ops.make_loss_params(1.0, self.qfl_beta, self.beta, LOGIT_SHIFT, ENCODE_LOG_EPS, BBOX_REG_WEIGHTS)
        return ops.make_loss_params(self.alpha, self.gamma, self.beta, LOGIT_SHIFT, ENCODE_LOG_EPS, BBOX_REG_WEIGHTS)

    def _fused(self, cls: Tensor, box: Tensor, anchors, boxes: Sequence[Tensor], labels: Sequence[Tensor]) -> Tensor:
        if self.matcher in ("atss", "tal"):
            # (the concatenated outputs carry no level layout, and matching them with K2 instead would be a silent change of rule)
            raise ValueError(f'matcher="{self.matcher}" runs on the per-level head outputs: use forward_levels / Retinanet.forward, not forward / calc_loss')
        if self.box_loss != "smooth_l1":
            # (the concatenated path has no flag words, and answering with smooth-L1 instead would be a silent change of loss)
            raise ValueError(f'box_loss="{self.box_loss}" runs on the per-level head outputs: use forward_levels / Retinanet.forward, not forward / calc_loss')
        if self.cls_loss != "focal":
            # (the concatenated path has no flag words, and answering with the focal loss instead would be a silent change of loss)
            raise ValueError(f'cls_loss="{self.cls_loss}" runs on the per-level head outputs: use forward_levels / Retinanet.forward, not forward / calc_loss')
        dev = cls.device
        counts = [int(b.reshape(-1, 4).shape[0]) for b in boxes]
        gt_boxes = torch.cat([b.reshape(-1, 4).to(device=dev, dtype=torch.float32) for b in boxes]) \
            if counts else torch.zeros((0, 4), device=dev)
        gt_labels = torch.cat([l.reshape(-1).to(device=dev, dtype=torch.int64) for l in labels]) \
            if counts else torch.zeros((0,), dtype=torch.int64, device=dev)
        gt_off = ops.gt_offsets(counts, dev)
        return _FusedDenseHeadLoss.apply(cls, box, _stack_anchors(anchors), gt_boxes, gt_labels, gt_off,
                                         self._params(), IOU_THRESHOLDS_FOREGROUND, IOU_THRESHOLDS_BACKGROUND)

    @staticmethod
    def fuses_match(targets) -> bool:
        """``RN_FUSE_MATCH=1``: the matcher runs inside the loss kernel (one launch, ``rn_loss_match_fwd_bwd_levels``) when no image has
        more than 64 GT boxes (packed GT: when its capacity per image is at most 64).  Off by default: measured slower than K2 + K3
        (see ``FUSE_MATCH``)."""
        return FUSE_MATCH and _resolve_gt(targets, None)[5] <= 64

    def _handle(self, targets, anchors, level_sizes, level_w=None) -> MatchAhead:
        """The handle of these targets and anchors: the GT resolved (``_resolve_gt``), the matcher named, nothing of it launched.
        ``level_sizes`` (anchors per pyramid level) is what ``matcher="atss"`` needs beside them; ``ops.atss_match`` checks its sum."""
        _check_matcher(self.matcher, self.atss_topk, (self.tal_topk, self.tal_alpha, self.tal_beta))   # (RN_FUSE_MATCH may have been switched on after construction)
        h = MatchAhead()
        if self.matcher == "tal":
            if level_sizes is None:
                raise ValueError('matcher="tal" needs the anchors per pyramid level (level_sizes)')
            h.rule = ("tal", list(level_sizes), self.cells, self.tal_topk, self.tal_alpha, self.tal_beta, None if level_w is None else list(level_w))
        elif self.matcher == "atss":
            if level_sizes is None:
                raise ValueError('matcher="atss" needs the anchors per pyramid level (level_sizes)')
            h.rule = ("atss", list(level_sizes), self.cells, self.atss_topk)
        else:
            h.rule = ("iou", IOU_THRESHOLDS_FOREGROUND, IOU_THRESHOLDS_BACKGROUND)
        h.anchors = _stack_anchors(anchors)
        h.gt_boxes, h.gt_labels, h.gt_off, h.num_fg0, h.B, h.max_gt = _resolve_gt(targets, h.anchors.device)
        h.matches = h.num_fg = h.special = h.done = None
        return h

    def match_ahead(self, targets: List[Dict[str, Tensor]], anchors, level_sizes=None, level_w=None) -> MatchAhead:
        """Launch K2 (IoU + matcher, box_utils.py:51-80) NOW, on a side stream: it depends only on the anchors and the GT boxes,
        both known as soon as the feature-map shapes are, and then runs beside the head convolutions instead of between the
        class-output conv and K3.  Pass the result to ``forward_levels(..., ahead=...)``, which makes the loss kernel wait
        for it.  The outputs belong to the CALLING stream (allocated before the fork, consumed after the join).
        ``matcher="atss"``: the same with ``ops.atss_match``; ``level_sizes`` (anchors per pyramid level) is needed then.
        ``matcher="tal"``: nothing is launched -- the rule reads the head's outputs -- and the handle only RECORDS the rule, with
        ``level_w`` (grid columns per level, optional: the kernel then visits only the cells under each box); ``forward_levels``
        launches it when the outputs arrive."""
        h = self._handle(targets, anchors, level_sizes, level_w)
        dev = h.anchors.device
        h.max_gt = None
        if h.rule[0] == "tal":
            return h
        if not isinstance(targets, ops.PackedGT):
            h.num_fg0 = None        # (only gt_stage's zeroed num_fg is used here; with a list the matcher clears its own)
        out = ops.iou_match_outputs(h.B, int(h.anchors.shape[-2]), dev, want_num_fg=h.num_fg0 is None)
        main, side = torch.cuda.current_stream(dev), _side_stream(dev)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            _launch_matcher(h, out)
            h.done = torch.cuda.Event()
            h.done.record(side)
        # the tensors were allocated on the calling stream but are written / read on the side stream: if the head raises before
        # the loss joins the streams and the handle is dropped, the allocator must not hand the blocks out while K2 still runs
        for t in (h.matches, h.num_fg, h.special, h.gt_boxes, h.gt_off, h.anchors):
            t.record_stream(side)
        return h

    def forward_levels(self, targets: List[Dict[str, Tensor]], cls_levels: Sequence[Tensor], box_levels: Sequence[Tensor],
                       anchors, ahead: Optional[MatchAhead] = None) -> Dict[str, Tensor]:
        """Same result as ``forward`` on ``torch.cat(levels, dim=1)``, without materialising the cat
        (the loss kernel reads the per-level conv outputs where they are).  ``ahead``: ``match_ahead``'s
        handle for these targets / anchors (K2 already in flight on a side stream).  ``targets`` may be an ``ops.PackedGT``
        (``ops.gt_stage``'s buffers; one loss call per staging: K2 adds into its zeroed ``num_fg``)."""
        box_loss = None
        if self.box_loss != "smooth_l1":
            _check_box_loss(self.box_loss, self.box_loss_weight)
            box_loss = (self.box_loss, self.box_loss_weight)
        extra = ()
        if self.matcher == "tal" and not cls_levels[0].is_cuda and isinstance(targets, ops.PackedGT):
            raise ValueError('matcher="tal" on CPU tensors takes the list of target dicts: packed GT (ops.PackedGT) lives on the device')
        if self.cls_loss != "focal":
            _check_cls_loss(self.cls_loss, self.qfl_beta)
            if not cls_levels[0].is_cuda:
                return self._qfl_torch(targets, cls_levels, box_levels, anchors)
            extra = ((self.cls_loss, self.qfl_beta),)
        h = ahead
        if h is None:
            # the matcher runs on this stream, from the Function (the level sizes: the per-level head outputs'); with RN_FUSE_MATCH it
            # is tried inside the loss kernel first, and K2 clears its own num_fg if the library declines
            h = self._handle(targets, anchors, [int(c.shape[1]) for c in cls_levels])
            if cls_levels[0].is_cuda and FUSE_MATCH and h.max_gt <= 64:
                h.num_fg0 = None
            else:
                h.max_gt = None
        if h.B != int(cls_levels[0].shape[0]):       # (the kernels read gt_off[0 .. B] of the head outputs' B)
            raise ValueError(f"targets (packed GT or a list) of {h.B} images for a batch of {int(cls_levels[0].shape[0])}")
        out = _FusedDenseHeadLossLevels.apply(h, self._params(), len(cls_levels), box_loss, *cls_levels, *box_levels, *extra)
        return {"classification_loss": out[0], "regression_loss": out[1]}

    def _qfl_torch(self, targets, cls_levels: Sequence[Tensor], box_levels: Sequence[Tensor], anchors) -> Dict[str, Tensor]:
        """``cls_loss="qfl"`` on CPU tensors, in plain differentiable torch from the restatements: what K3 (``alpha = 1,
        gamma = qfl_beta``), ``ops.box_iou_loss`` and ``ops.quality_focal_loss`` compute on the device, in the outputs' dtype.  The
        matcher is ``box_utils.atss_matcher``'s / ``box_utils.task_aligned_matcher``'s CPU restatement; the max-IoU matcher has none, so ``matcher="iou"`` is refused here."""
        from .box_utils import atss_matcher, bbox_2_activ, task_aligned_matcher
        if self.matcher not in ("atss", "tal"):
            raise ValueError('cls_loss="qfl" on CPU tensors needs matcher="atss" or "tal": the max-IoU matcher runs on the device only')
        if isinstance(targets, ops.PackedGT):
            raise TypeError("packed GT (ops.PackedGT) lives on the device")
        cls, box = torch.cat(list(cls_levels), 1), torch.cat(list(box_levels), 1)
        anc = _stack_anchors(anchors)
        sizes, B, dt = [int(c.shape[1]) for c in cls_levels], int(cls.shape[0]), cls.dtype
        if len(targets) != B:
            raise ValueError(f"targets of {len(targets)} images for a batch of {B}")
        cls_total, reg_total = cls.new_zeros(()), cls.new_zeros(())
        for b, t in enumerate(targets):
            an = anc if anc.dim() == 2 else anc[b]
            gt = t["boxes"].reshape(-1, 4).to(torch.float32)
            if not gt.shape[0]:
                m = torch.full((an.shape[0],), -1, dtype=torch.int64)
            elif self.matcher == "tal":
                m = task_aligned_matcher(cls[b].detach(), box[b].detach(), an, gt, t["labels"], self.tal_topk, self.tal_alpha, self.tal_beta,
                                         BBOX_REG_WEIGHTS, LOGIT_SHIFT)
            else:
                m = atss_matcher(an, gt, sizes, self.cells, self.atss_topk)
            rows = (m >= 0).nonzero().flatten()
            scale = 1.0 / max(int(rows.numel()), 1)
            z = cls[b] + LOGIT_SHIFT
            neg = torch.sigmoid(z.detach()).pow(self.qfl_beta) * F.softplus(z)          # sigma^beta * BCE(sigma, 0), the weight detached
            if rows.numel():
                g, d = gt[m[rows]], box[b, rows]
                c = t["labels"].reshape(-1).to(torch.int64)[m[rows]] - 1
                keep = torch.ones_like(neg, dtype=torch.bool)
                keep[rows, c] = False                                                    # the label elements: K3's weight there is 0
                q = box_quality_reference(d, an[rows], g, BBOX_REG_WEIGHTS)
                pos = quality_focal_loss_reference(cls[b, rows, c], q, self.qfl_beta, LOGIT_SHIFT)
                cls_total = cls_total + ((neg * keep).sum() + pos.sum()) * scale
                if self.box_loss == "smooth_l1":
                    reg = self.smooth_l1_loss(d, bbox_2_activ(g.to(dt), an[rows].to(dt)))
                else:
                    reg = box_iou_loss_reference(d, an[rows], g, self.box_loss, BBOX_REG_WEIGHTS).sum() * self.box_loss_weight
                reg_total = reg_total + reg * scale
            else:
                cls_total = cls_total + neg.sum() * scale
        return {"classification_loss": cls_total / B, "regression_loss": reg_total / B}

    def calc_loss(self, anchors: Tensor, clas_pred: Tensor, bbox_pred: Tensor, clas_tgt: Tensor,
                  bbox_tgt: Tensor) -> Tuple[Tensor, Tensor]:
        "One image: returns (bb_loss, clas_loss), each already / clamp(num_fg, 1) (losses.py:49-111)."
        out = self._fused(clas_pred[None], bbox_pred[None], anchors, [bbox_tgt], [clas_tgt])
        return out[1], out[0]

    def forward(self, targets: List[Dict[str, Tensor]], head_outputs: Dict[str, Tensor],
                anchors: List[Tensor]) -> Dict[str, Tensor]:
        "Batch means of the per-image normalised losses (losses.py:113-145)."
        if isinstance(targets, ops.PackedGT):
            raise TypeError("RetinaNetLosses.forward / compute_loss take the reference's list of target dicts; packed GT (ops.PackedGT) "
                            "goes through Retinanet.forward or RetinaNetLosses.forward_levels")
        clas_preds, bbox_preds = head_outputs["cls_preds"], head_outputs["bbox_preds"]
        if len(targets) != clas_preds.shape[0]:
            raise ValueError(f"{len(targets)} targets for a batch of {clas_preds.shape[0]}")
        out = self._fused(clas_preds, bbox_preds, anchors, [t["boxes"] for t in targets], [t["labels"] for t in targets])
        return {"classification_loss": out[0], "regression_loss": out[1]}
