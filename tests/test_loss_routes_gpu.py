"""GPU: every route from ``RetinaNetLosses.match_ahead`` / ``forward_levels`` to the kernels gives the bits of the same computation
spelled with the ``ops`` calls directly -- GT packing, matcher, K3, the IoU box loss where selected, the backward scale -- and issues
the launches listed in ``LAUNCHES``, name by name.

Shapes: three levels of 16 x 16, 8 x 8 and 4 x 4 locations with 9 anchors each (2304 + 576 + 144 = 3024 anchors of a 128 x 128 image:
47 full flag words and a ragged one of 16 bits), K = 8 classes, B = 3 images with 4, 0 and 9 GT boxes; the route that the fused kernel
declines has 65, 3 and 0.  The direct computation of a case is run once and shared by the routes that must equal it."""
import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEVELS = [(16, 16, 8), (8, 8, 16), (4, 4, 32)]
SIZES = [2304, 576, 144]
K, B, CAP = 8, 3, 16
S = 1024.0


def _id(matcher, packed, ahead, box_loss, fuse=False, counts=(4, 0, 9), fp16=False):
    return "-".join([matcher, "packed" if packed else "list", "ahead" if ahead else "now", box_loss] + ["fuse"] * fuse
                    + ["x".join(map(str, counts))] * (tuple(counts) != (4, 0, 9)) + ["fp16_prescale"] * fp16)


# (matcher, packed targets, match_ahead's handle, box loss, FUSE_MATCH, GT counts, fp16 under grad_prescale)
ROUTES = [(m, p, a, bl, False, (4, 0, 9), False) for m in ("iou", "atss") for p in (False, True) for a in (True, False) for bl in ("smooth_l1", "giou")]
ROUTES += [("iou", False, False, "smooth_l1", True, (4, 0, 9), False), ("iou", True, False, "smooth_l1", True, (4, 0, 9), False),
           ("iou", False, False, "smooth_l1", True, (65, 3, 0), False),          # more than 64 boxes in an image: the fused form declines, K2 + K3 run
           ("iou", False, False, "smooth_l1", False, (4, 0, 9), True)]

# Launches per timer name (``ops.enable_timing``) of match_ahead + forward_levels, route by route: recorded by running ``_route`` over
# ROUTES on the commit before the handle / marshalling refactor of losses.py and ops.py, and pasted here -- not derived from the code.
LAUNCHES = {
    "iou-list-ahead-smooth_l1": {"gt_pack": 1, "iou_match": 1, "loss_fwd_bwd": 1, "loss_stream_kernel": 1},
    "iou-list-ahead-giou": {"gt_pack": 1, "iou_match": 1, "loss_fwd_bwd": 1, "loss_stream_kernel": 1, "box_iou_loss": 1},
    "iou-list-now-smooth_l1": {"gt_pack": 1, "iou_match": 1, "loss_fwd_bwd": 1, "loss_stream_kernel": 1},
    "iou-list-now-giou": {"gt_pack": 1, "iou_match": 1, "loss_fwd_bwd": 1, "loss_stream_kernel": 1, "box_iou_loss": 1},
    "iou-packed-ahead-smooth_l1": {"iou_match": 1, "loss_fwd_bwd": 1, "loss_stream_kernel": 1},
    "iou-packed-ahead-giou": {"iou_match": 1, "loss_fwd_bwd": 1, "loss_stream_kernel": 1, "box_iou_loss": 1},
    "iou-packed-now-smooth_l1": {"iou_match": 1, "loss_fwd_bwd": 1, "loss_stream_kernel": 1},
    "iou-packed-now-giou": {"iou_match": 1, "loss_fwd_bwd": 1, "loss_stream_kernel": 1, "box_iou_loss": 1},
    "atss-list-ahead-smooth_l1": {"gt_pack": 1, "atss_match": 1, "loss_fwd_bwd": 1, "loss_stream_kernel": 1},
    "atss-list-ahead-giou": {"gt_pack": 1, "atss_match": 1, "loss_fwd_bwd": 1, "loss_stream_kernel": 1, "box_iou_loss": 1},
    "atss-list-now-smooth_l1": {"gt_pack": 1, "atss_match": 1, "loss_fwd_bwd": 1, "loss_stream_kernel": 1},
    "atss-list-now-giou": {"gt_pack": 1, "atss_match": 1, "loss_fwd_bwd": 1, "loss_stream_kernel": 1, "box_iou_loss": 1},
    "atss-packed-ahead-smooth_l1": {"atss_match": 1, "loss_fwd_bwd": 1, "loss_stream_kernel": 1},
    "atss-packed-ahead-giou": {"atss_match": 1, "loss_fwd_bwd": 1, "loss_stream_kernel": 1, "box_iou_loss": 1},
    "atss-packed-now-smooth_l1": {"atss_match": 1, "loss_fwd_bwd": 1, "loss_stream_kernel": 1},
    "atss-packed-now-giou": {"atss_match": 1, "loss_fwd_bwd": 1, "loss_stream_kernel": 1, "box_iou_loss": 1},
    "iou-list-now-smooth_l1-fuse": {"gt_pack": 1, "loss_fwd_bwd": 1, "loss_stream_kernel": 1, "loss_stream_kernel_fused_match": 1},
    "iou-packed-now-smooth_l1-fuse": {"loss_fwd_bwd": 1, "loss_stream_kernel": 1, "loss_stream_kernel_fused_match": 1},
    "iou-list-now-smooth_l1-fuse-65x3x0": {"gt_pack": 1, "iou_match": 1, "loss_fwd_bwd": 1, "loss_stream_kernel": 1},
    "iou-list-now-smooth_l1-fp16_prescale": {"gt_pack": 1, "iou_match": 1, "loss_fwd_bwd": 1, "loss_stream_kernel": 1},
}


def _anchors():
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.anchors import AnchorGenerator
    return ops.anchors_emit(LEVELS, list(AnchorGenerator().to(DEV).cell_anchors)[:len(LEVELS)], 0.0)


_INPUTS = {}


def _inputs(counts, dtype):
    "(anchors, cls levels, box levels, per-image boxes, per-image labels), cached: nothing below writes to them."
    key = (tuple(counts), dtype)
    if key not in _INPUTS:
        rng = np.random.default_rng(17 + sum(counts))
        cls, box = synth.head_outputs(rng, B, sum(SIZES), K)
        gtb, gtl = zip(*[synth.gt_boxes(rng, t, 128, 128, num_classes=K, wh_lo=16.0, wh_hi=100.0) for t in counts])
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        split = lambda t: [c.contiguous() for c in torch.split(t, SIZES, dim=1)]
        _INPUTS[key] = (_anchors(), split(to(cls).to(dtype)), split(to(box).to(dtype)),
                        [to(b.astype(np.float32)).reshape(-1, 4) for b in gtb], [to(l.astype(np.int64)).reshape(-1) for l in gtl])
    return _INPUTS[key]


def _route(route):
    "The route through the module: ((cls loss, reg loss), per-level gradients, launches per timer name)."
    from pytorch_retinanet_amd import losses, ops
    matcher, packed, ahead, box_loss, fuse, counts, fp16 = route
    anc, cls, box, boxes, labels = _inputs(counts, torch.float16 if fp16 else torch.bfloat16)
    old = losses.FUSE_MATCH
    losses.FUSE_MATCH = False                                       # (the switch refuses ATSS / IoU kinds at construction)
    try:
        crit = losses.RetinaNetLosses(K, matcher=matcher, box_loss=box_loss)
        losses.FUSE_MATCH = fuse
        if packed:
            targets = ops.gt_stage(boxes, labels, ops.PackedGT.empty(B, CAP, torch.device(DEV)))
        else:
            targets = [{"boxes": b, "labels": l} for b, l in zip(boxes, labels)]
        cl = [c.clone().requires_grad_() for c in cls]
        bl = [b.clone().requires_grad_() for b in box]
        scale = torch.full((1,), S, device=DEV) if fp16 else None
        ops.enable_timing(True)
        try:
            with losses.grad_prescale(scale):
                handle = crit.match_ahead(targets, [anc] * B, SIZES) if ahead else None
                out = crit.forward_levels(targets, cl, bl, [anc] * B, ahead=handle)
            launches = {name: len(ev) for name, ev in ops.timing_events().items()}
        finally:
            ops.enable_timing(False)
    finally:
        losses.FUSE_MATCH = old
    ((out["classification_loss"] + 2.0 * out["regression_loss"]) * (S if fp16 else 1.0)).backward()
    return (out["classification_loss"].detach(), out["regression_loss"].detach()), [t.grad for t in cl + bl], launches


_DIRECT = {}


def _direct(route):
    "The same computation with the ``ops`` calls themselves (one run per case: the handle and the fused switch do not enter)."
    from pytorch_retinanet_amd import losses, ops
    from pytorch_retinanet_amd.config import IOU_THRESHOLDS_BACKGROUND, IOU_THRESHOLDS_FOREGROUND
    matcher, packed, _, box_loss, _, counts, fp16 = route
    key = (matcher, packed, box_loss, counts, fp16)
    if key in _DIRECT:
        return _DIRECT[key]
    anc, cls, box, boxes, labels = _inputs(counts, torch.float16 if fp16 else torch.bfloat16)
    dev = torch.device(DEV)
    if packed:
        p = ops.gt_stage(boxes, labels, ops.PackedGT.empty(B, CAP, dev))
        gt_boxes, gt_labels, gt_off = p.gt_boxes, p.gt_labels, p.gt_off
    else:
        gt_boxes, gt_labels, gt_off, _ = ops.gt_pack(boxes, labels, dev)
    if matcher == "atss":
        m, nfg, sp = ops.atss_match(anc, gt_boxes, gt_off, B, SIZES, 9, 9, want_special=True, flagged_only=True)
    else:
        m, nfg, sp = ops.iou_match(anc, gt_boxes, gt_off, B, IOU_THRESHOLDS_FOREGROUND, IOU_THRESHOLDS_BACKGROUND, want_special=True, flagged_only=True)
    params = losses.RetinaNetLosses(K)._params()
    pre = torch.full((1,), S, device=DEV) if fp16 else None
    loss, gcls, gbox = ops.loss_fwd_bwd_levels(cls, box, anc, gt_boxes, gt_labels, gt_off, m, nfg, params, True, special=sp,
                                               in_kernel_finalize=losses.IN_KERNEL_FINALIZE, grad_prescale=pre,
                                               form=losses.k3_form(int(gt_boxes.shape[0]), B))
    if box_loss != "smooth_l1":
        ops.box_iou_loss(box, anc, gt_boxes, gt_off, m, nfg, sp, loss, gbox, box_loss, reg_w=tuple(params.reg_w), weight=1.0, grad_prescale=pre)
    up = S if fp16 else 1.0                                         # upstream of (cls + 2 reg) * up, over the pre-scale the gradients already carry
    g0, g1 = torch.full((1,), up, device=DEV), torch.full((1,), 2.0 * up, device=DEV)
    if pre is not None:
        g0, g1 = g0 / pre, g1 / pre
    ops.scale_inplace_batched(list(gcls) + list(gbox), [g0] * len(gcls) + [g1] * len(gbox))
    torch.cuda.synchronize()
    _DIRECT[key] = ((loss[0].clone(), loss[1].clone()), list(gcls) + list(gbox))
    return _DIRECT[key]


@pytest.mark.parametrize("route", ROUTES, ids=[_id(*r) for r in ROUTES])
def test_route_gives_the_direct_calls_bits_and_launches(route):
    got_loss, got_grads, launches = _route(route)
    want_loss, want_grads = _direct(route)
    torch.cuda.synchronize()
    print(_id(*route), launches)
    assert torch.equal(got_loss[0], want_loss[0]) and torch.equal(got_loss[1], want_loss[1]), (got_loss, want_loss)
    assert float(want_loss[0]) > 0 and float(want_loss[1]) > 0
    for i, (g, w) in enumerate(zip(got_grads, want_grads)):
        assert g.dtype == w.dtype and torch.equal(g, w), (i, int((g != w).sum()))
    assert launches == LAUNCHES[_id(*route)]
