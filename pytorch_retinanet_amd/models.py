"""``Retinanet`` -- the detector, with the reference's constructor, methods,
state-dict keys and output formats (``retinanet/models.py:21-288``).

Host side (this file, PyTorch-ROCm): transform -> ResNet -> FPN -> heads.
Device side (HIP, ``csrc/``): anchors (K1), matching + loss with gradients
(K2, K3) in ``forward``; decode, per-class NMS and top-k (K4-K7) in ``predict``.
"""
import logging
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from . import ops
from .anchors import AnchorGenerator
from .backbone import get_backbone
from .config import (BACKBONE, BBOX_REG_WEIGHTS, FREEZE_BN, MAX_DETECTIONS_PER_IMAGE, MAX_IMAGE_SIZE, MEAN,
                     MIN_BOX_SIZE, MIN_IMAGE_SIZE, NMS_THRES, NUM_CLASSES, PRETRAINED_BACKBONE, PRIOR, SCORE_THRES, STD)
from .layers import FeaturePyramid, RetinaNetHead
from .transform import GeneralizedRCNNTransform
from .utilities import ifnone

__small__ = ["resnet18", "resnet34"]
__big__ = ["resnet50", "resnet101", "resnet101", "resnet152"]


class Retinanet(nn.Module):
    """RetinaNet (Lin et al.) on a ResNet-FPN backbone.

    ``forward(images, targets)`` -> ``{"classification_loss", "regression_loss"}``;
    ``predict(images)`` -> ``[{"boxes" [n,4], "scores" [n], "labels" [n] in 1..K}]``, n <= 100.
    ``images``: list of ``[3,H,W]`` tensors in 0..1; ``targets``: list of
    ``{"boxes": F32[N,4] xyxy, "labels": I64[N] in 1..K}``.  Every constructor argument
    defaults to ``config.py`` (models.py:73-107).
    """

    def __init__(
        self,
        num_classes: Optional[int] = None,
        backbone_kind: Optional[str] = None,
        prior: Optional[float] = None,
        pretrained: Optional[bool] = None,
        nms_thres: Optional[float] = None,
        score_thres: Optional[float] = None,
        max_detections_per_images: Optional[int] = None,
        freeze_bn: Optional[bool] = None,
        min_size: Optional[int] = None,
        max_size: Optional[int] = None,
        image_mean: Optional[List[float]] = None,
        image_std: Optional[List[float]] = None,
        anchor_generator: Optional[AnchorGenerator] = None,
        logger=None,
        matcher: Optional[str] = None,
        atss_topk: Optional[int] = None,
        box_loss: Optional[str] = None,
        box_loss_weight: Optional[float] = None,
        box_decode: Optional[str] = None,
        nms: Optional[str] = None,
        soft_nms_sigma: Optional[float] = None,
        soft_nms_min_score: Optional[float] = None,
        cls_loss: Optional[str] = None,
        qfl_beta: Optional[float] = None,
        tal_topk: Optional[int] = None,
        tal_alpha: Optional[int] = None,
        tal_beta: Optional[int] = None,
    ) -> None:
        """``matcher``: how anchors are labelled -- None / "iou" (the reference's max-IoU rule, K2), "atss" (``ops.atss_match``,
        with ``atss_topk`` nearest locations per level and object, None -> 9) or "tal" (``ops.tal_match``, TOOD's task-aligned
        assignment: per object the ``tal_topk`` (None -> 13) anchors with the largest ``score^tal_alpha * IoU^tal_beta`` (None -> 1
        and 6; integers) among those whose centre lies inside the box, from what the head predicts at that step);
        ``model: {matcher: atss}`` / ``model: {matcher: tal}`` in the hparams.  "tal" ranks by the IoU of the box
        ``box_decode="standard"`` decodes, so with the reference decode it logs the warning "giou" / "diou" / "qfl" log.
        ``box_loss``: the box regression loss -- None / "smooth_l1" (the reference's, inside K3) or "giou" / "diou" (``ops.box_iou_loss``
        behind K3), times ``box_loss_weight`` (None -> 1.0); ``model: {box_loss: giou, box_loss_weight: 2.0}`` in the hparams.  Training
        only: what decodes the detections is ``box_decode``, whatever the loss.
        ``box_decode``: how ``predict`` / ``predict_staged`` / ``process_detections*`` turn the four box outputs into a box -- None /
        "reference" (K4 with the reference's quirk Q4: the sizes come from ``exp(dx)``, ``exp(dy)`` and ``dw``, ``dh`` are never read) or
        "standard" (the inverse of the training targets' encode, which is also what "giou" / "diou" optimise: sizes from ``dw``,
        ``dh``, clipped at ``ops.BOX_XFORM_CLIP``); ``model: {box_decode: standard}`` in the hparams.  Stored as ``net.box_decode`` and
        read at every call.  A model trained with "giou" / "diou" and inferred with the reference decode logs a warning here.
        ``nms``: the per-class NMS of the same calls -- None / "hard" (K6: greedy NMS at ``nms_thres``, the reference's) or Soft-NMS,
        which lowers the score of a box that overlaps a picked one instead of dropping it: "soft_linear" (by 1 - IoU where IoU >
        ``nms_thres``) or "soft_gaussian" (by exp(-IoU^2 / ``soft_nms_sigma``), None -> 0.5); a class ends when its best remaining score
        is not above ``soft_nms_min_score`` (None -> 1e-3); ``model: {nms: soft_gaussian}`` in the hparams.  Stored as ``net.nms``,
        ``net.soft_nms_sigma`` and ``net.soft_nms_min_score`` and read at every call (``ops.detect_levels``).
        ``cls_loss``: the classification loss -- None / "focal" (the reference's, inside K3) or "qfl" (Quality Focal Loss:
        ``ops.quality_focal_loss`` behind K3; the label element's target is the IoU of the row's standard-decoded box with its GT
        box, the exponent ``qfl_beta``, None -> 2.0); ``model: {cls_loss: qfl, qfl_beta: 2.0}`` in the hparams.  Training only: the
        score already is what NMS and the evaluator rank.  The quality is the IoU of the box ``box_decode="standard"`` decodes, so
        "qfl" with the reference decode logs a warning here, as "giou" / "diou" do."""
        super().__init__()
        cls_loss = ifnone(cls_loss, "focal")
        if cls_loss not in ops.CLS_LOSSES:
            raise ValueError(f"cls_loss must be one of {ops.CLS_LOSSES}, got {cls_loss!r}")
        qfl_beta = ifnone(qfl_beta, 2.0)
        nms = ifnone(nms, "hard")
        if nms not in ops.NMS_KINDS:
            raise ValueError(f"nms must be one of {ops.NMS_KINDS}, got {nms!r}")
        soft_nms_sigma = ifnone(soft_nms_sigma, 0.5)
        soft_nms_min_score = ifnone(soft_nms_min_score, 1e-3)
        box_decode = ifnone(box_decode, "reference")
        if box_decode not in ops.BOX_DECODES:
            raise ValueError(f"box_decode must be one of {ops.BOX_DECODES}, got {box_decode!r}")
        matcher = ifnone(matcher, "iou")
        atss_topk = ifnone(atss_topk, 9)
        tal_topk, tal_alpha, tal_beta = ifnone(tal_topk, 13), ifnone(tal_alpha, 1), ifnone(tal_beta, 6)
        box_loss = ifnone(box_loss, "smooth_l1")
        box_loss_weight = ifnone(box_loss_weight, 1.0)
        num_classes = ifnone(num_classes, NUM_CLASSES)
        backbone_kind = ifnone(backbone_kind, BACKBONE)
        prior = ifnone(prior, PRIOR)
        pretrained = ifnone(pretrained, PRETRAINED_BACKBONE)
        nms_thres = ifnone(nms_thres, NMS_THRES)
        score_thres = ifnone(score_thres, SCORE_THRES)
        max_detections_per_images = ifnone(max_detections_per_images, MAX_DETECTIONS_PER_IMAGE)
        freeze_bn = ifnone(freeze_bn, FREEZE_BN)
        min_size = ifnone(min_size, MIN_IMAGE_SIZE)
        max_size = ifnone(max_size, MAX_IMAGE_SIZE)
        image_mean = ifnone(image_mean, MEAN)
        image_std = ifnone(image_std, STD)
        anchor_generator = ifnone(anchor_generator, AnchorGenerator())
        logger = ifnone(logger, logging.getLogger(__name__))
        logger.name = __name__

        if backbone_kind not in __small__ + __big__:
            raise ValueError(f"Expected `backbone_kind` to be one of {__small__ + __big__} got {backbone_kind}")

        self.backbone_kind = backbone_kind
        self.transform = GeneralizedRCNNTransform(min_size, max_size, image_mean, image_std)
        self.backbone = get_backbone(backbone_kind, pretrained, freeze_bn=freeze_bn)
        c3, c4, c5 = self._get_backbone_ouputs()
        self.fpn = FeaturePyramid(c3, c4, c5, 256)
        self.anchor_generator = anchor_generator
        num_anchors = self.anchor_generator.num_cell_anchors[0]
        self.retinanet_head = RetinaNetHead(256, 256, num_anchors, num_classes, prior, matcher=matcher, atss_topk=atss_topk,
                                            cells=self.anchor_generator.num_anchors, box_loss=box_loss, box_loss_weight=box_loss_weight,
                                            cls_loss=cls_loss, qfl_beta=qfl_beta, tal_topk=tal_topk, tal_alpha=tal_alpha, tal_beta=tal_beta)

        self.score_thres = score_thres
        self.nms_thres = nms_thres
        self.detections_per_img = max_detections_per_images
        self.num_classes = num_classes
        self.box_decode = box_decode
        self.nms = nms
        self.soft_nms_sigma = float(soft_nms_sigma)
        self.soft_nms_min_score = float(soft_nms_min_score)
        if box_loss in ("giou", "diou") and box_decode == "reference":
            logger.warning(f'box_loss="{box_loss}" trains the box that box_decode="standard" decodes, but this model infers with the '
                           'reference decode (sizes from exp(dx), exp(dy)): pass box_decode="standard" (model: {box_decode: standard}) '
                           "to evaluate what was trained")
        if matcher == "tal" and box_decode == "reference":
            logger.warning('matcher="tal" picks the positives by the IoU of the box that box_decode="standard" decodes, but this model '
                           'infers with the reference decode (sizes from exp(dx), exp(dy)): pass box_decode="standard" '
                           "(model: {box_decode: standard}) so that inference decodes the box the labels were aligned to")
        if cls_loss == "qfl" and box_decode == "reference":
            logger.warning('cls_loss="qfl" trains the class score towards the IoU of the box that box_decode="standard" decodes, but this '
                           'model infers with the reference decode (sizes from exp(dx), exp(dy)): pass box_decode="standard" '
                           "(model: {box_decode: standard}) so that the score ranks the box it was trained on")

        logger.info(f"BACKBONE     : {backbone_kind}")
        logger.info(f"INPUT_PARAMS : MAX_SIZE={max_size}, MIN_SIZE={min_size}")
        logger.info(f"NUM_CLASSES  : {self.num_classes}")

    def _get_backbone_ouputs(self) -> List[int]:
        "Channel counts of C3, C4, C5 (models.py:135-150)."
        net = self.backbone.backbone
        last = "conv2" if self.backbone_kind in __small__ else "conv3"
        return [getattr(stage[-1], last).out_channels for stage in (net.layer2, net.layer3, net.layer4)]

    # -- conv stack ------------------------------------------------------------------------
    def _features(self, batch: Tensor) -> Tuple[List[Tensor], Dict[str, Tensor]]:
        if self.backbone.backbone.conv1.weight.is_contiguous(memory_format=torch.channels_last):
            batch = batch.contiguous(memory_format=torch.channels_last)   # model was moved to channels_last
        feature_maps = self.fpn(self.backbone(batch))
        return feature_maps, self.retinanet_head(feature_maps)

    def _batch_layout(self) -> Dict[str, object]:
        """Layout / dtype the conv stack will consume, for the fused transform kernel: channels-last when
        the model is, and autocast's dtype when autocast is on (conv1 would cast its input to it anyway,
        with the same round-to-nearest-even)."""
        w = self.backbone.backbone.conv1.weight
        cl = w.is_contiguous(memory_format=torch.channels_last)
        dt = torch.get_autocast_dtype("cuda") if (w.is_cuda and torch.is_autocast_enabled("cuda")) else None
        return {"out_dtype": dt, "channels_last": cl}

    # -- training ----------------------------------------------------------------------------
    def compute_loss(self, targets: List[Dict[str, Tensor]], outputs: Dict[str, Tensor],
                     anchors: List[Tensor]) -> Dict[str, Tensor]:
        return self.retinanet_head.compute_loss(targets, outputs, anchors)

    def forward(self, images: List[Tensor], targets: Optional[List[Dict[str, Tensor]]] = None):
        """Losses of the batch (models.py:274-288).  The reference requires `targets`
        (its Lightning wrapper's ``forward`` therefore raises); here
        ``targets=None`` means inference and returns ``predict(images)``.  ``targets`` may also be packed GT
        (``ops.PackedGT``, staged by ``ops.gt_stage``: the GT capacity mode of ``graph.CapturedTrainStep``), and ``images`` staged
        images (``ops.StagedImages``, staged by ``ops.image_stage``: its image capacity mode; training mode only -- inference on staged images is
        ``predict_staged``) -- they go to
        the transform as they are, with the canvas they carry."""
        if targets is None:
            return self.predict(images)
        from .transform import _is_staged
        if _is_staged(images):
            if not self.training:
                raise ValueError("staged images (ops.StagedImages) are a training input")
            images, targets = self.transform(images, targets, canvas=images.canvas, **self._batch_layout())
        else:
            images, targets = self.transform(images, targets, **self._batch_layout())
        batch = images.tensors
        if self.backbone.backbone.conv1.weight.is_contiguous(memory_format=torch.channels_last):
            batch = batch.contiguous(memory_format=torch.channels_last)        # no-op after the fused transform
        if batch.is_cuda and self.training and torch.is_grad_enabled():
            from . import biasact
            biasact.refresh_dgrad_weights(batch.device)            # the backward pass's flipped 3x3 weights: one launch for the whole model
        feature_maps = self.fpn(self.backbone(batch))
        anchors = self.anchor_generator(images, feature_maps)
        # K2 (IoU + matcher) needs only the anchors and the GT boxes: it goes out on a side stream here and runs beside the
        # head convolutions; K3 waits for it (losses.RetinaNetLosses.match_ahead).  NOT while the step is being captured into a
        # hipGraph: a graph with a forked branch costs hipGraphLaunch 20 ms of host time per replay on ROCm 7.0 (0.4 ms for
        # the linear graph of the same step, bench.py host_enqueue_ms_per_step) -- 25 us of GPU time are not worth that.
        ahead = None
        crit = self.retinanet_head.losses
        if batch.is_cuda and crit.matcher == "tal":
            # the task-aligned rule reads the head's outputs: the handle only records it (nothing is launched, so a capture may hold
            # it too), with the grid width of every level -- its kernel then visits only the cells under each box
            sizes = [int(f.shape[-2]) * int(f.shape[-1]) * n for f, n in zip(feature_maps, self.anchor_generator.num_anchors)]
            ahead = crit.match_ahead(targets, anchors, sizes, level_w=[int(f.shape[-1]) for f in feature_maps])
        elif batch.is_cuda and not torch.cuda.is_current_stream_capturing() and not crit.fuses_match(targets):
            sizes = None
            if crit.matcher == "atss":                                            # (its candidates are chosen per pyramid level)
                sizes = [int(f.shape[-2]) * int(f.shape[-1]) * n for f, n in zip(feature_maps, self.anchor_generator.num_anchors)]
            ahead = crit.match_ahead(targets, anchors, sizes)                     # (<= 64 GT per image: K2 runs inside K3, no launch at all)
        # same losses as compute_loss(targets, retinanet_head(feature_maps), anchors), but the loss kernel
        # reads the five per-level conv outputs in place instead of their torch.cat (layers.py:195, :259)
        outputs = self.retinanet_head.forward_levels(feature_maps)
        return self.retinanet_head.compute_loss_levels(targets, outputs, anchors, ahead=ahead)

    # -- inference ---------------------------------------------------------------------------
    def process_detections(self, outputs: Dict[str, Tensor], anchors: List[Tensor],
                           im_szs: List[Tuple[int, int]]) -> List[Dict[str, Tensor]]:
        """Raw head outputs -> per-image detections (models.py:160-243): one HIP call
        (``rn_detect``) for the whole batch instead of B*K sequential NMS launches.  Boxes are decoded as ``self.box_decode`` says and
        suppressed as ``self.nms`` says."""
        class_logits = outputs.pop("cls_preds")
        bboxes = outputs.pop("bbox_preds")
        if any(w != 1.0 for w in BBOX_REG_WEIGHTS):
            bboxes.div_(bboxes.new_tensor([BBOX_REG_WEIGHTS]))          # box_utils.py:43 (in place, Q5)
        return ops.detect(class_logits, bboxes, anchors, im_szs, self.score_thres, MIN_BOX_SIZE, self.nms_thres,
                          self.detections_per_img, decode=self.box_decode, **self._nms_args())

    def process_detections_levels(self, outputs: Dict[str, List[Tensor]], anchors: List[Tensor],
                                  im_szs: List[Tuple[int, int]]) -> List[Dict[str, Tensor]]:
        """``process_detections`` on the per-level head outputs of ``retinanet_head.forward_levels``: the scan
        and decode kernels read the five conv outputs in place (no ``torch.cat``, layers.py:195, :259)."""
        return ops.detect_levels(outputs["cls_levels"], outputs["bbox_levels"], anchors, im_szs, self.score_thres,
                                 MIN_BOX_SIZE, self.nms_thres, self.detections_per_img, reg_w=BBOX_REG_WEIGHTS,
                                 decode=self.box_decode, **self._nms_args())

    def _nms_args(self) -> Dict[str, object]:
        "The NMS kind of the detect chain as ``ops.detect*`` takes it, read from the attributes at every call."
        return {"nms": self.nms, "nms_sigma": self.soft_nms_sigma, "nms_min_score": self.soft_nms_min_score}

    def predict(self, images: List[Tensor]) -> List[Dict[str, Tensor]]:
        """Detections in original image coordinates (models.py:245-272).  Like the
        reference this only flips the TOP module's ``training`` flag (Q17): call
        ``.eval()`` first for eval-mode BN and for the rescale to original sizes.
        The conv stack runs under ``no_grad`` (nothing back-propagates through detections)."""
        if self.training:
            self.training = False
        original_image_sizes = []
        for img in images:
            val = img.shape[-2:]
            assert len(val) == 2
            original_image_sizes.append((int(val[0]), int(val[1])))
        with torch.no_grad():
            images, _ = self.transform(images, None, **self._batch_layout())
            batch = images.tensors
            if self.backbone.backbone.conv1.weight.is_contiguous(memory_format=torch.channels_last):
                batch = batch.contiguous(memory_format=torch.channels_last)
            feature_maps = self.fpn(self.backbone(batch))
            anchors = self.anchor_generator(images, feature_maps)
            detections = self.process_detections_levels(self.retinanet_head.forward_levels(feature_maps), anchors,
                                                        images.image_sizes)
            return self.transform.postprocess(detections, images.image_sizes, original_image_sizes)

    def predict_staged(self, staged, canvas: Optional[Tuple[int, int]] = None, max_candidates=None) -> Tensor:
        """``predict`` on staged images (``ops.StagedImages``, staged by ``ops.image_stage``) over the padded canvas ``canvas`` (default:
        the one the arena carries) -> the DEVICE result block of ``ops.detect_finish_var`` (``ops.detect_result_dicts`` turns it
        into ``predict``'s list of dicts).  The same chain -- transform, conv stack under ``no_grad``, anchors on the canvas, detect,
        rescale to the original sizes -- but nothing it launches takes an image's address or size as an argument and nothing is read
        back: the sizes stay on the device from ``rn_image_stage`` to ``rn_detect_finish_var``.  No synchronisation, so
        ``graph.CapturedPredict`` captures it.  ``max_candidates``: the detect chain's per-image capacity (``ops.detect_levels``: an
        int, None for its default, "all" for the worst case); an image that needed more has ``status != 0`` in the block, and the
        caller runs the batch again with "all".  Eval mode only: ``net.eval()`` first -- this does not flip the flag as ``predict`` does."""
        if self.training or self.transform.training:
            raise ValueError("predict_staged runs in eval mode: call net.eval() first")
        canvas = staged.canvas if canvas is None else canvas
        with torch.no_grad():
            images, _ = self.transform(staged, None, canvas=canvas, **self._batch_layout())
            batch = images.tensors
            if self.backbone.backbone.conv1.weight.is_contiguous(memory_format=torch.channels_last):
                batch = batch.contiguous(memory_format=torch.channels_last)        # no-op after the fused transform
            feature_maps = self.fpn(self.backbone(batch))
            anchors = self.anchor_generator(images, feature_maps)
            outputs = self.retinanet_head.forward_levels(feature_maps)
            padded = ops.detect_levels(outputs["cls_levels"], outputs["bbox_levels"], anchors, None, self.score_thres, MIN_BOX_SIZE,
                                       self.nms_thres, self.detections_per_img, reg_w=BBOX_REG_WEIGHTS, max_candidates=max_candidates,
                                       image_hw_dev=images.image_sizes_dev, padded=True, decode=self.box_decode,
                                       **self._nms_args())
            return ops.detect_finish_var(*padded, staged.in_hw, images.image_sizes_dev)
