"""Input transform used by ``Retinanet`` (reference call sites ``retinanet/models.py:116,
:262, :271, :279``; the reference takes it from torchvision's detection package,
which this framework does not depend on).

Semantics (torchvision 0.7/0.8 ``GeneralizedRCNNTransform``): per image
``(x - mean) / std`` -> bilinear resize so the short side is ``min_size`` unless the
long side would exceed ``max_size`` (``align_corners=False``, scale recomputed from
the integer output size) -> GT boxes scaled by the per-axis size ratio -> images
zero-padded into one batch whose H, W are rounded up to a multiple of 32.
``postprocess`` maps detections back to the original image sizes (eval mode only).

For CUDA fp32 images the normalise / resize / pad / batch sequence is ONE HIP launch
(``rn_transform_batch``, ``csrc/transform.hip``) that can also write the batch
directly in the layout and dtype the conv stack consumes (channels-last, autocast dtype), so the
per-image elementwise kernels, the batch memset + copies, the ``contiguous(channels_last)`` pass
and autocast's cast of the conv1 input all disappear.  Anything else (CPU tensors, other dtypes)
takes the PyTorch ops below, which implement the same arithmetic.  uint8 ``[3, h, w]`` images -- planes or
interleaved, what image decoders give -- are converted to fp32 in [0, 1] first (``ops.images_u8_to_f32``:
``float(v) / 255`` with one correctly rounded division; ``rn_image_stage_u8`` on CUDA, a true division on the
CPU, the same bits) and then take the same two paths.

Train-time horizontal flip (``hflip``: an ``augment.RandomHorizontalFlip``, None by default): in training mode and when targets
are given, each image is flipped with probability p before the normalise / resize, and its boxes with it (x1' = W - x2,
x2' = W - x1, W = the width before the resize; the reference's ``RandomHorizontalFlip`` / albumentations ``HorizontalFlip``).
On the fused path the decisions are drawn on the device (``rn_hflip_draw``), the flip is the transform kernel's mirrored
gather (``rn_transform_batch_flip``) and the boxes' flip + resize one launch (``rn_gt_flip_scale_many`` / ``_packed``), so
a captured train step draws new flips at every replay.  The PyTorch path does the same with ``img.flip(-1)`` and the box
formula, selected by the flags with ``torch.where``.  ``hflip`` is a plain attribute: the state-dict keys do not change.

Multi-scale training on the device (``scale_jitter``: an ``augment.RandomShortSide``, None by default): in training mode and when
targets are given, each image's short side is drawn by the installed object instead of by ``_target_short_side`` (which is then not
consulted; eval mode is exactly as without one).  The padded canvas is computed on the host from the object's upper bound of every
image's size (its largest short side), rounded up to ``size_divisible``: it depends on the image shapes alone, so a captured
train step keeps ONE graph while the scales vary.  On the fused path the sizes are drawn on the device (``rn_short_side_draw``),
stay there as ``scale_jitter.sizes_drawn`` (int32 [B, 2]) and are read by the transform kernel (``rn_transform_batch_dev``) and
the box kernels (``rn_gt_flip_scale_many_dev`` / ``_packed_dev``); the flip composes.  ``ImageList.image_sizes`` then holds the
upper-bound sizes, not the drawn ones -- the training pass does not read them beyond their number (anchors, matching and the
loss are laid out on the padded canvas).  The PyTorch path draws the same sizes from the Python restatement, resizes each image
with ``resize`` and pads the batch to the same canvas.  The known cost: the whole canvas is processed whatever was drawn, so small
draws save no compute.  ``scale_jitter`` is a plain attribute too.

Train-time colour jitter (``color_jitter``: an ``augment.ColorJitter``, None by default): in training mode and when targets are given,
each image is jittered with probability p -- torchvision's tensor ``ColorJitter`` on the raw fp32 RGB image in [0, 1], before the
normalisation, the resize and the flip (it is per pixel apart from the contrast's mean, so it commutes with the flip).  On the fused
paths the factors and the order are drawn on the device (``rn_color_jitter_draw``), the contrast's mean gray is one pair of launches
over the source images when a contrast is enabled (``rn_color_mean``), and the operations run inside the transform kernel on every
source pixel it reads (``rn_transform_batch_color``); the rows stay on the device as ``color_jitter.coef``.  The PyTorch path draws the
same stream from the Python restatement and applies ``augment.apply_color_ops``.  ``color_jitter`` is a plain attribute too.

Train-time brightness / contrast (``brightness_contrast``: an ``augment.RandomBrightnessContrast``, None by default): in training mode
and when targets are given, each image becomes ``clamp(alpha x + beta ref)`` with probability p -- albumentations'
``RandomBrightnessContrast`` on the raw fp32 RGB image in [0, 1], after the crop, the warp and the colour jitter's operations, before the
normalisation, the resize and the flip.  On the fused paths its two coefficients are drawn into the colour jitter's rows
(``rn_brightness_contrast_draw``; fresh identity rows without a jitter), the by-mean reference is one more pair of launches over the
source images (``rn_brightness_contrast_mean``, only with ``brightness_by_max=False``), and the transform kernel applies them to every
source pixel it reads; the rows stay on the device as ``brightness_contrast.coef``.  The PyTorch path draws the same stream from the
Python restatement and applies ``augment.apply_brightness_contrast``.  A plain attribute too.

Staged images (``forward(ops.StagedImages, packed GT, canvas=(Hp, Wp))``: the image capacity mode of ``graph.CapturedTrainStep``):
the batch lies in a fixed device arena with its sizes next to it (``ops.image_stage``), and nothing this call launches takes an
image's address or size as an argument -- the resize plan (``rn_resize_plan_dev``: the fixed short side, or the ``scale_jitter``'s
draw), the boxes (``rn_gt_flip_scale_packed_var``) and the transform kernel (``rn_transform_batch_var``) read them on the device, over
the canvas the caller fixed.  In training mode with packed GT, or in eval mode without targets (``Retinanet.predict_staged``: the plan
with the fixed eval short side ``min_size[-1]``, no flip, no jitter; the sizes it wrote stay on the device as ``ImageList.image_sizes_dev``);
the fused path only.  The result is bit-identical to the list path's on the same canvas; the cost is the jitter's: the conv stack
processes the whole class canvas whatever the batch's own canvas was.

Train-time bbox-safe random crop (``crop``: an ``augment.BBoxSafeRandomCrop``, None by default): in training mode and when targets are
given, each image is cropped with probability p to a random window that contains all of its boxes, and the boxes are shifted with it --
FIRST, before the flip, the colour jitter and the resize, which then see the cropped image.  On staged images with packed GT it is a
second staging pass on the device (``ops.bbox_crop_staged``: ``rn_bbox_crop_draw`` + ``rn_image_crop_stage`` into a second arena, the
cropped sizes next to it), so everything after it runs unchanged and is bit-identical to the same call on the sliced images; the canvas
follows from ``crop.bound`` (the crop keeps the orientation), so ``staged_bounds`` depends on the image shapes alone.  Every other input
draws the same rectangles on the HOST from the Python restatement -- the boxes and the counter are read back, one synchronisation on
CUDA -- slices the images and shifts the boxes with torch, and goes on as without a crop.  ``crop`` is a plain attribute too.

Train-time shift / scale / rotate (``shift_scale_rotate``: an ``augment.ShiftScaleRotate``, None by default): in training mode and when
targets are given, each image is moved with probability p by a random shift, scale and rotation about its centre (bilinear, reflect-101
border), its boxes become the clipped bounding boxes of their moved corners, and boxes of which nothing (or less than
``min_visibility``) is left are dropped -- AFTER the crop and before the flip, the colour jitter and the resize.  Sizes do not change, so
``staged_bounds`` is untouched.  On staged images with packed GT it is one more staging pass on the device
(``ops.shift_scale_rotate_staged``: ``rn_affine_draw`` + ``rn_image_warp_stage`` into another arena, the surviving rows packed into new
buffers with new offsets), bit-identical to the same call on images and targets pre-warped by the restatement with the device's
coefficients.  Every other input draws from the Python restatement on the HOST (one synchronisation on CUDA) and warps with torch ops.
"""
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor, nn


# The train-time augmentation slots of ``GeneralizedRCNNTransform`` (module docstring): plain attributes, None by default, each acting
# in training mode when targets are given.  The order is the one ``graph.CapturedTrainStep`` lists them in its key.  Adding one:
# DESIGN.md, "Adding an augmentation".
AUGMENT_SLOTS = (
    "hflip",                  # augment.RandomHorizontalFlip: the train-time flip
    "scale_jitter",           # augment.RandomShortSide: the short side drawn on the device
    "color_jitter",           # augment.ColorJitter: the colour jitter drawn and applied on the device
    "crop",                   # augment.BBoxSafeRandomCrop: the bbox-safe random crop, before everything else
    "shift_scale_rotate",     # augment.ShiftScaleRotate: shift / scale / rotate, after the crop
    "brightness_contrast",    # augment.RandomBrightnessContrast: alpha x + beta ref behind the colour jitter
)


def augments_of(transform) -> List[Tuple[str, object]]:
    """The augmentations installed in ``transform``'s slots, as (name, object) pairs in ``AUGMENT_SLOTS`` order.  THE way to read a
    slot: a transform unpickled from before a slot existed has no such attribute, and neither has a foreign transform or None."""
    return [(name, obj) for name in AUGMENT_SLOTS for obj in (getattr(transform, name, None),) if obj is not None]


class ImageList(object):
    """A padded batch plus each image's (h, w) before padding."""

    def __init__(self, tensors: Tensor, image_sizes: List[Tuple[int, int]]):
        self.tensors = tensors
        self.image_sizes = image_sizes

    def to(self, device) -> "ImageList":
        return ImageList(self.tensors.to(device), self.image_sizes)


def _ratios(original_size: Sequence[int], new_size: Sequence[int]) -> Tuple[float, float]:
    # fp32 ratios (as torchvision computes them), applied as host scalars: no H2D copy, no sync
    return (float(np.float32(new_size[0]) / np.float32(original_size[0])), float(np.float32(new_size[1]) / np.float32(original_size[1])))


def _resize_packed(targets, ratios: List[Tuple[float, float]]):
    """``resize_boxes`` for every image of packed GT (``ops.PackedGT``): one ``rn_gt_scale_packed`` launch into a buffer owned by this
    call -- never in place on the staged buffer, which a replayed graph reads again at the next step -- or ``targets`` itself when
    no ratio differs from 1."""
    if all(r == (1.0, 1.0) for r in ratios):
        return targets
    from . import ops
    return ops.gt_scale_packed(targets, ratios)


def _is_packed(targets) -> bool:
    if targets is None or isinstance(targets, (list, tuple)):
        return False
    from .ops import PackedGT
    return isinstance(targets, PackedGT)


def _is_staged(images) -> bool:
    if isinstance(images, (list, tuple)):
        return False
    from .ops import StagedImages
    return isinstance(images, StagedImages)


def resize_boxes(boxes: Tensor, original_size: Sequence[int], new_size: Sequence[int]) -> Tensor:
    rh, rw = _ratios(original_size, new_size)
    if rh == 1.0 and rw == 1.0:
        return boxes
    x1, y1, x2, y2 = boxes.unbind(1)
    return torch.stack((x1 * rw, y1 * rh, x2 * rw, y2 * rh), dim=1)


def hflip_boxes(boxes: Tensor, width: float) -> Tensor:
    "Boxes of an image of width ``width`` after a horizontal flip: x1' = W - x2, x2' = W - x1 (fp32; the reference's formula)."
    x1, y1, x2, y2 = boxes.reshape(-1, 4).unbind(1)
    return torch.stack((width - x2, y1, width - x1, y2), dim=1)


def _flip_where(flag: Tensor, image: Tensor, target: Optional[Dict[str, Tensor]]):
    "The PyTorch path's flip of one image (and its boxes) where ``flag`` (0-dim) is set: no host synchronisation."
    f = flag.to(device=image.device, dtype=torch.bool)
    image = torch.where(f, image.flip(-1), image)
    if target is not None:
        b = target["boxes"].reshape(-1, 4)
        target["boxes"] = torch.where(f.to(b.device), hflip_boxes(b, float(image.shape[-1])), b)
    return image, target


def _boxes_into(targets: List[Dict[str, Tensor]], rows: Tensor) -> None:
    "One buffer with every image's boxes (what a flip + resize launch over the whole batch writes) into the target dicts: each gets its rows as a view."
    counts = [int(t["boxes"].reshape(-1, 4).shape[0]) for t in targets]
    for t, r in zip(targets, rows.split(counts)):
        t["boxes"] = r


def _gt_rows(targets, with_labels: bool):
    """GT as per-image rows, for the augmentations drawn on the host -> (boxes, labels, put).  ``boxes[b]`` [n_b, 4] and ``labels[b]``
    [n_b] are the target dicts' own tensors, or each image's range of ONE host copy of packed GT (``ops.PackedGT``: a synchronisation
    on CUDA); ``labels`` is None unless ``with_labels``, and a dict without labels gives None.  ``put(boxes, labels=None)`` -> the
    targets holding these rows instead: the dicts themselves, or a new PackedGT on the old one's device with buffers of the old size.
    Without ``labels`` no row was dropped: the labels and the offsets stay as they are."""
    if not _is_packed(targets):
        boxes = [t["boxes"].reshape(-1, 4) for t in targets]
        labels = [t["labels"].reshape(-1) if "labels" in t else None for t in targets] if with_labels else None

        def put(new_boxes, new_labels=None):
            for b, (t, bx) in enumerate(zip(targets, new_boxes)):
                t["boxes"] = bx.to(boxes[b].device)
                if new_labels is not None and new_labels[b] is not None:
                    t["labels"] = new_labels[b]
            return targets
        return boxes, labels, put
    off = [int(v) for v in targets.gt_off.tolist()]
    ranges = list(zip(off[:-1], off[1:]))
    rows = targets.gt_boxes.detach().cpu()
    row_labels = targets.gt_labels.detach().cpu() if with_labels else None

    def put(new_boxes, new_labels=None):
        dev = targets.gt_boxes.device
        out_b = rows.clone()
        if new_labels is None:
            for (lo, hi), bx in zip(ranges, new_boxes):
                out_b[lo:hi] = bx
            return targets.with_boxes(out_b.to(dev))
        out_l, new_off = row_labels.clone(), [0]
        for bx, lb in zip(new_boxes, new_labels):         # the rows that are left, packed from row 0
            at, n = new_off[-1], int(bx.shape[0])
            out_b[at:at + n], out_l[at:at + n] = bx, lb
            new_off.append(at + n)
        return targets.with_rows(out_b.to(dev), out_l.to(dev), torch.tensor(new_off, dtype=torch.int32).to(dev))
    return [rows[lo:hi] for lo, hi in ranges], None if row_labels is None else [row_labels[lo:hi] for lo, hi in ranges], put


class GeneralizedRCNNTransform(nn.Module):
    def __init__(self, min_size, max_size: int, image_mean: Sequence[float], image_std: Sequence[float],
                 size_divisible: int = 32):
        super().__init__()
        self.min_size = tuple(min_size) if isinstance(min_size, (list, tuple)) else (min_size,)
        self.max_size = max_size
        self.image_mean = list(image_mean)
        self.image_std = list(image_std)
        self.size_divisible = size_divisible
        self._stats = {}
        for name in AUGMENT_SLOTS:
            setattr(self, name, None)

    # -- the augmentation slots ----------------------------------------------------------
    def augments(self) -> List[Tuple[str, object]]:
        "The installed augmentations as (name, object) pairs in ``AUGMENT_SLOTS`` order (``augments_of``)."
        return augments_of(self)

    def _acting(self, targets) -> bool:
        "Whether the augmentations act on this call: in training mode and when targets are given."
        return self.training and targets is not None

    def _slot(self, name: str, targets):
        "The object installed in slot ``name`` when it acts on this call, else None."
        return getattr(self, name, None) if self._acting(targets) else None

    def set_rank(self, rank: int) -> None:
        "One stream of draws per data-parallel rank: every installed object's seed = its base seed + rank, its counter kept."
        for _, obj in self.augments():
            obj.set_rank(rank)

    # -- pieces ------------------------------------------------------------------------
    def normalize(self, image: Tensor) -> Tensor:
        key = (image.device, image.dtype, tuple(self.image_mean), tuple(self.image_std))
        stats = self._stats.get(key)
        if stats is None:       # uploaded once per (device, dtype): no per-image H2D copies
            mean = torch.as_tensor(self.image_mean, dtype=image.dtype, device=image.device)
            std = torch.as_tensor(self.image_std, dtype=image.dtype, device=image.device)
            stats = self._stats[key] = (mean[:, None, None], std[:, None, None])
        return (image - stats[0]) / stats[1]

    def _target_short_side(self) -> float:
        if self.training and len(self.min_size) > 1:
            return float(self.min_size[int(torch.empty(1).uniform_(0.0, float(len(self.min_size))).item())])
        return float(self.min_size[-1])

    def _scale_for(self, h: int, w: int, short: float) -> float:
        lo, hi = float(min(h, w)), float(max(h, w))
        scale = short / lo
        if hi * scale > float(self.max_size):
            scale = float(self.max_size) / hi
        return scale

    def resize(self, image: Tensor, target: Optional[Dict[str, Tensor]], short: Optional[float] = None):
        "``short``: the short side to resize to (a ``scale_jitter``'s draw) instead of ``_target_short_side()``."
        h, w = int(image.shape[-2]), int(image.shape[-1])
        scale = self._scale_for(h, w, self._target_short_side() if short is None else float(short))
        nh, nw = int(math.floor(h * scale)), int(math.floor(w * scale))
        if (nh, nw) != (h, w):
            image = F.interpolate(image[None], scale_factor=scale, mode="bilinear",
                                  recompute_scale_factor=True, align_corners=False)[0]
        # (same size => bilinear resampling with align_corners=False is the identity: skip the launch)
        if target is not None:
            target["boxes"] = resize_boxes(target["boxes"], (h, w), image.shape[-2:])
        return image, target

    def _canvas(self, sizes: Sequence[Tuple[int, int]]) -> Tuple[int, int]:
        d = float(self.size_divisible)
        return int(math.ceil(max(s[0] for s in sizes) / d) * d), int(math.ceil(max(s[1] for s in sizes) / d) * d)

    def batch_images(self, images: List[Tensor], canvas: Optional[Tuple[int, int]] = None) -> Tensor:
        "``canvas``: the padded (H, W) to use instead of the images' own maximum rounded up (a ``scale_jitter``'s fixed canvas)."
        c = max(im.shape[0] for im in images)
        hh, ww = canvas if canvas is not None else self._canvas([im.shape[1:] for im in images])
        out = images[0].new_zeros((len(images), c, hh, ww))
        for im, dst in zip(images, out):
            dst[: im.shape[0], : im.shape[1], : im.shape[2]].copy_(im)
        return out

    # -- fused path ----------------------------------------------------------------------
    def _fused_config(self) -> bool:
        "What the HIP transform kernels need of THIS module, whatever the images: three channels, a canvas in multiples of 4."
        return len(self.image_mean) == 3 and len(self.image_std) == 3 and self.size_divisible % 4 == 0

    def _fusable(self, images: List[Tensor]) -> bool:
        return (self._fused_config() and
                all(im.is_cuda and im.dim() == 3 and im.shape[0] == 3 and im.dtype == torch.float32 for im in images))

    def _flips(self, images: List[Tensor], targets) -> Optional[Tensor]:
        "This batch's flip decisions (uint8 [B], on the images' device; the flip's counter advances), or None when nothing flips."
        hflip = self._slot("hflip", targets)
        return None if hflip is None else hflip.next_flags(len(images), images[0].device)

    def _jitter(self, targets):
        "The installed ``scale_jitter`` when it acts on this call (training mode, targets given), else None."
        return self._slot("scale_jitter", targets)

    def _color(self, images, targets) -> Optional[Tensor]:
        """This batch's ``rn_color_coef`` rows (f32 [B, 8] on the images' device; the counters of the objects that act advance), or
        None when neither ``color_jitter`` nor ``brightness_contrast`` acts on this call.  The jitter draws first (its contrast mean
        included); brightness / contrast writes its two coefficients into the same rows, or into fresh identity rows.  ``images``:
        fusable CUDA images or ``ops.StagedImages``."""
        cj, bc = self._slot("color_jitter", targets), self._slot("brightness_contrast", targets)
        coef = cj.next_coef(images) if cj is not None else None
        return bc.next_coef(images, coef) if bc is not None else coef

    def _forward_fused_jitter(self, jitter, images: List[Tensor], targets, out_dtype: torch.dtype, channels_last: bool, flags, coef=None):
        "The fused path with the sizes drawn on the device: nothing about the draw reaches the host, the canvas is the bound's."
        from . import ops
        in_hw = [(int(im.shape[-2]), int(im.shape[-1])) for im in images]
        widths = [float(w) for _, w in in_hw]
        bounds = [jitter.bound(h, w, self.max_size) for h, w in in_hw]
        out_hw, ratios = jitter.next_sizes(in_hw, self.max_size, images[0].device)
        if _is_packed(targets):
            targets = ops.gt_flip_scale_packed_dev(targets, widths, ratios, flags)
        else:
            _boxes_into(targets, ops.gt_flip_scale_many_dev([t["boxes"] for t in targets], widths, ratios, flags))
        hp, wp = self._canvas(bounds)
        batch = ops.transform_batch_dev(images, out_hw, self.image_mean, self.image_std, hp, wp, out_dtype, channels_last, flags=flags,
                                        coef=coef)
        return ImageList(batch, bounds), targets

    def _forward_fused(self, images: List[Tensor], targets, out_dtype: torch.dtype, channels_last: bool):
        from . import ops                       # the HIP library is only needed once a CUDA image shows up
        flags = self._flips(images, targets)
        coef = self._color(images, targets)
        jitter = self._jitter(targets)
        if jitter is not None:
            return self._forward_fused_jitter(jitter, images, targets, out_dtype, channels_last, flags, coef)
        sizes, ratios, widths = [], [], []
        packed = _is_packed(targets)
        for i, im in enumerate(images):
            h, w = int(im.shape[-2]), int(im.shape[-1])
            scale = self._scale_for(h, w, self._target_short_side())       # drawn per image, like torchvision
            new = (int(math.floor(h * scale)), int(math.floor(w * scale)))
            sizes.append(new)
            widths.append(float(w))
            if packed or flags is not None:
                ratios.append(_ratios((h, w), new))
            elif targets is not None:
                targets[i]["boxes"] = resize_boxes(targets[i]["boxes"], (h, w), new)
        if packed:
            targets = _resize_packed(targets, ratios) if flags is None else ops.gt_flip_scale_packed(targets, widths, ratios, flags)
        elif flags is not None:
            # every image's flip + resize in one launch into one buffer; each target gets its rows as a view
            _boxes_into(targets, ops.gt_flip_scale_many([t["boxes"] for t in targets], widths, ratios, flags))
        hp, wp = self._canvas(sizes)
        batch = ops.transform_batch(images, sizes, self.image_mean, self.image_std, hp, wp, out_dtype, channels_last, flags=flags, coef=coef)
        return ImageList(batch, sizes), targets

    def staged_short_side(self) -> Optional[int]:
        """The short side the staged path passes to the device when no ``scale_jitter`` is installed, or None when that path cannot
        serve this transform in training: a ``min_size`` tuple drawn on the host changes from step to step (install an
        ``augment.RandomShortSide``), and the device plan takes integers."""
        if len(self.min_size) != 1 or int(self.min_size[0]) != self.min_size[0] or int(self.max_size) != self.max_size:
            return None
        return int(self.min_size[0])

    def staged_bounds(self, in_hw: Sequence[Tuple[int, int]]) -> List[Tuple[int, int]]:
        """Host arithmetic on the raw sizes alone: per image the size after the resize -- with a ``scale_jitter`` installed the upper
        bound of every size it can draw (``jitter.bound``).  The natural canvas of a staged batch is ``_canvas`` over these."""
        installed = dict(self.augments())
        jitter, crop = installed.get("scale_jitter"), installed.get("crop")
        short = None if jitter is not None else self.staged_short_side()      # (the value the device plan gets: bound and plan cannot drift apart)
        if jitter is None and short is None:
            raise ValueError(f"staged images need one integer min_size and an integer max_size (got {self.min_size}, {self.max_size}), "
                             "or an augment.RandomShortSide as scale_jitter")
        if crop is not None:
            # the window is drawn on the device: the bound is that of every window of the image's orientation (``crop.bound``)
            most = max((jitter.canvas_short,) + tuple(jitter.sizes)) if jitter is not None else short
            return [crop.bound(int(h), int(w), most, int(self.max_size)) for h, w in in_hw]
        if jitter is not None:
            return [jitter.bound(int(h), int(w), self.max_size) for h, w in in_hw]
        return self._sizes_for(in_hw, float(short))

    def _sizes_for(self, in_hw: Sequence[Tuple[int, int]], short: float) -> List[Tuple[int, int]]:
        out = []
        for h, w in in_hw:
            scale = self._scale_for(int(h), int(w), short)
            out.append((int(math.floor(h * scale)), int(math.floor(w * scale))))
        return out

    def staged_eval_short_side(self) -> Optional[int]:
        """The short side the staged path passes to the device in eval mode -- ``min_size[-1]``, what ``_target_short_side`` returns
        there -- or None when it or ``max_size`` is no integer (the device plan takes integers)."""
        if int(self.min_size[-1]) != self.min_size[-1] or int(self.max_size) != self.max_size:
            return None
        return int(self.min_size[-1])

    def staged_eval_bounds(self, in_hw: Sequence[Tuple[int, int]]) -> List[Tuple[int, int]]:
        "``staged_bounds`` for eval mode: the sizes after the resize to the fixed eval short side (a ``scale_jitter`` does not act there)."
        short = self.staged_eval_short_side()
        if short is None:
            raise ValueError(f"staged images in eval mode need an integer min_size[-1] and an integer max_size (got {self.min_size}, {self.max_size})")
        return self._sizes_for(in_hw, float(short))

    def _check_staged_canvas(self, canvas, staged, bounds_of) -> Tuple[Tuple[int, int], List[Tuple[int, int]]]:
        "-> ((Hp, Wp), the per-image bounds: the stager's when it has them, else ``bounds_of(staged.hw)``); ValueError when they do not fit."
        if canvas is None:
            raise ValueError("staged images need canvas=(Hp, Wp)")
        if not (len(self.image_mean) == 3 and len(self.image_std) == 3 and self.size_divisible % 4 == 0):
            raise ValueError("staged images take the fused transform only: 3 channels, size_divisible a multiple of 4")
        hp, wp = int(canvas[0]), int(canvas[1])
        bounds = staged.bounds if staged.bounds is not None else bounds_of(staged.hw)
        need = self._canvas(bounds)
        if need[0] > hp or need[1] > wp:
            raise ValueError(f"canvas {hp} x {wp} does not contain the batch's own canvas {need[0]} x {need[1]}")
        return (hp, wp), bounds

    def _forward_staged_eval(self, staged, canvas, out_dtype: torch.dtype, channels_last: bool):
        """Staged images in eval mode (``Retinanet.predict_staged``): the resize plan with the fixed eval short side, no flip, no
        jitter, no targets.  The sizes the plan wrote stay on the device as ``ImageList.image_sizes_dev`` (int32 [B, 2]): the detect
        chain clips to them and ``rn_detect_finish_var`` maps the boxes back with them; ``image_sizes`` holds the host's restatement."""
        from . import ops
        if len(staged.hw) != staged.B:
            raise ValueError(f"{len(staged.hw)} staged images in an arena of {staged.B}")
        (hp, wp), bounds = self._check_staged_canvas(canvas, staged, self.staged_eval_bounds)
        short = self.staged_eval_short_side()
        if short is None:
            raise ValueError(f"staged images in eval mode need an integer min_size[-1] and an integer max_size (got {self.min_size}, {self.max_size})")
        out_hw, _ = ops.resize_plan_dev(None, staged.in_hw, short, int(self.max_size))
        batch = ops.transform_batch_var(staged, out_hw, self.image_mean, self.image_std, hp, wp, out_dtype, channels_last)
        images = ImageList(batch, bounds)
        images.image_sizes_dev = out_hw
        return images, None

    def _forward_staged(self, staged, targets, canvas, out_dtype: torch.dtype, channels_last: bool):
        "Staged images over a fixed canvas: every input size is read on the device (module docstring)."
        from . import ops
        if not self.training and targets is None:
            return self._forward_staged_eval(staged, canvas, out_dtype, channels_last)
        if not self.training or not _is_packed(targets):
            raise ValueError("staged images (ops.StagedImages) are a training input and come with packed GT (ops.PackedGT)")
        if targets.B != staged.B or len(staged.hw) != staged.B:
            raise ValueError(f"packed GT of {targets.B} images for {len(staged.hw)} staged images in an arena of {staged.B}")
        (hp, wp), bounds = self._check_staged_canvas(canvas, staged, self.staged_bounds)
        # (training mode, packed GT: every installed augmentation acts here)
        crop = self._slot("crop", targets)
        if crop is not None:
            # a second staging pass: from here on ``staged`` is the arena of the windows and its sizes are the cropped ones
            staged, targets = ops.bbox_crop_staged(crop, staged, targets)
        ssr = self._slot("shift_scale_rotate", targets)
        if ssr is not None:
            # one more staging pass: the warped images at the same sizes, and the packed GT of the rows that survive
            staged, targets = ops.shift_scale_rotate_staged(ssr, staged, targets)
        hflip = self._slot("hflip", targets)
        flags = hflip.next_flags(staged.B, staged.device) if hflip is not None else None
        coef = self._color(staged, targets)
        jitter = self._jitter(targets)
        if jitter is not None:
            out_hw, ratios = jitter.next_sizes_dev(staged.in_hw, self.max_size)
        else:
            # (staged_short_side() is not None here: staged_bounds / the stager checked it)
            out_hw, ratios = ops.resize_plan_dev(None, staged.in_hw, self.staged_short_side(), int(self.max_size))
        # (launched whatever the ratios are: the host cannot know them; a ratio of 1 leaves a row bit for bit as it was)
        targets = ops.gt_flip_scale_packed_var(targets, staged.in_hw, ratios, flags)
        batch = ops.transform_batch_var(staged, out_hw, self.image_mean, self.image_std, hp, wp, out_dtype, channels_last, flags=flags,
                                        coef=coef)
        return ImageList(batch, bounds), targets

    def _crop_on_host(self, crop, images: List[Tensor], targets):
        """``crop`` for images that are not staged: the rectangles from the Python restatement (``crop.next_rects`` reads
        the boxes and the counter on the host: one synchronisation on CUDA), the images sliced (views) and the boxes shifted with
        torch -- one fp32 subtraction each, as the kernel does -- for target dicts and packed GT alike."""
        in_hw = [(int(im.shape[-2]), int(im.shape[-1])) for im in images]
        boxes, _, put = _gt_rows(targets, with_labels=False)
        rects = crop.next_rects(in_hw, boxes)
        images = [im[:, y0:y0 + ch, x0:x0 + cw] for im, (y0, x0, ch, cw) in zip(images, rects)]
        shifted = []
        for bx, (y0, x0, _, _) in zip(boxes, rects):
            moved = (y0, x0) != (0, 0) and bx.shape[0] > 0
            shifted.append(bx - bx.new_tensor([x0, y0, x0, y0], dtype=torch.float32) if moved else bx)
        return images, put(shifted)

    def _shift_scale_rotate_on_host(self, ssr, images: List[Tensor], targets):
        """``ssr`` for images that are not staged: the coefficients from the Python restatement
        (``next_coefs`` reads the boxes and the counter on the host: one synchronisation on CUDA), the images warped with torch ops
        (``warp_image``) and the rows moved, clipped and dropped by ``warp_boxes`` -- for target dicts and packed GT alike."""
        in_hw = [(int(im.shape[-2]), int(im.shape[-1])) for im in images]
        boxes, labels, put = _gt_rows(targets, with_labels=True)
        coefs = ssr.next_coefs(in_hw, boxes)
        images = [ssr.warp_image(im, coefs.inv[b], coefs.applied[b]) for b, im in enumerate(images)]
        moved = ssr.warp_boxes(coefs, in_hw, boxes, labels, ssr.min_visibility)
        return images, put([bx for bx, _ in moved], [lb for _, lb in moved])

    @staticmethod
    def _u8_to_f32(images: List[Tensor]) -> List[Tensor]:
        """uint8 ``[3, h, w]`` images (planes or interleaved: what image decoders give) become fp32 in [0, 1] first -- ``float(v) / 255``,
        ``ops.images_u8_to_f32``: one HIP launch per 64 CUDA images, a true division on the CPU, the same bits -- and then take the
        paths below like any fp32 image.  All at once when the whole list is uint8, image by image in a mixed list."""
        u8 = [im.dtype == torch.uint8 and im.shape[0] == 3 for im in images]
        if not any(u8):
            return images
        from . import ops
        if all(u8):
            return ops.images_u8_to_f32(images)
        return [ops.images_u8_to_f32([im])[0] if u else im for im, u in zip(images, u8)]

    # -- whole transform -----------------------------------------------------------------
    def forward(self, images: List[Tensor], targets: Optional[List[Dict[str, Tensor]]] = None,
                out_dtype: Optional[torch.dtype] = None, channels_last: bool = False, canvas: Optional[Tuple[int, int]] = None):
        """``out_dtype`` / ``channels_last``: layout hints for the fused CUDA path (defaults: fp32, NCHW --
        what torchvision's transform returns); ignored by the PyTorch fallback.  ``targets`` may be packed GT (``ops.PackedGT``):
        its boxes are rescaled per image on the device (``rn_gt_scale_packed``) and a PackedGT comes back.  ``images`` may be staged
        images (``ops.StagedImages``) with ``canvas`` = the padded (Hp, Wp) to produce: the module docstring's last paragraph."""
        if _is_staged(images):
            return self._forward_staged(images, targets, canvas, out_dtype or torch.float32, channels_last)
        if canvas is not None:
            raise ValueError("canvas= goes with staged images (ops.StagedImages) only")
        images = list(images)
        packed = _is_packed(targets)
        if packed:
            if targets.B != len(images):
                raise ValueError(f"packed GT of {targets.B} images for {len(images)} images")
        elif targets is not None:
            targets = [dict(t) for t in targets]
        for im in images:
            if im.dim() != 3:
                raise ValueError(f"images is expected to be a list of 3d tensors of shape [C, H, W], got {tuple(im.shape)}")
        images = self._u8_to_f32(images)
        crop, ssr = self._slot("crop", targets), self._slot("shift_scale_rotate", targets)
        if crop is not None:
            images, targets = self._crop_on_host(crop, images, targets)
        if ssr is not None:
            images, targets = self._shift_scale_rotate_on_host(ssr, images, targets)
        if self._fusable(images):
            return self._forward_fused(images, targets, out_dtype or torch.float32, channels_last)
        flags = self._flips(images, targets)
        cj, bc = self._slot("color_jitter", targets), self._slot("brightness_contrast", targets)
        if cj is not None:
            # the same draw from the Python restatement, applied with torch ops (augment.apply_color_ops) to the raw image
            from .augment import apply_color_ops
            images = [apply_color_ops(im, fac, order) for im, (fac, order) in zip(images, cj.next_draw(len(images)))]
        if bc is not None:
            # likewise (augment.apply_brightness_contrast), behind the jitter's operations: the by-mean reference sees their result
            from .augment import apply_brightness_contrast
            ref = 1.0 if bc.brightness_by_max else None
            images = [apply_brightness_contrast(im, alpha, beta, ref) if applied else im
                      for im, (applied, alpha, beta) in zip(images, bc.next_draw(len(images)))]
        jitter = self._jitter(targets)
        shorts = bounds = None
        if jitter is not None:
            # the same draw from the Python restatement (CUDA images that are not fusable: the counter is read back, one synchronisation)
            in_hw = [(int(im.shape[-2]), int(im.shape[-1])) for im in images]
            shorts = jitter.draw_short(jitter.counter, len(images))
            jitter.next_sizes(in_hw, self.max_size, images[0].device)
            bounds = [jitter.bound(h, w, self.max_size) for h, w in in_hw]
        ratios, widths = [], []
        for i, im in enumerate(images):
            if im.dim() != 3:
                raise ValueError(f"images is expected to be a list of 3d tensors of shape [C, H, W], got {tuple(im.shape)}")
            tgt = targets[i] if (targets is not None and not packed) else None
            hw = (int(im.shape[-2]), int(im.shape[-1]))
            widths.append(float(hw[1]))
            if flags is not None:
                im, tgt = _flip_where(flags[i], im, tgt)
            im, tgt = self.resize(self.normalize(im), tgt, None if shorts is None else shorts[i])
            images[i] = im
            if packed:
                ratios.append(_ratios(hw, im.shape[-2:]))
            if tgt is not None:
                targets[i] = tgt
        if packed:
            from . import ops
            targets = _resize_packed(targets, ratios) if flags is None else ops.gt_flip_scale_packed(targets, widths, ratios, flags)
        if bounds is not None:
            return ImageList(self.batch_images(images, self._canvas(bounds)), bounds), targets
        sizes = [(int(im.shape[-2]), int(im.shape[-1])) for im in images]
        return ImageList(self.batch_images(images), sizes), targets

    def postprocess(self, result: List[Dict[str, Tensor]], image_shapes: List[Tuple[int, int]],
                    original_image_sizes: List[Tuple[int, int]]) -> List[Dict[str, Tensor]]:
        if self.training:
            return result
        for i, (pred, s, o) in enumerate(zip(result, image_shapes, original_image_sizes)):
            result[i]["boxes"] = resize_boxes(pred["boxes"], s, o)
        return result
