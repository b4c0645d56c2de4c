"""``CapturedTrainStep`` -- one whole train step (zero_grad -> transform -> conv stack -> K1-K3 -> backward -> bucketed
all-reduce -> SGD) captured in a hipGraph and replayed with ONE host call per step.

Why: the step is ~700 kernel launches.  Enqueued one by one from Python they cost 21-26 ms of host time against a GPU
step of ~30 ms (``bench.py``: ``host_enqueue_ms_per_step``), so every millisecond the kernels get faster moves the step
closer to being host-bound.  The library never synchronises with the host and every shape of a step is static once the
image sizes and the GT counts are known, so the launch sequence is captured once per (input signature) and replayed
(reference analogue: none -- the reference launches ~40 torch ops per image from a Python loop with 4 host syncs each,
``retinanet/losses.py:66-126``).

The step has ONE body, ``CapturedTrainStep._step``, and every kind of step is that body with other arguments:
  zero the gradients -> ``_forward`` (the net under autocast and ``losses.grad_prescale``; total = the sum of its two losses)
  -> ``_backward`` ((scaled) total.backward()) -> ``ddp.finish()`` -> ``accumulate`` -> ``apply_gradients`` -> ``advance`` -> the loss dict.
  * a gradient exchange (``ddp=``) replaces the optimizer's zero_grad by its own and adds the wait for the collectives (``finish``);
  * a segmented step (below, ``segmented=``) installs ``backbone.StageCuts`` for the forward pass and ``_backward`` then runs three
    stages, calling ``mark(i)`` after each: the eager step issues the finished buckets' all-reduces there, the capture also ends one
    graph and begins the next;
  * an accumulator (``accumulate=``) adds the gradients to its fp32 sums after the backward pass and moves its window after the
    optimizer; a micro step (``final=False``) is the same body without ``apply_gradients``;
  * ``apply_gradients(optimizer, scaler, source)`` is the one place that decides how the gradients reach the optimizer: through the
    scaler or not, from the source (the exchange's buckets or the accumulator: ``step_exchanged`` / ``step(grads=...)``) or from ``.grad``.
    ``model.SimpleTrainer``'s eager loop ends in the same function.

Rules the capture relies on (all true of this package; checked by ``tests/test_graph_gpu.py``):
  * no host synchronisation and no host->device copy from temporary host memory inside the step: the GT offsets come from
    ``ops.gt_offsets`` (cached per count tuple), canvas masks / anchors / zero pages from their caches -- the eager steps
    that precede the capture fill them;
  * every pointer the kernels receive is a static input buffer, a parameter / optimizer state, or memory allocated from
    the graph's private pool during capture (same address at every replay);
  * scalars passed by value (learning rate, momentum, weight decay) are part of the signature: a change re-captures.
    Optimizers with device-resident hyperparameters (``optim.MasterAdam`` / ``MasterAdamW`` and ``MasterSGD(capturable=True)``:
    ``_rn_device_hparams``) are the exception: their kernels read lr and the rest from device blocks, which ``sync_device_hparams()`` refreshes
    before every replay, so those values are left out of the signature and a per-step LR schedule replays one graph.
    The augmentations of the net's transform (``transform.AUGMENT_SLOTS``: ``net.transform.hflip``, ``scale_jitter``, ``color_jitter``,
    ``crop``, ``shift_scale_rotate``, ``brightness_contrast``), gradient clipping (``optimizer.grad_clip``, ``optim.GradClip``) and a
    weight average (``optimizer.weight_ema``, ``optim.WeightEMA``) are each keyed by the installed object alone: what they draw or
    compute happens inside the step and reads its settings, seed and counter from the object's device block (created by the first,
    eager, step), so eager steps and replays advance one counter, a new p, range or ``max_norm`` needs no capture, and a graph
    captured without an object is never replayed once one is installed, and the reverse; with none the key is the plain one.  With a
    ``scale_jitter`` the padded canvas depends on the image shapes alone, so one graph replays while the scales vary (the host-side
    draw from a ``min_size`` tuple makes nearly every batch a new signature).
    Gradient accumulation (``accumulate=optim.GradAccumulator``) is keyed by the installed object too, and the window position is NOT
    part of the key: it lives in the object's device block.  A signature then holds up to two graphs -- the micro step and the final
    step (``_Signature.steps``) -- each warmed by its own ``eager_steps`` eager calls; ``max_graphs`` still counts signatures.
    The bbox-safe random crop (``crop``) needs the image capacity mode (a ``ValueError`` says so): the rectangles are drawn inside
    the step from the staged GT and the windows copied into a second arena.  A batch no class holds runs eagerly with the crop drawn
    on the host.
    Shift / scale / rotate (``shift_scale_rotate``) needs both capacity modes (a ``ValueError`` says so): the rows that survive are
    packed on the device -- the GT counts change from replay to replay, which only packed GT can hold -- and the images are warped
    into another arena.  A batch no class holds runs eagerly with the draw on the host.

``__call__(images, targets)`` performs exactly one optimisation step and returns the loss dict (static tensors: read them
before the next call).  The first ``eager_steps`` calls with a new signature run eagerly (they are real steps and they warm
MIOpen's find, the caches and the optimizer state); the next one captures and replays.  At most ``max_graphs`` signatures
are kept (least recently used goes first); a capture that fails falls back to eager for that signature.

GT capacity mode (``gt_capacity="auto"`` or a list of classes): real detection data has a different number of boxes in every
image, so the exact target shapes make nearly every batch a new signature and training never reaches a replay.  With the mode on,
a batch is keyed by its capacity class -- the smallest class >= its largest per-image box count (``gt_capacity_class``) -- and
every call, eager ones included, first stages its GT into the entry's fixed-size buffers (``ops.gt_stage``: B x class rows, the
offsets written on the device); the step then runs on that ``ops.PackedGT``.  The GT kernels read each image's range from the
device offsets and take the host-side counts only as launch hints, for which the capacity is an upper bound
(``losses.RetinaNetLosses.forward_levels``).  A batch above the last class keeps the exact-shape key.

Image capacity mode (``image_capacity="auto"`` or a list of padded canvases; needs the GT capacity mode): real detection data has
images of hundreds of different sizes, and the transform bakes every image's address, input size and resized size into kernel
arguments, so again nearly every batch is a new signature.  With the mode on, a batch is keyed by its canvas class -- the first
listed canvas (Hp, Wp) that contains the batch's own padded canvas (``image_canvas_class``; host arithmetic on the image shapes) --
and its pixel class -- the smallest power of two >= its largest h x w, at least 2**16 (``image_pixel_class``) -- and every call,
eager ones included, first stages its images into the entry's fixed arena (``ops.image_stage``: B slots of 3 x pixel class fp32, the
sizes written on the device); the step then runs on that ``ops.StagedImages``.  The resize plan, the box rescale and the transform
kernel read every input size from device memory (``rn_resize_plan_dev``, ``rn_gt_flip_scale_packed_var``, ``rn_transform_batch_var``)
and write the class canvas.  The cost: the conv stack processes the class canvas whatever the batch's own canvas was; a finer class
list trades captures for compute.  A batch that fits no class -- or whose GT fits no capacity class -- keeps the exact-shape key
and path.  CUDA images, all fp32 ``[3, h, w]`` (copied: ``ops.image_stage``) or all uint8 ``[3, h, w]``, planes or interleaved (converted on the way in:
``ops.image_stage_u8``); the arena is fp32 either way, so both kinds of batch share one graph per class.

Inference (``CapturedPredict``, at the end of this file): ``net.predict(images)`` as one graph replay per batch, for batches whose image sizes
vary.  A batch is keyed by B, its canvas class and pixel class (the same ``image_capacity_classes`` / ``image_canvas_class`` / ``image_pixel_class``,
over the sizes after the resize to the fixed eval short side), the autocast dtype and the memory format; every call stages its images into the
key's arena and runs ``Retinanet.predict_staged`` -- the eval-mode staged transform, the conv stack under ``no_grad``, the anchors of the canvas,
``rn_detect_levels`` on the device sizes and ``rn_detect_finish_var``, which maps the boxes back to the original sizes and gathers everything the
host reads into one block -- eagerly for the first ``eager_calls`` calls of a key and as a captured linear graph afterwards, followed by ONE
device-to-host copy and one wait.  A captured pass bakes in the folded BatchNorm weights (``backbone._folded``), so the predictor stamps the
weights (``norm.RAW_WRITES`` plus every parameter's and buffer's ``(data_ptr, _version)``) and drops every graph when the stamp moves; an image with
more candidates than the fixed ``max_candidates`` reruns its batch eagerly with the worst case; a batch no class holds goes to plain ``net.predict``.
"""
import ctypes as C
import math
import os
import logging
import time
from collections import OrderedDict
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import ops
from ._lib import check, lib
from .norm import RAW_WRITES, note_raw_write
from .transform import augments_of

_log = logging.getLogger(__name__)

GT_CAPACITY_CLASSES = (8, 32, 128, 512)      # gt_capacity="auto"


def gt_capacity_classes(value) -> Optional[Tuple[int, ...]]:
    """``CapturedTrainStep(gt_capacity=...)`` -> the capacity classes: None (off), "auto" (``GT_CAPACITY_CLASSES``) or a strictly
    increasing sequence of positive ints; ValueError for anything else."""
    if value is None:
        return None
    if isinstance(value, str):
        if value == "auto":
            return GT_CAPACITY_CLASSES
        raise ValueError(f"gt_capacity: expected None, 'auto' or increasing positive ints, got {value!r}")
    try:
        classes = tuple(value)
    except TypeError:
        raise ValueError(f"gt_capacity: expected None, 'auto' or increasing positive ints, got {value!r}") from None
    if not classes or any(isinstance(c, bool) or not isinstance(c, int) or c <= 0 for c in classes) \
            or any(b <= a for a, b in zip(classes, classes[1:])):
        raise ValueError(f"gt_capacity: expected None, 'auto' or increasing positive ints, got {value!r}")
    return classes


def gt_capacity_class(counts: Sequence[int], classes: Sequence[int]) -> Optional[int]:
    "The smallest class >= max(counts) (0 for no counts), or None when the largest count exceeds the last class."
    most = max((int(c) for c in counts), default=0)
    for c in classes:
        if most <= c:
            return int(c)
    return None


_UNSET = object()                           # "not computed by the caller" (None is a value: no class)
IMAGE_PIXEL_CLASS_FLOOR = 2 ** 16           # the smallest pixel class (an arena slot is 3 x the class fp32)


def _ceil_to(v, d: int) -> int:
    return int(math.ceil(float(v) / d) * d)           # (transform.GeneralizedRCNNTransform._canvas rounds the same way)


def image_capacity_classes(value, transform=None) -> Optional[Tuple[Tuple[int, int], ...]]:
    """``CapturedTrainStep(image_capacity=...)`` -> the canvas classes: None (off), "auto" or a non-empty sequence of distinct (Hp, Wp)
    pairs of positive ints, each a multiple of the transform's ``size_divisible``; ValueError for anything else.  "auto" is derived
    from ``transform``: with m = max(min_size) and M = max_size, both rounded up to ``size_divisible``, [(m, M), (M, m), (M, M)] with
    duplicates removed -- landscape, portrait, mixed.  Without a transform (``SimpleTrainer``'s constructor) "auto" stays "auto" and a
    list is checked for everything but divisibility."""
    if value is None:
        return None
    msg = f"image_capacity: expected None, 'auto' or distinct (Hp, Wp) pairs of positive ints, got {value!r}"
    if isinstance(value, str):
        if value != "auto":
            raise ValueError(msg)
        if transform is None:
            return "auto"
        d = int(transform.size_divisible)
        m, M = _ceil_to(max(transform.min_size), d), _ceil_to(transform.max_size, d)
        return tuple(dict.fromkeys([(m, M), (M, m), (M, M)]))
    try:
        classes = tuple(tuple(c) for c in value)
    except TypeError:
        raise ValueError(msg) from None
    if not classes or any(len(c) != 2 or any(isinstance(v, bool) or not isinstance(v, int) or v <= 0 for v in c) for c in classes) \
            or len(set(classes)) != len(classes):
        raise ValueError(msg)
    if transform is not None:
        d = int(transform.size_divisible)
        if any(v % d for c in classes for v in c):
            raise ValueError(f"image_capacity: every canvas side must be a multiple of the transform's size_divisible ({d}), got {value!r}")
    return tuple((int(h), int(w)) for h, w in classes)


def image_canvas_class(canvas: Sequence[int], classes: Sequence[Tuple[int, int]]) -> Optional[Tuple[int, int]]:
    "The first listed class that contains the padded canvas (H, W), or None when none does."
    for hp, wp in classes:
        if canvas[0] <= hp and canvas[1] <= wp:
            return (int(hp), int(wp))
    return None


def image_pixel_class(in_hw: Sequence[Tuple[int, int]]) -> int:
    "The smallest power of two >= the largest h x w of the batch, at least ``IMAGE_PIXEL_CLASS_FLOOR``."
    most = max((int(h) * int(w) for h, w in in_hw), default=0)
    return max(IMAGE_PIXEL_CLASS_FLOOR, 1 << max(most - 1, 0).bit_length())


def _all_u8(images) -> bool:
    "Every image a CUDA uint8 ``[3, h, w]`` tensor: what ``ops.image_stage_u8`` stages (planes, interleaved or any other strides)."
    return len(images) > 0 and all(im.is_cuda and im.dim() == 3 and im.shape[0] == 3 and im.dtype == torch.uint8 for im in images)


def _stageable(tr, images) -> bool:
    """A batch the staged path takes: images the fused transform takes (fp32, ``ops.image_stage``), or -- under the same conditions on
    the transform -- an all-uint8 batch (``ops.image_stage_u8`` converts it on the way into the same fp32 arena)."""
    images = list(images)
    return tr._fusable(images) or (_all_u8(images) and tr._fused_config())


def _stage(images, staged, bounds) -> None:
    "This batch's images into the entry's arena: fp32 images are copied, uint8 ones converted (classed batches are all one or the other)."
    (ops.image_stage_u8 if images[0].dtype == torch.uint8 else ops.image_stage)(images, staged, bounds=bounds)


def _gt_counts(targets) -> List[int]:
    return [int(t["boxes"].reshape(-1, 4).shape[0]) for t in targets]


def _device_of(images) -> torch.device:
    return images.device if isinstance(images, ops.StagedImages) else images[0].device


def _net_targets(targets):
    "What the step hands to ``Retinanet.forward``: packed GT as it is, a copy of each target dict otherwise."
    return targets if isinstance(targets, ops.PackedGT) else [dict(t) for t in targets]


class _Entry:
    "One kind of step of one signature: the calls seen so far and, once captured, the graph(s), their static inputs and the losses they write."
    __slots__ = ("calls", "failed", "graph", "segments", "bucket_ids", "pool", "images", "targets", "losses", "match_state", "atss_ws")

    def __init__(self):
        self.calls, self.failed = 0, False
        # the ATSS matcher's workspaces (``ops.use_atss_workspaces``): allocated and zero-filled by this entry's eager steps, read by
        # its capture and replays, which leave the conflict table zero -- the graph never clears it
        self.atss_ws = {}
        self.clear()

    def clear(self) -> None:
        "Nothing captured (the initial state, and what a failed capture goes back to): drops the graphs and their private memory pool."
        self.graph = self.segments = self.bucket_ids = self.pool = None
        self.images = self.targets = self.losses = self.match_state = None

    def hold_inputs(self, images, targets) -> None:
        """The static inputs every replay reads (copies of this call's; packed GT and staged images are static already) and the fused
        loss kernel's state words: zero-filled here, OUTSIDE the capture, and owned by this entry (``ops.use_match_state``)."""
        self.images = images if isinstance(images, ops.StagedImages) else [im.clone() for im in images]
        self.targets = targets if isinstance(targets, ops.PackedGT) else \
            [{k: (v.clone() if isinstance(v, Tensor) else v) for k, v in t.items()} for t in targets]
        self.match_state = ops.new_match_state(_device_of(images))


class _Signature:
    "What one input signature owns: the GT staging buffers and the image arena of the capacity modes and an ``_Entry`` per kind of step."
    __slots__ = ("packed", "staged", "steps")

    def __init__(self, packed=None, staged=None):
        self.packed = packed      # GT capacity mode: ops.PackedGT (B x class rows), staged before every call of either kind
        self.staged = staged      # image capacity mode: ops.StagedImages (B slots of 3 x pixel class), staged the same way
        self.steps = {}           # final -> _Entry.  Without gradient accumulation every step is final


class MemsetNodeInGraph(RuntimeError):
    pass


class CaptureUnwindError(RuntimeError):
    "A failed capture could not be unwound: some stream of this process is still in capture mode (see ``_device_usable``)."


def _device_usable(dev) -> Optional[BaseException]:
    """After a failed capture: can this process still allocate, launch and run autograd on ``dev``?  A failure raised by the autograd
    engine's worker thread in the middle of a captured backward pass leaves streams the engine pulled into the capture (the legacy
    stream, through AccumulateGrad nodes created by an eager step) in capture mode on ROCm 7 even after the capture has been ended;
    every later allocation in that thread then fails with hipErrorStreamCaptureImplicit.  -> the exception the probe met, or None."""
    try:
        t = torch.ones(8, device=dev, requires_grad=True)
        (t * 2.0).sum().backward()                 # (runs on the engine's device thread)
        torch.cuda.synchronize(dev)
        return None
    except Exception as exc:                       # noqa: BLE001
        return exc


LAST_CENSUS: Dict[str, int] = {}          # node counts of the graphs captured so far in this process (bench.py reports them)


_WARNED_NO_HANDLE = False


def _new_graph() -> "torch.cuda.CUDAGraph":
    try:
        return torch.cuda.CUDAGraph(keep_graph=True)          # (keeps the hipGraph_t for the node census below)
    except TypeError:
        return torch.cuda.CUDAGraph()


def _uninspectable(g) -> None:
    """The raw hipGraph_t is not available (a torch without ``CUDAGraph(keep_graph=True)``): no node census, no memset repair.  On ROCm
    that is exactly the case the repair exists for, so the capture is REFUSED there (the step runs eagerly: slower, never wrong);
    elsewhere it is logged once."""
    global _WARNED_NO_HANDLE
    if getattr(torch.version, "hip", None):
        raise MemsetNodeInGraph("this torch cannot hand out the captured hipGraph_t (CUDAGraph(keep_graph=True) is missing): memset nodes "
                                "of third-party libraries can be neither counted nor replaced, and their replays are not trusted on ROCm")
    if not _WARNED_NO_HANDLE:
        _WARNED_NO_HANDLE = True
        _log.warning("captured graph cannot be inspected (no raw graph handle): node census and memset-node repair skipped")


def _repair_memset_nodes(g) -> None:
    """(Repairs, then refuses what is left.)  A captured step must not hold a MEMSET node: on ROCm 7.0 the memset nodes of a replayed hipGraph write garbage once the
    process has synchronised with the device and enqueued other blit work (round 4: K2's 32-byte ``num_fg`` clear scaled every loss
    after bench.py's warm-up synchronisation by 1 / garbage).  This package issues no memset (kernels clear what needs clearing,
    ``layers.FeaturePyramid._conv_own_bias``); MIOpen still does for some weight-gradient algorithms at some shapes -- such a step
    is refused here and runs eagerly (``CapturedTrainStep.__call__`` catches the exception)."""
    raw = getattr(g, "raw_cuda_graph", None)
    try:
        handle = raw() if raw is not None else None
    except Exception:                    # noqa: BLE001 -- graph not kept (older torch): nothing to inspect
        handle = None
    if handle:
        counts = (C.c_int64 * 4)()
        check(lib.rn_hipgraph_node_census(C.c_void_p(int(handle)), counts), "rn_hipgraph_node_census")
        LAST_CENSUS.update(kernel=LAST_CENSUS.get("kernel", 0) + int(counts[0]), memset=LAST_CENSUS.get("memset", 0) + int(counts[1]),
                           memcpy=LAST_CENSUS.get("memcpy", 0) + int(counts[2]), other=LAST_CENSUS.get("other", 0) + int(counts[3]))
        if counts[1] and not os.environ.get("RN_GRAPH_KEEP_MEMSET_NODES"):
            # the repair: each memset node becomes a kernel node with the same parameters, dependencies and dependents
            n = C.c_int64(0)
            check(lib.rn_hipgraph_replace_memset_nodes(C.c_void_p(int(handle)), C.byref(n)), "rn_hipgraph_replace_memset_nodes")
            LAST_CENSUS["memset_replaced"] = LAST_CENSUS.get("memset_replaced", 0) + int(n.value)
            check(lib.rn_hipgraph_node_census(C.c_void_p(int(handle)), counts), "rn_hipgraph_node_census")
        if counts[1]:
            raise MemsetNodeInGraph(f"the captured step holds {counts[1]} memset node(s) next to {counts[0]} kernels (a third-party "
                                    f"library cleared a buffer with hipMemsetAsync); replays of such a graph are not trusted on this ROCm")
    else:
        _uninspectable(g)
    inst = getattr(g, "instantiate", None)
    if handle and inst is not None:
        inst()


def retinanet_stage_of(name: str) -> int:
    """Backward stage of a ``Retinanet`` parameter (``BucketedGradAllReduce(stage_of=...)``): 0 = head + FPN, 1 = layer4 + layer3,
    2 = layer2 .. stem -- the order in which the staged backward pass finishes their gradients."""
    if name.startswith("backbone.backbone.layer4") or name.startswith("backbone.backbone.layer3"):
        return 1
    if name.startswith("backbone."):
        return 2
    return 0


def apply_gradients(optimizer, scaler, source=None) -> None:
    """How the gradients of a finished backward pass reach the optimizer -- decided here and nowhere else.  ``source``: who holds them
    when ``.grad`` is not the place to look -- a gradient exchange (``parallel.BucketedGradAllReduce``, after ``finish()``), an
    ``optim.GradAccumulator``, or None.  A scaler takes its found_inf from the source (``ExchangeGradScaler.step_exchanged``) and is
    updated; the master optimizers step on the source's fp32 views (``step(grads=source.grad_views())``); any other optimizer, and
    every optimizer without a source, reads ``.grad``."""
    if scaler is not None:
        if source is not None:
            scaler.step_exchanged(optimizer, source)
        else:
            scaler.step(optimizer)
        scaler.update()
    elif source is not None and getattr(optimizer, "_rn_master_weights", False):
        optimizer.step(grads=source.grad_views())
    else:
        optimizer.step()


class CapturedTrainStep:
    def __init__(self, net, optimizer, ddp=None, amp_dtype: Optional[torch.dtype] = torch.bfloat16, eager_steps: int = 2,
                 max_graphs: int = 4, enabled: bool = True, segmented: Optional[bool] = None, scaler=None, gt_capacity=None,
                 accumulate=None, image_capacity=None):
        """``segmented`` (default: on whenever gradients are exchanged): the step with a gradient exchange as FOUR linear hipGraphs --
        forward + head / FPN backward | layer4, layer3 backward | layer2 .. stem backward | optimizer -- with the finished buckets'
        all-reduces issued EAGERLY on the process group's communication stream between the replays and the wait for them in
        front of the last segment.  Why not one graph: torch's process group runs the collectives on its own stream, a capture
        turns that into forked graph branches, and ROCm replays such a graph slower than Python enqueues the same kernels
        (DESIGN.md section 6); why not eager: ~20 ms of host time per 25 ms step.  The backward pass is cut at C3 / C4 / C5
        (``backbone.StageCuts``) and run as separate autograd calls, so each segment's capture begins and ends on this thread.
        ``gt_capacity``: None (default: the exact target shapes are part of the signature), "auto" (classes ``GT_CAPACITY_CLASSES``)
        or increasing positive ints -- the GT capacity mode of the module docstring.
        ``accumulate``: None (default) or an ``optim.GradAccumulator`` -- gradient accumulation.  A call is then a micro step (forward,
        backward, accumulate) or a final step (the same, then clip + optimizer step on the accumulators): ``stepper(images, targets,
        final=...)``, the default being the accumulator's own count (every ``accumulate.n``-th call is final).  Single process only.
        ``image_capacity``: None (default: the exact image shapes are part of the signature), "auto" (three canvases derived from the
        net's transform) or a list of padded canvases (Hp, Wp) -- the image capacity mode of the module docstring.  Needs
        ``gt_capacity``: real data varies in both, and the staged path rescales packed GT only."""
        self.gt_capacity = gt_capacity_classes(gt_capacity)
        self.image_capacity = image_capacity_classes(image_capacity, getattr(net, "transform", None))
        if self.image_capacity is not None:
            if self.gt_capacity is None:
                raise ValueError("image_capacity needs gt_capacity as well (\"auto\" or a class list): the staged path rescales packed GT only")
            if self.image_capacity == "auto":
                raise ValueError("image_capacity='auto' needs a net with a transform to derive the canvases from")
        if accumulate is not None:
            from .optim import GradAccumulator
            if not isinstance(accumulate, GradAccumulator):
                raise TypeError(f"accumulate must be an optim.GradAccumulator, not {type(accumulate).__name__}")
            if ddp is not None:
                raise ValueError("gradient accumulation is single-process only: accumulate= cannot be combined with a gradient exchange "
                                 "(ddp=); skipping the exchange on micro steps is not implemented")
            if not getattr(optimizer, "_rn_master_weights", False):
                raise ValueError(f"accumulate= needs an optimizer that steps on fp32 gradients handed to step(grads=...) "
                                 f"(optim.MasterSGD / MasterAdam / MasterAdamW), not {type(optimizer).__name__}")
            if scaler is not None and not hasattr(scaler, "step_exchanged"):
                raise ValueError("with accumulate= the loss scaler must be a parallel.ExchangeGradScaler: found_inf has to cover every "
                                 "micro-batch of the window, which the stock GradScaler's look at param.grad does not")
        self.accumulate = accumulate
        self.net, self.optimizer, self.ddp = net, optimizer, ddp
        # fp16 autocast: a torch.amp.GradScaler (the reference's precision=16 run is native AMP, demo.ipynb).  Its scale / growth
        # tracker are device tensors and optim.MasterSGD takes grad_scale / found_inf on the device, so scale -> backward -> step ->
        # update records into the graph like the rest of the step.  Under a gradient exchange: parallel.ExchangeGradScaler.
        self.scaler = scaler
        if scaler is not None and ddp is not None and not hasattr(scaler, "step_exchanged"):
            raise ValueError("under a gradient exchange the loss scaler must be a parallel.ExchangeGradScaler: found_inf has to come "
                             "from the exchanged buckets, or one rank skips a step the others take")
        self.segmented = (ddp is not None) if segmented is None else (bool(segmented) and ddp is not None)
        if self.segmented:
            ddp.deferred = True
        self.amp_dtype = amp_dtype
        self.eager_steps, self.max_graphs, self.enabled = max(int(eager_steps), 1), int(max_graphs), enabled
        self._entries: "OrderedDict[tuple, _Signature]" = OrderedDict()
        self.replays = 0          # steps served by a graph replay (diagnostics / tests)
        self.captures = 0

    # -- the step itself (identical in eager mode and under capture) -------------------------------------------------
    def _forward(self, images, targets) -> Tuple[Dict[str, Tensor], Tensor]:
        "The forward pass under autocast -> (the net's loss dict, the sum of the two losses)."
        from .losses import grad_prescale, scaler_prescale
        # fp16: the loss kernel multiplies the GradScaler's scale into its gradients before it rounds them to fp16 (losses.grad_prescale)
        dev = _device_of(images)
        pre = scaler_prescale(self.scaler, dev) if dev.type == "cuda" else None
        with torch.autocast(dev.type, dtype=self.amp_dtype, enabled=self.amp_dtype is not None, cache_enabled=False), \
                grad_prescale(pre):
            losses = self.net(images if isinstance(images, ops.StagedImages) else list(images), _net_targets(targets))
            total = losses["classification_loss"] + losses["regression_loss"]
        return losses, total

    def _backward(self, total: Tensor, cuts, mark) -> None:
        """The backward pass: one autograd call, or -- ``cuts``: the ``backbone.StageCuts`` the forward pass filled -- three stages, with
        ``mark(i)`` after stage i's kernels have been enqueued (the buckets completed so far may be exchanged)."""
        # fp16: the scaled loss -- every later stage starts from scaled leaf gradients
        (self.scaler.scale(total) if self.scaler is not None else total).backward()
        if cuts is None:
            return
        mark(0)                                                   # stage 0 was head + FPN; gradients of the cut leaves
        pairs = cuts.pairs                                        # [(C3, leaf), (C4, leaf), (C5, leaf)] in forward order
        # C3 / C4 join the data gradients of their consumers in the receiver's GEMM (pwconv._GradJoin); the FPN lateral's gradient was
        # produced in ANOTHER autograd pass (stage 0), so it is handed to the join here: the receiver accumulates into it (addmm_) and
        # autograd ASSIGNS the result to the leaf -- no 137 / 69 MB add per cut
        for _, leaf in pairs:
            j = getattr(leaf, "_rn_join", None)
            if j is not None and j._has_receiver and not j.recv_done and j.full is None and leaf.grad is not None:
                j.full, leaf.grad = leaf.grad, None
        for out, leaf in reversed(pairs[1:]):                     # stage 1: layer4, then layer3 (each adds to the leaf below it)
            if leaf.grad is not None:
                out.backward(leaf.grad)
                leaf.grad = None
        mark(1)
        if pairs and pairs[0][1].grad is not None:                # stage 2: layer2 .. stem
            pairs[0][0].backward(pairs[0][1].grad)
            pairs[0][1].grad = None
        mark(2)

    def _step(self, images: Sequence[Tensor], targets: Sequence[Dict[str, Tensor]], final: bool = True, mark=None) -> Dict[str, Tensor]:
        """One step.  ``final`` (gradient accumulation only; without it every step is final): False = a micro step, which stops
        short of the optimizer.  ``mark`` (segmented steps only): called with i = 0, 1, 2 after each backward stage and with 3 after
        the optimizer; the default issues the finished buckets' all-reduces, the segmented capture ends and begins its graphs in it.
        ``ddp.finish()`` -- the wait for the exchange -- runs between mark(2) and the optimizer, outside any capture."""
        net, opt, ddp, acc = self.net, self.optimizer, self.ddp, self.accumulate
        if ddp is not None:
            ddp.zero_grad()
        else:
            opt.zero_grad(set_to_none=True)
        cuts = None
        if self.segmented:
            from .backbone import StageCuts
            if mark is None:
                mark = lambda i: ddp.issue_ready() if i < 3 else None
            trunk = net.backbone.backbone
            cuts = trunk.stage_cuts = StageCuts()
        try:
            losses, total = self._forward(images, targets)
        finally:
            if cuts is not None:
                trunk.stage_cuts = None
        self._backward(total, cuts, mark)
        if ddp is not None:
            ddp.finish()
        if acc is not None:
            # the UNDIVIDED loss went backward (and goes to the caller): the 1 / n of the window is the accumulate kernel's weight
            acc.accumulate(p for g in opt.param_groups for p in g["params"])
        if final:
            # (under a scaler, found_inf comes from the source: the exchanged buckets -- the same on every rank -- or the whole window)
            apply_gradients(opt, self.scaler, ddp if ddp is not None else acc)
        if acc is not None:
            acc.advance(final)                                    # (final: the window reset)
        if cuts is not None:
            mark(3)
        return {"classification_loss": losses["classification_loss"].detach(), "regression_loss": losses["regression_loss"].detach(),
                "loss": total.detach()}

    def _augments(self) -> Dict[str, object]:
        "The augmentations installed in the net's transform, by slot name, in ``AUGMENT_SLOTS`` order (a net without a transform: none)."
        return dict(augments_of(getattr(self.net, "transform", None)))

    def _capacity_of(self, targets) -> Optional[int]:
        "The batch's capacity class, or None (mode off, or a count above the last class: exact-shape keying)."
        return None if self.gt_capacity is None else gt_capacity_class(_gt_counts(targets), self.gt_capacity)

    def _image_class_of(self, images, targets, cap=_UNSET) -> Optional[Tuple[Tuple[int, int], int, List[Tuple[int, int]]]]:
        """The batch's (canvas class, pixel class, per-image resized bounds), or None: mode off, GT above its last class (the staged
        path takes packed GT; ``cap``: the batch's GT class when the caller has it), images the fused transform does not take, a short
        side drawn on the host, or a canvas no class contains -- exact-shape keying then.  Host arithmetic on the image shapes; nothing
        synchronises.  ``__call__`` computes it ONCE per step and hands it to ``_signature`` and, as ``StagedImages.bounds``, to the
        transform."""
        if self.image_capacity is None or (self._capacity_of(targets) if cap is _UNSET else cap) is None:
            return None
        tr = self.net.transform
        if not _stageable(tr, images) or ("scale_jitter" not in self._augments() and tr.staged_short_side() is None):
            return None
        in_hw = [(int(im.shape[-2]), int(im.shape[-1])) for im in images]
        bounds = tr.staged_bounds(in_hw)
        canvas = image_canvas_class(tr._canvas(bounds), self.image_capacity)
        return None if canvas is None else (canvas, image_pixel_class(in_hw), bounds)

    def _signature(self, images, targets, cap=_UNSET, icls=_UNSET) -> tuple:
        "``cap`` / ``icls``: the batch's GT class and image class when the caller has computed them (``__call__``); else computed here."
        if getattr(self.optimizer, "_rn_device_hparams", False):
            # (optim.MasterAdam / MasterAdamW / MasterSGD(capturable=True): the kernels read their hyperparameters from device blocks that
            # sync_device_hparams() refreshes before every replay -- a per-step LR schedule keeps one graph)
            groups = ("device_hparams", len(self.optimizer.param_groups))
        else:
            groups = tuple((g.get("lr"), g.get("momentum"), g.get("weight_decay"), g.get("dampening"), g.get("nesterov"))
                           for g in self.optimizer.param_groups)
        if cap is _UNSET:
            cap = self._capacity_of(targets)
        if icls is _UNSET:
            icls = self._image_class_of(images, targets, cap)
        if icls is not None:
            # (the entry's arena: B slots.  The dtype is the ARENA's: staging happens outside the graph, so a uint8 batch --
            # ``ops.image_stage_u8`` -- and an fp32 batch of the same classes share one graph)
            ims = ("img_cap", len(images), icls[0], icls[1], torch.float32, images[0].device)
        else:
            ims = tuple((tuple(im.shape), im.dtype, im.device) for im in images)
        if cap is not None:
            tgs = ("gt_cap", cap)          # (the entry's packed buffers are B x cap rows; B is in the image shapes)
        else:
            tgs = tuple(tuple(sorted((k, tuple(v.shape), v.dtype) for k, v in t.items() if isinstance(v, Tensor))) for t in targets)
        # Everything below is keyed by the installed OBJECT, never by its settings: the transform's augmentations, the global-norm clip
        # (optim.GradClip), the accumulator (optim.GradAccumulator) and the weight average (optim.WeightEMA) all do their work inside
        # the step and read what they need -- p, seed, counter, ranges, max_norm, the window position, the decay -- from the object's
        # device block.  A new setting therefore replays the same graph, installing, removing or swapping an object re-captures, and
        # the key keeps the object (and with it the block) alive as long as a graph reads it.  The flip has its place in the base key,
        # None when there is none; the accumulator, the average and the other slots (in ``AUGMENT_SLOTS`` order, tagged with their
        # names) follow only when installed, so without them the key is the base key.
        aug = self._augments()
        mode = tuple(m.training for m in self.net.modules())
        frozen = tuple(p.requires_grad for p in self.net.parameters())       # (freezing / unfreezing layers changes the launch sequence)
        key = (ims, tgs, groups, hash(mode), hash(frozen), self.amp_dtype, aug.pop("hflip", None), getattr(self.optimizer, "grad_clip", None))
        if self.accumulate is not None:
            key += (self.accumulate,)
        ema = getattr(self.optimizer, "weight_ema", None)
        if ema is not None:
            key += (("weight_ema", ema),)
        key += tuple(aug.items())
        # the matcher's launches are part of the step: another kind or another topk is another graph.  The default ("iou") adds nothing.
        crit = getattr(getattr(self.net, "retinanet_head", None), "losses", None)
        # "tal" carries its own topk and both exponents: they are baked into its launches.
        if getattr(crit, "matcher", "iou") == "tal":
            key += (("matcher", "tal", int(crit.tal_topk), int(crit.tal_alpha), int(crit.tal_beta)),)
        elif getattr(crit, "matcher", "iou") != "iou":
            key += (("matcher", crit.matcher, int(crit.atss_topk)),)
        # so is the box loss: an IoU kind adds ops.box_iou_loss's launches, and its weight is baked into them.  "smooth_l1" adds nothing.
        if getattr(crit, "box_loss", "smooth_l1") != "smooth_l1":
            key += (("box_loss", crit.box_loss, float(crit.box_loss_weight)),)
        # and the class loss: "qfl" adds ops.quality_focal_loss's launches, and its beta is baked into them and into K3's.  "focal" adds nothing.
        if getattr(crit, "cls_loss", "focal") != "focal":
            key += (("cls_loss", crit.cls_loss, float(crit.qfl_beta)),)
        return key

    def _capture_segments(self, e: _Entry, images, targets) -> None:
        "Four linear graphs sharing one memory pool; the exchange calls between them run eagerly, here as at every replay."
        dev = _device_of(images)
        e.hold_inputs(images, targets)
        e.pool = torch.cuda.graph_pool_handle()
        e.segments, e.bucket_ids = [], []
        ddp = self.ddp
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        state = {"g": None, "open": False}

        def begin():
            state["g"] = _new_graph()
            state["g"].capture_begin(pool=e.pool, capture_error_mode="thread_local")
            state["open"] = True

        def mark(i):
            state["g"].capture_end()
            state["open"] = False
            _repair_memset_nodes(state["g"])
            e.segments.append(state["g"])
            e.bucket_ids.append(ddp.issue_ready() if i < 3 else [])       # eager: the collectives of the buckets this segment completed
            if i < 2:
                begin()
            # (i == 2: ddp.finish() runs next -- eager: the compute stream waits for the communication stream -- and begins the
            # optimizer's segment, see finish_then_begin below)

        with ops.use_match_state(e.match_state), ops.use_atss_workspaces(e.atss_ws), torch.cuda.stream(side):
            orig_finish = ddp.finish

            def finish_then_begin():
                orig_finish()
                begin()
            ddp.finish = finish_then_begin
            try:
                begin()
                e.losses = self._step(e.images, e.targets, mark=mark)
            except BaseException:
                # a failure inside an open segment (a MIOpen / check() error in forward or backward) must END that capture before
                # anything else touches the device from this thread: torch.cuda.graph.__exit__ does this for the one-graph path, the
                # hand-driven begin / mark pair has to do it itself.  Then the half-built segments are reset (the caller clears the entry).
                if state["open"]:
                    # the autograd engine may have pulled OTHER streams into the capture (an AccumulateGrad node created by an eager
                    # step lives on the stream of that step: the engine makes that stream wait for the capturing one and joins it
                    # back at the end of the pass -- which a failure in the middle of the pass skips).  Join what can be joined, or
                    # the capture ends "unjoined" and that stream stays in capture mode.
                    for other in {torch.cuda.default_stream(dev), torch.cuda.current_stream(dev)} - {side}:
                        try:
                            side.wait_stream(other)
                        except Exception:            # noqa: BLE001
                            pass
                    try:
                        state["g"].capture_end()
                    except Exception:                # noqa: BLE001 -- the capture is already invalid: ending it may raise again
                        pass
                    state["open"] = False
                for g in e.segments + [state["g"]]:
                    try:
                        if g is not None:
                            g.reset()
                    except Exception:                # noqa: BLE001
                        pass
                state["g"] = None
                raise
            finally:
                ddp.finish = orig_finish
                torch.cuda.current_stream(dev).wait_stream(side)
        self.captures += 1

    def _replay_segments(self, e: _Entry) -> None:
        ddp = self.ddp
        for i in range(3):
            e.segments[i].replay()
            ddp.issue(e.bucket_ids[i])
        ddp.finish()
        e.segments[3].replay()

    def _capture(self, e: _Entry, images, targets, final: bool = True) -> None:
        if self.segmented:
            return self._capture_segments(e, images, targets)
        e.hold_inputs(images, targets)
        torch.cuda.synchronize()
        g = _new_graph()
        with ops.use_match_state(e.match_state), ops.use_atss_workspaces(e.atss_ws), torch.cuda.graph(g, capture_error_mode="thread_local"):
            e.losses = self._step(e.images, e.targets, final)
        _repair_memset_nodes(g)
        e.graph = g
        self.captures += 1

    def __call__(self, images: Sequence[Tensor], targets: Sequence[Dict[str, Tensor]], final: Optional[bool] = None) -> Dict[str, Tensor]:
        """``final`` (gradient accumulation only): whether this call completes the window and steps the optimizer; None = the
        accumulator's own count (every ``n``-th call since the last final one).  Without ``accumulate=`` every call is a whole step."""
        acc = self.accumulate
        if acc is None:
            if final is not None and not final:
                raise ValueError("final=False needs a CapturedTrainStep(accumulate=optim.GradAccumulator(...))")
            final = True
        elif final is None:
            final = acc.next_is_final()
        final = bool(final)
        if not self.enabled or not images or not images[0].is_cuda:
            return self._step(images, targets, final)
        aug = self._augments()
        ssr = aug.get("shift_scale_rotate")
        if ssr is not None and (self.image_capacity is None or self.gt_capacity is None):
            raise ValueError("a shift / scale / rotate (net.transform.shift_scale_rotate) warps every image and drops boxes from step to "
                             "step: CapturedTrainStep needs gt_capacity= and image_capacity= for it -- the staged path draws and applies "
                             "it on the device; without them call the net directly (it is then drawn on the host)")
        cap = self._capacity_of(targets)
        icls = self._image_class_of(images, targets, cap)          # (once per step: the key, the arena and the transform's bounds)
        if "crop" in aug:
            if self.image_capacity is None:
                raise ValueError("a bbox-safe random crop (net.transform.crop) changes every image's size from step to step: "
                                 "CapturedTrainStep needs image_capacity= (and gt_capacity=) for it -- the staged path draws the crop on "
                                 "the device; without them call the net directly (the crop is then drawn on the host)")
            if icls is None:
                # a batch no class holds: the crop is drawn on the host there (a synchronisation), which no capture can contain
                return self._step(images, targets, final)
        if ssr is not None:
            if icls is None or cap is None:
                # a batch no class holds: drawn on the host there (a synchronisation), which no capture can contain
                return self._step(images, targets, final)
        key = self._signature(images, targets, cap, icls)
        dev = images[0].device
        sig = self._entries.get(key)
        if sig is None:
            sig = self._entries[key] = _Signature(ops.PackedGT.empty(len(images), cap, dev) if cap is not None else None,
                                                  ops.new_image_arena(len(images), icls[1], dev, icls[0]) if icls is not None else None)
            while len(self._entries) > self.max_graphs:
                self._entries.popitem(last=False)            # drops the signature's graphs and their private memory pools
        else:
            self._entries.move_to_end(key)
        # (gradient accumulation: the micro and the final step of a signature each have their graph, static buffers and warm-up count)
        e = sig.steps.get(final)
        if e is None:
            e = sig.steps[final] = _Entry()
        e.calls += 1
        if sig.packed is not None:
            # GT capacity mode: this batch's GT into the signature's static buffers (one launch, current stream), for eager steps,
            # the capture and replays alike; the step itself then reads nothing but sig.packed
            ops.gt_stage([t["boxes"] for t in targets], [t["labels"] for t in targets], sig.packed)
            targets = sig.packed
        if sig.staged is not None:
            # image capacity mode: this batch's images into the signature's arena and their sizes next to them (one launch per 64
            # images, current stream), for eager steps, the capture and replays alike; the step reads nothing but sig.staged
            _stage(images, sig.staged, icls[2])
            images = sig.staged
        if e.failed or e.calls <= self.eager_steps:
            with ops.use_atss_workspaces(e.atss_ws):
                return self._step(images, targets, final)
        if e.graph is None and e.segments is None:
            try:
                self._capture(e, images, targets, final)
            except Exception as exc:                          # noqa: BLE001 -- a step that cannot be captured still has to run
                _log.warning("train-step capture failed (%s: %s); this input signature runs eagerly", type(exc).__name__, exc)
                e.failed = True
                e.clear()
                torch.cuda.synchronize()                      # (the capture's side stream has been joined by _capture_segments' finally)
                if self.ddp is not None:
                    self.ddp.reset()
                stuck = _device_usable(dev)
                if stuck is not None:
                    raise CaptureUnwindError(f"the failed capture ({type(exc).__name__}: {exc}) left the device in stream-capture mode "
                                             f"({type(stuck).__name__}: {stuck}); this process cannot run further GPU work") from exc
                e.atss_ws.clear()                             # (an unfinished capture never ran the kernels that put the table back to zero)
                with ops.use_atss_workspaces(e.atss_ws):
                    return self._step(images, targets, final)
        else:
            # the step's inputs into the graph's static buffers: one multi-tensor launch per dtype for what already lives on the
            # device (24 separate copies cost 0.19 ms per step), plain copies for the rest
            dsts, srcs = [], []
            pairs = list(zip(e.images, images)) if sig.staged is None else []
            if sig.packed is None:
                pairs += [(dt[k], v) for dt, st in zip(e.targets, targets) for k, v in st.items() if isinstance(v, Tensor)]
            for dst, src in pairs:
                if src.device == dst.device and src.dtype == dst.dtype and src.shape == dst.shape and src.is_contiguous() and dst.is_contiguous():
                    dsts.append(dst); srcs.append(src)
                else:
                    dst.copy_(src, non_blocking=True)
            if dsts:
                # (torch._foreach_copy_ still issues one hipMemcpyAsync per tensor: 24 x 11 us of GPU time)
                n = len(dsts)
                check(lib.rn_copy_many((C.c_void_p * n)(*[t.data_ptr() for t in srcs]), (C.c_void_p * n)(*[t.data_ptr() for t in dsts]),
                                       (C.c_int64 * n)(*[t.numel() * t.element_size() for t in dsts]), n,
                                       torch.cuda.current_stream(dsts[0].device).cuda_stream), "rn_copy_many")
        if getattr(self.optimizer, "_rn_device_hparams", False):
            self.optimizer.sync_device_hparams()              # the groups' current hyperparameters (lr, ...), read by the graph
        if e.segments is not None:
            self._replay_segments(e)
        else:
            e.graph.replay()
        if acc is not None:
            acc.note_step(final)                              # (the replayed advance moved the device's window position)
        note_raw_write()                                      # parameters and BN statistics changed behind torch's back
        self.replays += 1
        return e.losses


# ---- inference ------------------------------------------------------------------------------------------------------------------
class _PredictEntry:
    "One key of ``CapturedPredict``: the image arena every call of that key stages into and, once captured, the graph and the block it writes."
    __slots__ = ("calls", "failed", "graph", "staged", "block", "host", "keep")

    def __init__(self, staged, host):
        self.calls, self.failed = 0, False
        self.graph = self.block = self.keep = None
        self.staged = staged          # ops.StagedImages: B slots of 3 x pixel class, canvas = the class canvas
        self.host = host              # pinned uint8 [rn_detect_result_bytes]: where the one device-to-host copy of a call lands
        # keep: once captured, every tensor the graph reads or writes that an out-of-graph CACHE owns (_cached_tensors) -- the graph
        # holds their addresses, the caches may drop them (the anchor cache clears itself beyond 16 shapes, a scratch buffer is
        # replaced when a call needs a larger one), and memory handed back to the allocator is reused by whoever asks next


def _cached_tensors(net) -> List[Tensor]:
    """Every tensor owned by a cache that evicts or replaces its entries and whose address a captured pass of ``net`` may hold: the
    anchors of ``AnchorGenerator._cache`` (cleared beyond 16 feature-map shapes: every ``predict`` on a canvas of its own adds one),
    the per-(name, device, stream) scratch buffers of ``_launch.scratch`` and the BatchNorm workspaces of ``norm._WS`` (each replaced
    when a call needs more).  A reference taken here keeps the memory the graph points at from being handed out again.  The zero page
    (``_launch.zero_page``) and the level canvases (``biasact.Canvas._cache``) are never evicted; the folded weights of
    ``backbone._folded`` are replaced only when the weights change, which drops the graph first (``_weights_stamp``)."""
    from . import _launch, norm
    gen = getattr(net, "anchor_generator", None)
    return list(getattr(gen, "_cache", {}).values()) + list(_launch._SCRATCH.values()) + list(norm._WS.values())


class CapturedPredict:
    """``net.predict(images)`` as ONE graph replay per batch, for batches whose image sizes vary (the module docstring's last section).

    ``predictor(images)`` -- a list of fp32 CHW CUDA images -- returns what ``net.predict(images)`` returns: a list of
    ``{"boxes", "scores", "labels"}`` in original image coordinates; CPU tensors by default, ``to="device"`` gives views of the entry's
    device block instead (read them before the next call with the same key overwrites it).  ``net`` must be in eval mode (a net in
    training mode is served by plain ``net.predict``).  ``image_capacity``: "auto" or a list of padded canvases (Hp, Wp), as for
    ``CapturedTrainStep``; ``amp_dtype``: the autocast dtype of the pass (None: whatever autocast state the caller is in);
    ``eager_calls`` (>= 1): calls of a new key that run ``predict_staged`` eagerly before the capture (they fill the anchor, zero-page
    and folded-weight caches and let MIOpen choose its algorithms); ``max_graphs``: keys kept, least recently used first out;
    ``max_candidates``: the detect chain's fixed per-image candidate capacity (None: ``ops.detect_levels``' default).

    ``stats``: ``captures`` (graphs captured), ``replays`` (calls served by one), ``eager`` (calls that ran ``predict_staged`` eagerly:
    warm-up, failed captures, overflow reruns), ``fallbacks`` (calls whose result came from outside the replayed path: plain
    ``net.predict`` for a batch no class holds, or the eager rerun after a candidate overflow), ``overflows`` (the latter alone) and
    ``invalidations`` (times every graph was dropped because the weights had changed).  ``host_seconds``: the time spent inside
    ``__call__`` so far EXCEPT the waits for the device -- the per-call host cost (class and key arithmetic, the stamp walk, staging,
    the replay, the copy's enqueue, building the result), ``host_calls`` the calls it covers (fallbacks to ``net.predict`` excluded)."""

    def __init__(self, net, image_capacity="auto", amp_dtype: Optional[torch.dtype] = None, eager_calls: int = 1, max_graphs: int = 8,
                 max_candidates: Optional[int] = None):
        if image_capacity is None:
            raise ValueError("image_capacity: CapturedPredict needs 'auto' or a list of (Hp, Wp) canvases (None would never replay)")
        self.image_capacity = image_capacity_classes(image_capacity, getattr(net, "transform", None))
        if self.image_capacity == "auto":
            raise ValueError("image_capacity='auto' needs a net with a transform to derive the canvases from")
        if amp_dtype not in (None, torch.bfloat16, torch.float16):
            raise ValueError(f"amp_dtype: expected None, torch.bfloat16 or torch.float16, got {amp_dtype!r}")
        if isinstance(eager_calls, bool) or int(eager_calls) != eager_calls or int(eager_calls) < 1:
            raise ValueError(f"eager_calls must be an int >= 1 (the first call of a key fills the caches a capture must not), got {eager_calls!r}")
        if isinstance(max_graphs, bool) or int(max_graphs) != max_graphs or int(max_graphs) < 1:
            raise ValueError(f"max_graphs must be an int >= 1, got {max_graphs!r}")
        if max_candidates is not None and (isinstance(max_candidates, bool) or not isinstance(max_candidates, int) or max_candidates < 1):
            raise ValueError(f"max_candidates must be None or an int >= 1, got {max_candidates!r}")
        self.net, self.amp_dtype, self.max_candidates = net, amp_dtype, max_candidates
        self.eager_calls, self.max_graphs = int(eager_calls), int(max_graphs)
        self._entries: "OrderedDict[tuple, _PredictEntry]" = OrderedDict()
        self._stamp = None            # the weights the entries' graphs were captured under (_weights_stamp)
        self.stats = {"captures": 0, "replays": 0, "eager": 0, "fallbacks": 0, "overflows": 0, "invalidations": 0}
        self.host_seconds, self.host_calls, self._waited = 0.0, 0, 0.0

    # -- keys ---------------------------------------------------------------------------------------------------------------------
    def _autocast_dtype(self) -> Optional[torch.dtype]:
        "The autocast dtype of this call: ``amp_dtype``, else the caller's own autocast state (None: fp32)."
        if self.amp_dtype is not None:
            return self.amp_dtype
        return torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else None

    def _autocast(self, dtype):
        return torch.autocast("cuda", dtype=dtype, enabled=dtype is not None, cache_enabled=False)

    def _class_of(self, images, u8: bool = False) -> Optional[Tuple[Tuple[int, int], int, List[Tuple[int, int]]]]:
        """The batch's (canvas class, pixel class, per-image resized sizes), or None -- the batch goes to plain ``net.predict``: no
        images, images the fused transform does not take, a net or transform in training mode, a short side the device plan cannot
        take, or a canvas no class contains.  Host arithmetic on the image shapes; nothing synchronises.  ``u8``: class an all-uint8
        ``[3, h, w]`` CUDA batch like an fp32 one (``__call__`` does: ``ops.image_stage_u8`` converts it on the way into the same
        fp32 arena); by default only what the fused transform takes is classed."""
        net = self.net
        tr = net.transform
        if not isinstance(images, (list, tuple)) or not images or net.training or tr.training:
            return None
        if not all(isinstance(im, Tensor) for im in images) or tr.staged_eval_short_side() is None:
            return None
        if not (_stageable(tr, images) if u8 else tr._fusable(list(images))):
            return None
        if any(im.device != images[0].device for im in images):
            return None
        in_hw = [(int(im.shape[-2]), int(im.shape[-1])) for im in images]
        if any(h <= 0 or w <= 0 for h, w in in_hw):
            return None
        bounds = tr.staged_eval_bounds(in_hw)
        canvas = image_canvas_class(tr._canvas(bounds), self.image_capacity)
        return None if canvas is None else (canvas, image_pixel_class(in_hw), bounds)

    def _walk(self) -> Tuple[tuple, tuple]:
        """ONE walk over the net's modules per call -> (every module's ``training`` flag, the weights stamp).  The stamp is what a
        captured inference graph bakes in beyond its inputs: the folded BatchNorm weights of ``backbone._folded`` and every other tensor
        derived from the weights outside the graph.  ``norm.RAW_WRITES`` (the library's own raw-pointer writes: optimizer steps, EMA
        swaps, train-step replays) plus (data_ptr, _version) of every parameter and buffer (load_state_dict, in-place torch ops, .to())."""
        mode, stamp = [], [RAW_WRITES[0]]
        for m in self.net.modules():
            mode.append(m.training)
            for t in m._parameters.values():
                if t is not None:
                    stamp.append((t.data_ptr(), t._version))
            for t in m._buffers.values():
                if t is not None:
                    stamp.append((t.data_ptr(), t._version))
        return tuple(mode), tuple(stamp)

    def _key(self, images, icls, dtype, mode: Optional[tuple] = None) -> tuple:
        "``mode``: the modules' training flags when the caller has them from ``_walk`` (``__call__``); else walked here."
        net = self.net
        tr = net.transform
        cl = net.backbone.backbone.conv1.weight.is_contiguous(memory_format=torch.channels_last)
        if mode is None:
            mode = self._walk()[0]
        # (what the pass takes BY VALUE: the eval short side, max_size, mean and std are kernel arguments of the plan and the transform,
        # the thresholds, the box decode, the NMS kind with its two constants and max_det of the detect chain: a graph captured with one
        # decode or one NMS kind never serves another)
        return ("predict", len(images), icls[0], icls[1], dtype, cl, images[0].device, mode, tr.staged_eval_short_side(), int(tr.max_size),
                tuple(tr.image_mean), tuple(tr.image_std), net.score_thres, net.nms_thres, getattr(net, "box_decode", "reference"),
                getattr(net, "nms", "hard"), getattr(net, "soft_nms_sigma", 0.5), getattr(net, "soft_nms_min_score", 1e-3),
                net.detections_per_img)

    def _weights_stamp(self) -> tuple:
        return self._walk()[1]

    # -- the call -----------------------------------------------------------------------------------------------------------------
    def _body(self, staged, dtype, max_candidates) -> Tensor:
        "The pass itself, identical in eager mode and under capture: linear, on the current stream, nothing read back."
        with self._autocast(dtype):
            return self.net.predict_staged(staged, staged.canvas, max_candidates)

    def _read(self, e: _PredictEntry, block: Tensor, B: int) -> Tensor:
        "The one device-to-host copy of a call, into the entry's pinned buffer, and the one wait -> a host copy of the block."
        e.host.copy_(block, non_blocking=True)
        t0 = time.perf_counter()
        torch.cuda.current_stream(block.device).synchronize()
        self._waited += time.perf_counter() - t0
        return e.host.clone()

    def _fallback(self, images, dtype):
        self.stats["fallbacks"] += 1
        with self._autocast(dtype):
            return self.net.predict(images)

    def __call__(self, images: Sequence[Tensor], to: str = "cpu") -> List[Dict[str, Tensor]]:
        if to not in ("cpu", "device"):
            raise ValueError(f"to: expected 'cpu' or 'device', got {to!r}")
        dtype = self._autocast_dtype()
        icls = self._class_of(images, u8=True)
        if icls is None:
            out = self._fallback(images, dtype)
            return out if to == "device" else [{k: v.cpu() for k, v in d.items()} for d in out]
        t0, w0 = time.perf_counter(), self._waited
        try:
            return self._serve(list(images), icls, dtype, to)
        finally:
            self.host_seconds += (time.perf_counter() - t0) - (self._waited - w0)
            self.host_calls += 1

    def _serve(self, images: List[Tensor], icls, dtype, to: str) -> List[Dict[str, Tensor]]:
        B, dev, max_det = len(images), images[0].device, int(self.net.detections_per_img)
        mode, stamp = self._walk()
        if self._stamp is not None and stamp != self._stamp and self._entries:
            self._entries.clear()                             # every graph, arena and private pool: they were built on other weights
            self.stats["invalidations"] += 1
        self._stamp = stamp
        key = self._key(images, icls, dtype, mode)
        e = self._entries.get(key)
        if e is None:
            total = ops.detect_result_layout(B, max_det)["total"]
            e = self._entries[key] = _PredictEntry(ops.new_image_arena(B, icls[1], dev, icls[0]),
                                                   torch.empty((total,), dtype=torch.uint8).pin_memory())
            while len(self._entries) > self.max_graphs:
                self._entries.popitem(last=False)
        else:
            self._entries.move_to_end(key)
        e.calls += 1
        # this batch's images into the entry's arena and their sizes next to them: eager calls, the capture and replays alike
        _stage(images, e.staged, icls[2])
        if e.graph is None and not e.failed and e.calls > self.eager_calls:
            try:
                torch.cuda.synchronize()
                g = _new_graph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    e.block = self._body(e.staged, dtype, self.max_candidates)
                _repair_memset_nodes(g)
                e.graph, e.keep = g, _cached_tensors(self.net)
                self.stats["captures"] += 1
            except Exception as exc:                          # noqa: BLE001 -- a pass that cannot be captured still has to run
                _log.warning("predict capture failed (%s: %s); this key runs eagerly", type(exc).__name__, exc)
                e.failed, e.graph, e.block, e.keep = True, None, None, None
                torch.cuda.synchronize()
        if e.graph is not None:
            e.graph.replay()
            block = e.block
            self.stats["replays"] += 1
        else:
            block = self._body(e.staged, dtype, self.max_candidates)
            self.stats["eager"] += 1
        host = self._read(e, block, B)
        if bool(ops.detect_result_views(host, B, max_det)["status"].any()):
            # the fixed candidate capacity was too small for an image of this batch: once more, eagerly, on the same staged batch with
            # the worst case -- what ops.detect_levels' own retry does
            block = self._body(e.staged, dtype, "all")
            self.stats["eager"] += 1
            self.stats["overflows"] += 1
            self.stats["fallbacks"] += 1
            host = self._read(e, block, B)
        if to == "device":
            counts = ops.detect_result_views(host, B, max_det)["counts"].tolist()
            v = ops.detect_result_views(block, B, max_det)
            return [{"boxes": v["boxes"][b, :n], "scores": v["scores"][b, :n], "labels": v["labels"][b, :n]}
                    for b, n in enumerate(min(max(int(c), 0), max_det) for c in counts)]
        return ops.detect_result_dicts(host, B, max_det)
