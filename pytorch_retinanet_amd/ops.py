"""Tensor-level wrappers over the C ABI (``include/retinanet_hip.h``).

PyTorch is plumbing here: it owns device memory and the stream.  Every wrapper
passes ``tensor.data_ptr()`` and ``torch.cuda.current_stream().cuda_stream`` to
the HIP library, never synchronises with the host, and REFUSES CPU tensors --
there is no CPU implementation of this path in the product.
"""
import ctypes as C
from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib, draw_state
from ._launch import zero_page
from .draw_state import AFFINE, BBOX_CROP, COLOR_IDENTITY, COLOR_JITTER, COLOR_OPS, HFLIP, SHORT_SIDE, SHORT_SIDE_MAX  # noqa: F401
from ._lib import RN_BF16, RN_F16, RN_F32, RnDetectParams, RnLevel, RnLossParams, RnNmsParams, check, lib

RN_MATCH_NUM_FG_ZEROED, RN_MATCH_FLAGGED_ONLY = 1, 2          # include/retinanet_hip.h
LOSS_FORM_CHUNKS, LOSS_FORM_REPAIR_PASS, LOSS_FORM_LIST = 0, 1, 2   # RN_LOSS_FORM_*

_DT = {torch.float32: RN_F32, torch.bfloat16: RN_BF16, torch.float16: RN_F16}


# Optional per-op device timing (bench.py): name -> list of (start_event, end_event) recorded on the
# stream the kernels are launched on (torch's current stream).  None = disabled (default).
_TIMERS = None


def enable_timing(on: bool = True) -> None:
    global _TIMERS
    _TIMERS = {} if on else None


def timing_events():
    return _TIMERS


class _timed:
    def __init__(self, name: str, dev: torch.device):
        self.name, self.dev = name, dev

    def __enter__(self):
        if _TIMERS is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record(torch.cuda.current_stream(self.dev))
        return self

    def __exit__(self, *exc):
        if _TIMERS is not None:
            self.e1.record(torch.cuda.current_stream(self.dev))
            _TIMERS.setdefault(self.name, []).append((self.e0, self.e1))
        return False


class _KernelEvents:
    """With timing on, a pair of events that the LIBRARY records right around the streaming kernel of a loss launch (the dominant
    kernel: what bench.py's roofline is quoted on; the ``_timed`` pair around the call also covers the one-block finalize).
    ``args``: the two handles for the C call (None, None with timing off); ``note``: file the pair under timer names."""

    def __init__(self, dev: torch.device):
        self.pair = None
        if _TIMERS is not None:
            self.pair = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            for e in self.pair:
                e.record(torch.cuda.current_stream(dev))      # creates the handles
        self.args = tuple(e.cuda_event for e in self.pair) if self.pair else (None, None)

    def note(self, *names: str) -> None:
        if self.pair is not None:
            for name in names:
                _TIMERS.setdefault(name, []).append(self.pair)


class _Override:
    """``with name(value):`` -- a process-wide value that the block replaces and its exit puts back; ``name.value`` reads it (None
    outside every block).  One subclass per value: ``use_atss_workspaces``, ``use_match_state``, ``losses.grad_prescale``."""
    value = None

    def __init__(self, value):
        self.new = value

    def __enter__(self):
        cls = type(self)
        self.prev, cls.value = cls.value, self.new
        return self

    def __exit__(self, *exc):
        type(self).value = self.prev
        return False


def _need_dev(*tensors: Tensor) -> torch.device:
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "pytorch_retinanet_amd: the dense-head path runs only as HIP kernels on an MI355X; "
                f"got a {t.device} tensor (there is no CPU fallback).")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"tensors on different devices: {dev} vs {t.device}")
    return dev


def _stream(dev: torch.device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ptr(t: Optional[Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None or t.numel() == 0 else t.data_ptr())


def _dtype_code(t: Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"unsupported dtype {t.dtype}; expected float32, bfloat16 or float16")


def _c(t: Tensor) -> Tensor:
    """Dense and 16-byte aligned (the kernels use 16-byte vector accesses): views into the middle of a
    tensor (e.g. ``cls_preds[1]``) are copied to a fresh allocation."""
    if not t.is_contiguous():
        return t.contiguous()
    if t.numel() and t.data_ptr() % 16:
        return t.clone()
    return t


def _aligned(t: Tensor, align: int) -> Tensor:
    "Dense, base pointer a multiple of ``align`` bytes (copied otherwise)."
    t = t.contiguous()
    return t.clone() if t.numel() and t.data_ptr() % align else t


def _anchor_args(anchors: Tensor, B: int, A: int) -> Tuple[Tensor, int]:
    """anchors [A,4] shared or [B,A,4] per image -> (contiguous fp32 tensor, batch stride in elements)."""
    anchors = _c(anchors)
    if anchors.dtype != torch.float32:
        anchors = anchors.float()
    if anchors.dim() == 2:
        if anchors.shape != (A, 4):
            raise ValueError(f"anchors shape {tuple(anchors.shape)} != ({A}, 4)")
        return anchors, 0
    if anchors.shape != (B, A, 4):
        raise ValueError(f"anchors shape {tuple(anchors.shape)} != ({B}, {A}, 4)")
    return anchors, A * 4


# --------------------------------------------------------------------------- #
def anchors_emit(levels: Sequence[Tuple[int, int, int]], cells: Sequence[Tensor], offset: float) -> Tensor:
    """K1.  levels: [(H, W, stride)], cells: per-level device f32 [num_cell,4].  -> f32 [A,4]."""
    L = len(levels)
    if L == 0 or L > _lib.RN_MAX_LEVELS or len(cells) != L:
        raise ValueError("need 1..8 levels and one cell-anchor tensor per level")
    dev = _need_dev(*cells)
    cells = [_c(c.float()) for c in cells]
    lv = (RnLevel * L)(*[RnLevel(int(h), int(w), int(s), int(c.shape[0])) for (h, w, s), c in zip(levels, cells)])
    total = lib.rn_anchors_count(lv, L)
    out = torch.empty((total, 4), dtype=torch.float32, device=dev)
    ptrs = (C.c_void_p * L)(*[c.data_ptr() for c in cells])
    with torch.cuda.device(dev):
        check(lib.rn_anchors_emit(lv, L, ptrs, float(offset), _ptr(out), _stream(dev)), "rn_anchors_emit")
    return out


_GT_OFF_CACHE = {}          # (counts, device) -> device int32[B+1]; bounded (see gt_offsets)


def gt_offsets(counts: Sequence[int], device: torch.device) -> Tensor:
    """Prefix offsets of the per-image GT rows as a device int32[B+1].  Cached per (counts, device): training data repeats
    a handful of count tuples, the upload disappears from the step, and a step captured in a hipGraph (``graph.py``) never
    copies from temporary host memory.  Treat the result as read-only."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("pytorch_retinanet_amd: gt offsets are a device array (there is no CPU fallback)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (tuple(int(c) for c in counts), device.index)
    hit = _GT_OFF_CACHE.get(key)
    if hit is not None:
        return hit
    off = [0]
    for c in key[0]:
        off.append(off[-1] + c)
    host = torch.tensor(off, dtype=torch.int32)
    # pinned + non_blocking: the copy is stream-ordered and does not drain the launch queue
    dev_t = host.pin_memory().to(device, non_blocking=True)
    if len(_GT_OFF_CACHE) >= 4096:
        _GT_OFF_CACHE.clear()
    _GT_OFF_CACHE[key] = dev_t
    return dev_t


def gt_pack(boxes: Sequence[Tensor], labels: Sequence[Tensor], dev: torch.device):
    """The ragged GT of a batch as the library takes it -- (gt_boxes f32 [sum T, 4], gt_labels i64 [sum T], gt_off i32 [B + 1]) -- plus a
    ZEROED ``num_fg`` i32 [B] for K2, all written by ONE launch (``rn_copy_many``: 2 B + 1 small copies, the last from the zero page)
    when the per-image tensors already are f32 / i64 CUDA tensors; else two ``torch.cat`` and num_fg = None (K2 then clears it).
    Reference: the per-image ``targets[i]["boxes"]`` / ``["labels"]`` of ``RetinaNetLosses.forward`` (losses.py:113-145)."""
    counts = [int(b.reshape(-1, 4).shape[0]) for b in boxes]
    gt_off = gt_offsets(counts, dev)
    B, total = len(counts), sum(counts)
    bs = [b.reshape(-1, 4) for b in boxes]
    ls = [l.reshape(-1) for l in labels]
    fast = total > 0 and 2 * B + 1 <= 64 and 4 * B <= 256 and all(b.is_cuda and b.device == dev and b.dtype == torch.float32 and b.is_contiguous() for b in bs) \
        and all(l.is_cuda and l.device == dev and l.dtype == torch.int64 and l.is_contiguous() for l in ls)
    if not fast:
        gt_boxes = torch.cat([b.to(device=dev, dtype=torch.float32) for b in bs]) if B else torch.zeros((0, 4), device=dev)
        gt_labels = torch.cat([l.to(device=dev, dtype=torch.int64) for l in ls]) if B else torch.zeros((0,), dtype=torch.int64, device=dev)
        return gt_boxes, gt_labels, gt_off, None
    gt_boxes = torch.empty((total, 4), dtype=torch.float32, device=dev)
    gt_labels = torch.empty((total,), dtype=torch.int64, device=dev)
    num_fg = torch.empty((B,), dtype=torch.int32, device=dev)
    srcs, dsts, nb, o = [], [], [], 0
    for b, l, c in zip(bs, ls, counts):
        if c:
            srcs += [b.data_ptr(), l.data_ptr()]
            dsts += [gt_boxes.data_ptr() + 16 * o, gt_labels.data_ptr() + 8 * o]
            nb += [16 * c, 8 * c]
            o += c
    srcs.append(zero_page(dev).data_ptr()); dsts.append(num_fg.data_ptr()); nb.append(4 * B)
    n = len(srcs)
    with torch.cuda.device(dev), _timed("gt_pack", dev):
        check(lib.rn_copy_many((C.c_void_p * n)(*srcs), (C.c_void_p * n)(*dsts), (C.c_int64 * n)(*nb), n, _stream(dev)), "rn_copy_many")
    return gt_boxes, gt_labels, gt_off, num_fg


class PackedGT:
    """The GT of a batch in fixed-size device buffers (``graph.CapturedTrainStep``'s GT capacity mode): ``gt_boxes`` f32 [rows, 4],
    ``gt_labels`` i64 [rows], ``gt_off`` i32 [B + 1] and a zeroed ``num_fg`` i32 [B], as ``gt_stage`` writes them.  Only the device
    knows the per-image counts; the host knows the bounds: ``rows`` (R) and ``cap_per_image`` (no image has more boxes).  Rows
    [gt_off[B], rows) hold whatever they held before: no kernel reads them."""
    __slots__ = ("gt_boxes", "gt_labels", "gt_off", "num_fg", "rows", "cap_per_image", "B")

    def __init__(self, gt_boxes: Tensor, gt_labels: Tensor, gt_off: Tensor, num_fg: Tensor, cap_per_image: int):
        self.gt_boxes, self.gt_labels, self.gt_off, self.num_fg = gt_boxes, gt_labels, gt_off, num_fg
        self.rows, self.B, self.cap_per_image = int(gt_boxes.shape[0]), int(num_fg.shape[0]), int(cap_per_image)

    @classmethod
    def empty(cls, B: int, cap_per_image: int, dev: torch.device) -> "PackedGT":
        "Buffers for B images of at most ``cap_per_image`` boxes each (uninitialised: ``gt_stage`` fills them)."
        R = B * cap_per_image
        return cls(torch.empty((R, 4), dtype=torch.float32, device=dev), torch.empty((R,), dtype=torch.int64, device=dev),
                   torch.empty((B + 1,), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev), cap_per_image)

    def with_boxes(self, gt_boxes: Tensor) -> "PackedGT":
        return PackedGT(gt_boxes, self.gt_labels, self.gt_off, self.num_fg, self.cap_per_image)

    def with_rows(self, gt_boxes: Tensor, gt_labels: Tensor, gt_off: Tensor) -> "PackedGT":
        "New boxes, labels and offsets (an augmentation that drops rows) sharing ``num_fg``: no more rows per image than before."
        return PackedGT(gt_boxes, gt_labels, gt_off, self.num_fg, self.cap_per_image)


def gt_stage(boxes: Sequence[Tensor], labels: Sequence[Tensor], out: PackedGT) -> PackedGT:
    """The per-image GT (``boxes[b]`` [T_b, 4], ``labels[b]`` [T_b]) into ``out``'s buffers, ``gt_off`` = prefix of the counts,
    ``num_fg`` = 0: one launch per 64 images (``rn_gt_stage``) on the current stream; no host copy, no synchronisation.  Tensors that
    are not contiguous, aligned f32 / i64 tensors on ``out``'s device are converted first.  ValueError when the batch does not fit."""
    dev = out.gt_off.device
    B = len(boxes)
    if B != out.B or len(labels) != B:
        raise ValueError(f"{B} box / {len(labels)} label tensors for packed GT of {out.B} images")
    bs, ls, counts = [], [], []
    for b, l in zip(boxes, labels):
        b, l = b.reshape(-1, 4), l.reshape(-1)
        if b.shape[0] != l.shape[0]:
            raise ValueError(f"{b.shape[0]} boxes but {l.shape[0]} labels in one image")
        if b.shape[0] > out.cap_per_image:
            raise ValueError(f"an image with {b.shape[0]} boxes does not fit packed GT of {out.cap_per_image} per image")
        bs.append(_aligned(b.to(device=dev, dtype=torch.float32), 16))
        ls.append(_aligned(l.to(device=dev, dtype=torch.int64), 8))
        counts.append(int(b.shape[0]))
    n = len(counts)
    with torch.cuda.device(dev), _timed("gt_stage", dev):
        check(lib.rn_gt_stage((C.c_void_p * n)(*[_ptr(t).value for t in bs]), (C.c_void_p * n)(*[_ptr(t).value for t in ls]),
                              (C.c_int64 * n)(*counts), n, _ptr(out.gt_boxes), _ptr(out.gt_labels), out.rows, _ptr(out.gt_off),
                              _ptr(out.num_fg), _stream(dev)), "rn_gt_stage")
    return out


def gt_scale_packed(gt: PackedGT, ratios: Sequence[Tuple[float, float]]) -> PackedGT:
    """``transform.resize_boxes`` on packed GT, out of place: image b's rows times (rw, rh, rw, rh), ``ratios[b]`` = (rh, rw) fp32
    values (bit-identical to the per-image path).  -> a PackedGT sharing labels / offsets / num_fg with ``gt``, boxes in a fresh
    buffer (rows outside the images' ranges unwritten)."""
    dev = _need_dev(gt.gt_boxes, gt.gt_off)
    if len(ratios) != gt.B:
        raise ValueError(f"{len(ratios)} ratio pairs for packed GT of {gt.B} images")
    out = torch.empty_like(gt.gt_boxes)
    flat = [float(v) for r in ratios for v in r]
    with torch.cuda.device(dev), _timed("gt_scale_packed", dev):
        check(lib.rn_gt_scale_packed(_ptr(gt.gt_boxes), _ptr(out), _ptr(gt.gt_off), (C.c_float * len(flat))(*flat), gt.B, gt.rows,
                                     gt.cap_per_image, _stream(dev)), "rn_gt_scale_packed")
    return gt.with_boxes(out)


def iou_match(anchors: Tensor, gt_boxes: Tensor, gt_off: Tensor, B: int, fg_thr: float, bg_thr: float,
              want_num_fg: bool = True, want_special: bool = False, out: Optional[tuple] = None, flagged_only: bool = False,
              zeroed_num_fg: Optional[Tensor] = None):
    """K2.  anchors [A,4] or [B,A,4]; gt_boxes f32 [sum T,4]; gt_off i32 [B+1] (device).
    -> (matches i64 [B,A], num_fg i32 [B]) and, with ``want_special``, a third tensor ``special`` i64 [B, ceil(A/64)]:
    bit (a & 63) of word a >> 6 is set where ``matches[b, a] != -1`` (what ``loss_fwd_bwd_levels(special=...)`` reads instead of
    streaming ``matches``).  ``out``: pre-allocated (matches, num_fg, special) -- for a caller that launches K2 on a side
    stream and wants the outputs to belong to its main stream (``losses.RetinaNetLosses.match_ahead``).
    ``flagged_only`` (needs ``want_special``): ``matches`` is written only where a flag bit is set -- every other entry is
    UNINITIALISED; for results that go straight into ``loss_fwd_bwd_levels(special=...)`` (RN_MATCH_FLAGGED_ONLY).
    ``zeroed_num_fg``: an i32 [B] tensor that already holds zeros (``gt_pack``): used as ``num_fg``, no clear launch."""
    if not fg_thr > bg_thr:
        raise AssertionError("match_thr must be greater than back_thr")   # box_utils.py:66
    dev, A, anchors, bstride, gt_boxes, (matches, num_fg, special), flags, ret = _match_args(
        anchors, gt_boxes, gt_off, B, want_num_fg, want_special, out, flagged_only, zeroed_num_fg)
    with torch.cuda.device(dev), _timed("iou_match", dev):
        # gt_off[B] - gt_off[0] == the row count of gt_boxes (host-known): lets the library pick the batch-shaped kernel
        check(lib.rn_iou_match_special_ex(_ptr(anchors), bstride, _ptr(gt_boxes), _ptr(gt_off), B, A, fg_thr, bg_thr,
                                          _ptr(matches), _ptr(num_fg), _ptr(special), int(gt_boxes.shape[0]), flags, _stream(dev)),
              "rn_iou_match_special_ex")
    return ret


def _match_args(anchors: Tensor, gt_boxes: Tensor, gt_off: Tensor, B: int, want_num_fg: bool, want_special: bool, out: Optional[tuple],
                flagged_only: bool, zeroed_num_fg: Optional[Tensor]):
    """What ``iou_match`` and ``atss_match`` share: the converted inputs, the three output buffers (``out`` or fresh ones; ``zeroed_num_fg``
    in place of ``num_fg``), the RN_MATCH_* flag bits and the tuple to return -- three tensors with ``want_special`` or ``out``, else two.
    -> (dev, A, anchors, bstride, gt_boxes, (matches, num_fg, special), flags, ret)."""
    dev = _need_dev(anchors, gt_boxes, gt_off)
    A = anchors.shape[-2]
    anchors, bstride = _anchor_args(anchors, B, A)
    gt_boxes = _c(gt_boxes.float()).reshape(-1, 4)
    matches, num_fg, special = out if out is not None else iou_match_outputs(B, A, dev, want_num_fg and zeroed_num_fg is None, want_special)
    flags = 0
    if zeroed_num_fg is not None:
        num_fg, flags = zeroed_num_fg, RN_MATCH_NUM_FG_ZEROED
    if flagged_only:
        if special is None:
            raise ValueError("flagged_only needs the flag words (want_special=True)")
        flags |= RN_MATCH_FLAGGED_ONLY
    bufs = (matches, num_fg, special)
    return dev, A, anchors, bstride, gt_boxes, bufs, flags, bufs if (want_special or out is not None) else bufs[:2]


def iou_match_outputs(B: int, A: int, dev: torch.device, want_num_fg: bool = True, want_special: bool = True):
    "Uninitialised output tensors of ``iou_match`` (matches, num_fg, special), allocated on the current stream."
    matches = torch.empty((B, A), dtype=torch.int64, device=dev)
    num_fg = torch.empty((B,), dtype=torch.int32, device=dev) if want_num_fg else None
    special = torch.empty((B, (A + 63) // 64), dtype=torch.int64, device=dev) if want_special else None
    return matches, num_fg, special


# ---- ATSS matcher ------------------------------------------------------------------------------------------------------------
# rn_atss_match's workspace starts with its [B][A] conflict table, which must be ZERO on entry and is zero again after every completed
# call: it is zero-filled once here and then reused, so no step clears its B * A * 8 bytes.  One buffer per device, stream and anchor
# layout (two streams must not share a table); a hipGraph capture uses the buffers of its own holder (``use_atss_workspaces``: a dict
# owned by the captured entry, filled by that entry's eager steps, so the capture allocates -- and zero-fills -- nothing).
_ATSS_WS = {}
ATSS_MATCHERS = ("iou", "atss")


class use_atss_workspaces(_Override):
    "``with use_atss_workspaces(holder):`` -- ``atss_match`` calls inside the block keep their workspaces in the dict ``holder``."


def reset_atss_workspaces() -> None:
    "Drop the cached workspaces: the next call allocates zero-filled ones (for after a call that did not complete)."
    _ATSS_WS.clear()


def atss_layout(level_sizes: Sequence[int], cells, topk: int):
    "(level_off i64[L + 1], cells i32[L], L) as ctypes arrays, plus the hashable form of the same."
    sizes = [int(s) for s in level_sizes]
    L = len(sizes)
    if L == 0 or L > _lib.RN_MAX_LEVELS:
        raise ValueError(f"need 1..{_lib.RN_MAX_LEVELS} levels, got {L}")
    cells = [int(cells)] * L if isinstance(cells, int) else [int(c) for c in cells]
    if len(cells) != L:
        raise ValueError(f"{len(cells)} cell counts for {L} levels")
    if int(topk) <= 0 or any(c <= 0 for c in cells) or any(s < 0 for s in sizes):
        raise ValueError(f"topk and cells must be positive and level sizes non-negative, got topk={topk} cells={cells} sizes={sizes}")
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    return (C.c_int64 * (L + 1))(*off), (C.c_int32 * L)(*cells), L, (tuple(sizes), tuple(cells), int(topk))


def _assign_workspace(dev: torch.device, key: tuple, rows: int, nbytes_of, what: str) -> Tensor:
    """The (cached) workspace of a matcher with a conflict table (``atss_match``, ``tal_match``) under ``key`` on the current stream:
    uint8, zero-filled once.  ``nbytes_of(cap)``: the library's size for ``cap`` rows; the buffer is sized for a power-of-two row
    capacity >= ``rows``, so batches with other GT counts reuse it.  Inside ``use_atss_workspaces(holder)`` it lives in ``holder``."""
    holder = use_atss_workspaces.value
    if holder is None:
        holder, key = _ATSS_WS, key + (torch.cuda.current_stream(dev).cuda_stream,)
    hit = holder.get(key)
    if hit is not None and hit[1] >= rows:
        return hit[0]
    cap = 64
    while cap < rows:
        cap *= 2
    nbytes = nbytes_of(cap)
    if nbytes == 0:
        raise ValueError(f"{what} takes no such layout: {key}")
    if holder is _ATSS_WS and len(holder) >= 8:
        holder.clear()
    ws = torch.zeros((nbytes,), dtype=torch.uint8, device=dev)
    holder[key] = (ws, cap)
    return ws


def atss_workspace(dev: torch.device, B: int, A: int, rows: int, level_sizes: Sequence[int], cells, topk: int) -> Tensor:
    """The (cached) workspace of ``atss_match`` for these shapes on the current stream: uint8, its conflict table zero.  Sized for a
    power-of-two row capacity >= ``rows``, so batches with other GT counts reuse it."""
    off, cl, L, lkey = atss_layout(level_sizes, cells, topk)
    return _assign_workspace(dev, (dev.index, B, A) + lkey, rows,
                             lambda cap: lib.rn_atss_match_workspace_bytes(B, A, cap, off, cl, L, int(topk)), "rn_atss_match")


def atss_match(anchors: Tensor, gt_boxes: Tensor, gt_off: Tensor, B: int, level_sizes: Sequence[int], cells, topk: int = 9,
               want_num_fg: bool = True, want_special: bool = False, out: Optional[tuple] = None, flagged_only: bool = False,
               zeroed_num_fg: Optional[Tensor] = None, workspace: Optional[Tensor] = None):
    """The ATSS matcher (``rn_atss_match``; the rule: include/retinanet_hip.h, restated by ``box_utils.atss_matcher``).  Arguments and
    results as ``iou_match`` -- (matches i64 [B,A] with -1 background / GT index, num_fg i32 [B][, special]) -- with the level layout
    in place of the thresholds: ``level_sizes`` = anchors per pyramid level (in anchor order, summing to A), ``cells`` = anchors per
    grid location (an int or one per level).  ``gt_boxes.shape[0]`` is the host's upper bound on the rows (packed GT: its capacity);
    the counts are read from ``gt_off`` on the device.  ``workspace``: a uint8 tensor from ``atss_workspace`` (default: the cached
    one for these shapes and the current stream); its conflict table is zero before and after the call."""
    off, cl, L, lkey = atss_layout(level_sizes, cells, topk)
    if sum(lkey[0]) != anchors.shape[-2]:          # (the one place the level sizes are checked: a host argument, so before the device is)
        raise ValueError(f"level sizes {lkey[0]} do not sum to the {anchors.shape[-2]} anchors")
    dev, A, anchors, bstride, gt_boxes, (matches, num_fg, special), flags, ret = _match_args(
        anchors, gt_boxes, gt_off, B, want_num_fg, want_special, out, flagged_only, zeroed_num_fg)
    rows = int(gt_boxes.shape[0])
    ws = workspace if workspace is not None else atss_workspace(dev, B, A, rows, lkey[0], lkey[1], topk)
    with torch.cuda.device(dev), _timed("atss_match", dev):
        check(lib.rn_atss_match(_ptr(anchors), bstride, _ptr(gt_boxes), _ptr(gt_off), B, A, off, cl, L, int(topk), _ptr(matches),
                                _ptr(num_fg), _ptr(special), rows, flags, _ptr(ws), ws.numel(), _stream(dev)), "rn_atss_match")
    return ret


def make_loss_params(alpha: float, gamma: float, beta: float, logit_shift: float = 1.0, log_eps: float = 1e-8,
                     reg_w: Sequence[float] = (1.0, 1.0, 1.0, 1.0)) -> RnLossParams:
    return RnLossParams(alpha, gamma, beta, logit_shift, log_eps, (C.c_float * 4)(*reg_w))


def loss_fwd_bwd(cls: Tensor, box: Tensor, anchors: Tensor, gt_boxes: Tensor, gt_labels: Tensor, gt_off: Tensor,
                 matches: Tensor, num_fg: Tensor, params: RnLossParams, want_grad: bool = True):
    """K3.  cls [B,A,K], box [B,A,4] (same dtype) -> (loss f32[2] = (cls, reg), grad_cls, grad_box)."""
    dev = _need_dev(cls, box, anchors, gt_boxes, gt_labels, gt_off, matches, num_fg)
    if cls.dim() != 3 or box.dim() != 3 or box.shape[-1] != 4 or cls.shape[:2] != box.shape[:2]:
        raise ValueError(f"bad head output shapes {tuple(cls.shape)} / {tuple(box.shape)}")
    if box.dtype != cls.dtype:
        box = box.to(cls.dtype)
    B, A, K = cls.shape
    cls, box = _c(cls), _c(box)
    anchors, bstride = _anchor_args(anchors, B, A)
    gt_boxes = _c(gt_boxes.float()).reshape(-1, 4)
    gt_labels = _c(gt_labels.to(torch.int64)).reshape(-1)
    code = _dtype_code(cls)
    out = torch.empty((2,), dtype=torch.float32, device=dev)
    gcls = torch.empty_like(cls) if want_grad else None
    gbox = torch.empty_like(box) if want_grad else None
    ws_bytes = lib.rn_loss_workspace_bytes(B, A, K)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev), _timed("loss_fwd_bwd" if want_grad else "loss_fwd", dev):
        check(lib.rn_loss_fwd_bwd(_ptr(cls), _ptr(box), code, B, A, K, _ptr(anchors), bstride, _ptr(gt_boxes),
                                  _ptr(gt_labels), _ptr(gt_off), _ptr(matches), _ptr(num_fg), C.byref(params),
                                  _ptr(out), _ptr(gcls), _ptr(gbox), _ptr(ws), ws_bytes, _stream(dev)),
              "rn_loss_fwd_bwd")
    return out, gcls, gbox


class _LevelArgs:
    """What the per-level entry points share: ``box_levels[l]`` [B,A_l,4] and, unless None, ``cls_levels[l]`` [B,A_l,K] validated and
    made contiguous in one dtype (``dt``, default the first level's), with the device of all tensors (``more``: further ones that must
    live there), L, B, K (None without class outputs), A, ``counts`` (ctypes i64[L]), the fp32 anchors with their batch stride, and the
    GT arrays as the library takes them."""

    def __init__(self, cls_levels, box_levels, anchors, gt_boxes, gt_labels, gt_off, *more, dt=None):
        L = len(box_levels)
        if L == 0 or L > _lib.RN_MAX_LEVELS or (cls_levels is not None and len(cls_levels) != L):
            raise ValueError("need 1..8 levels of (cls, box) outputs")
        self.dev = _need_dev(*(cls_levels or ()), *box_levels, anchors, gt_boxes, gt_labels, gt_off, *more)
        first = (cls_levels or box_levels)[0]
        if first.dim() != 3:
            raise ValueError(f"bad level shape {tuple(first.shape)}")
        dt = dt or first.dtype
        self.L, self.B, self.K = L, int(first.shape[0]), int(first.shape[2]) if cls_levels is not None else None
        counts = [int(t.shape[1]) for t in (cls_levels or box_levels)]
        for l, b in enumerate(box_levels):
            c = cls_levels[l] if cls_levels is not None else None
            if b.shape != (self.B, counts[l], 4) or (c is not None and (c.shape != (self.B, counts[l], self.K) or c.dtype != dt)):
                raise ValueError(f"bad level shapes {None if c is None else tuple(c.shape)} / {tuple(b.shape)}")
        self.cls = None if cls_levels is None else [_c(c) for c in cls_levels]
        self.box = [_c(b if b.dtype == dt else b.to(dt)) for b in box_levels]
        self.code, self.A, self.counts = _dtype_code(self.box[0]), sum(counts), (C.c_int64 * L)(*counts)
        self.anchors, self.bstride = _anchor_args(anchors, self.B, self.A)
        self.gt_boxes = _c(gt_boxes.float()).reshape(-1, 4)
        self.gt_labels = None if gt_labels is None else _c(gt_labels.to(torch.int64)).reshape(-1)
        self.gt_off = gt_off

    def arr(self, ts: Optional[Sequence[Tensor]]):
        "The per-level base pointers of ``ts`` as a ctypes array (None for None)."
        return None if ts is None else (C.c_void_p * self.L)(*[t.data_ptr() for t in ts])

    def k3_head(self) -> tuple:
        "The leading arguments of every per-level K3 entry point."
        return (self.arr(self.cls), self.arr(self.box), self.counts, self.L, self.code, self.B, self.K, _ptr(self.anchors), self.bstride,
                _ptr(self.gt_boxes), _ptr(self.gt_labels), _ptr(self.gt_off))

    def k3_outputs(self, want_grad: bool):
        "(loss f32[2], [grad_cls_l], [grad_box_l], workspace) of a K3 launch, uninitialised; the lists are None without ``want_grad``."
        out = torch.empty((2,), dtype=torch.float32, device=self.dev)
        gcls = [torch.empty_like(c) for c in self.cls] if want_grad else None
        gbox = [torch.empty_like(b) for b in self.box] if want_grad else None
        ws = torch.empty((lib.rn_loss_workspace_bytes(self.B, self.A, self.K),), dtype=torch.uint8, device=self.dev)
        return out, gcls, gbox, ws


def _check_special(special: Tensor, B: int, A: int) -> None:
    if special.dtype != torch.int64 or tuple(special.shape) != (B, (A + 63) // 64) or not special.is_contiguous():
        raise ValueError(f"special-row words: expected int64 [{B}, {(A + 63) // 64}], got {special.dtype} {tuple(special.shape)}")


def _check_prescale(grad_prescale: Optional[Tensor], like: Tensor) -> None:
    if grad_prescale is not None:
        if not (grad_prescale.is_cuda and grad_prescale.dtype == torch.float32 and grad_prescale.numel() == 1):
            raise TypeError("grad_prescale must be a CUDA fp32 scalar")
        _need_dev(grad_prescale, like)


def loss_fwd_bwd_levels(cls_levels: Sequence[Tensor], box_levels: Sequence[Tensor], anchors: Tensor, gt_boxes: Tensor,
                        gt_labels: Tensor, gt_off: Tensor, matches: Tensor, num_fg: Tensor, params: RnLossParams,
                        want_grad: bool = True, special: Optional[Tensor] = None, in_kernel_finalize: bool = False,
                        grad_prescale: Optional[Tensor] = None, repair_pass: bool = False, form: Optional[int] = None):
    """K3 on per-level head outputs (no concatenation): cls_levels[l] [B,A_l,K], box_levels[l] [B,A_l,4].
    -> (loss f32[2], [grad_cls_l], [grad_box_l]).  ``special``: the third output of ``iou_match(want_special=True)`` --
    the kernel then reads ``matches`` only at the rows flagged there instead of streaming all of it.
    ``in_kernel_finalize``: no finalize launch -- the streaming kernel's workgroup 0 writes the two losses
    (``rn_loss_fwd_bwd_levels_fin``; same bits; uses this device's / capture's state words, ``_match_state``).
    ``grad_prescale``: device f32 scalar every gradient is multiplied by BEFORE its rounding to the I/O dtype (a GradScaler's
    scale: fp16 class gradients of ~4e-10 would otherwise flush to zero).  ``form`` (``rn_loss_fwd_bwd_levels_rp``):
    ``LOSS_FORM_CHUNKS`` (default; the one-launch kernel repairing its special rows chunk by chunk), ``LOSS_FORM_LIST`` (one launch, the
    special rows of a wave through one compact list: faster from ~32 GT boxes per image on) or ``LOSS_FORM_REPAIR_PASS`` (= ``repair_pass``;
    needs ``special``: a pure background stream + a repair kernel over the flag words; slower, kept for A/B).
    ``in_kernel_finalize=False`` has no effect once ``grad_prescale`` is set or ``form != LOSS_FORM_CHUNKS``: those calls go through the
    ``_rp`` entry, which always finalizes in the kernel."""
    if form is None:
        form = LOSS_FORM_REPAIR_PASS if repair_pass else LOSS_FORM_CHUNKS
    a = _LevelArgs(cls_levels, box_levels, anchors, gt_boxes, gt_labels, gt_off, matches, num_fg)
    if special is not None:
        _check_special(special, a.B, a.A)
    elif form == LOSS_FORM_REPAIR_PASS:
        raise ValueError("repair_pass needs the flag words of iou_match(want_special=True)")
    _check_prescale(grad_prescale, a.box[0])
    out, gcls, gbox, ws = a.k3_outputs(want_grad)
    ev = _KernelEvents(a.dev)
    with torch.cuda.device(a.dev), _timed("loss_fwd_bwd" if want_grad else "loss_fwd", a.dev):
        # the three entry points differ in what stands between the inputs and the outputs, and in the state words behind them
        head = a.k3_head() + (_ptr(matches), _ptr(special), _ptr(num_fg), C.byref(params))
        tail = (_ptr(out), a.arr(gcls), a.arr(gbox), _ptr(ws), ws.numel())
        if form != LOSS_FORM_CHUNKS or grad_prescale is not None:
            name, args = "rn_loss_fwd_bwd_levels_rp", head + (_ptr(grad_prescale), int(form)) + tail + (_ptr(_match_state(a.dev)),)
        elif in_kernel_finalize:
            name, args = "rn_loss_fwd_bwd_levels_fin", head + tail + (_ptr(_match_state(a.dev)),)
        else:
            name, args = "rn_loss_fwd_bwd_levels_ex", head + tail
        check(getattr(lib, name)(*args, _stream(a.dev), *ev.args), name)
    ev.note("loss_stream_kernel" if want_grad else "loss_stream_kernel_fwd")
    return out, gcls, gbox


def _matched_rows_args(cls_levels, box_levels, anchors, gt_boxes, gt_labels, gt_off, matches: Tensor, num_fg,
                       special: Tensor, loss: Tensor, grads: Optional[Sequence[Tensor]], reg_w: Sequence[float],
                       grad_prescale: Optional[Tensor], workspace_bytes):
    """What the ops behind K3 that walk the matcher's flagged rows share: the checks of their common arguments -- ``grads`` (None:
    value only) goes level by level with the class outputs when there are any, otherwise with the box outputs -- and
    (the ``_LevelArgs``, ``reg_w`` as ctypes f32[4], the workspace)."""
    preds, what, gname = (box_levels, "box", "gbox") if cls_levels is None else (cls_levels, "class", "gcls")
    if grads is not None and len(grads) != len(preds):
        raise ValueError(f"need as many gradient tensors as levels of {what} outputs")
    a = _LevelArgs(cls_levels, box_levels, anchors, gt_boxes, gt_labels, gt_off, matches, num_fg, special, loss, *(grads or ()),
                   dt=grads[0].dtype if grads is not None and cls_levels is None else None)
    for l, (p, g) in enumerate(zip(a.box if cls_levels is None else a.cls, grads or ())):
        if g.shape != p.shape or g.dtype != p.dtype or not g.is_contiguous():
            raise ValueError(f"{gname}[{l}]: expected a contiguous {p.dtype} {tuple(p.shape)}, got {g.dtype} {tuple(g.shape)}")
    _check_special(special, a.B, a.A)
    if matches.dtype != torch.int64 or matches.numel() != a.B * a.A or not matches.is_contiguous():
        raise ValueError(f"matches: expected a contiguous int64 [{a.B}, {a.A}], got {matches.dtype} {tuple(matches.shape)}")
    if loss.dtype != torch.float32 or loss.numel() != 2 or not loss.is_contiguous():
        raise ValueError("loss: expected K3's float32[2]")
    _check_prescale(grad_prescale, loss)
    ws = torch.empty((max(workspace_bytes(a.B, a.A), 16),), dtype=torch.uint8, device=a.dev)
    return a, (C.c_float * 4)(*[float(v) for v in reg_w]), ws


# ---- IoU-type box regression losses -----------------------------------------------------------------------------------------
BOX_LOSSES = ("smooth_l1", "giou", "diou")
BOX_LOSS_KINDS = {"giou": 1, "diou": 2}                       # RN_BOX_LOSS_GIOU / RN_BOX_LOSS_DIOU
BOX_XFORM_CLIP = float(torch.tensor(4.135166556742356, dtype=torch.float32))      # RN_BOX_XFORM_CLIP: the fp32 nearest log(1000 / 16)


def box_iou_loss(box_levels: Sequence[Tensor], anchors: Tensor, gt_boxes: Tensor, gt_off: Tensor, matches: Tensor, num_fg: Tensor,
                 special: Tensor, loss: Tensor, gbox: Optional[Sequence[Tensor]], kind: str, reg_w: Sequence[float] = (1.0, 1.0, 1.0, 1.0),
                 weight: float = 1.0, grad_prescale: Optional[Tensor] = None) -> Tensor:
    """GIoU / DIoU on the matched rows, BEHIND ``loss_fwd_bwd_levels`` on the same stream (``rn_box_iou_loss``; the rule:
    include/retinanet_hip.h, restated by ``losses.box_iou_loss_reference``).  Takes K3's outputs -- ``loss`` f32[2] and the ``gbox``
    list (None: value only) -- and the matcher's three buffers, and updates IN PLACE: ``loss[1]`` is replaced, the matched rows of
    ``gbox`` are overwritten; ``loss[0]`` and every other row keep what K3 wrote.  ``box_levels``: the head's box outputs, [B,A_l,4]
    in ``gbox``'s dtype; ``special`` (the flag words) is required: ``matches`` is read through them only.  ``grad_prescale`` as K3's.
    No synchronisation, nothing cleared: capturable.  Returns ``loss``."""
    if kind not in BOX_LOSS_KINDS:
        raise ValueError(f"kind must be one of {tuple(BOX_LOSS_KINDS)}, got {kind!r}")
    if not float(weight) > 0.0:
        raise ValueError(f"weight must be positive, got {weight!r}")
    a, reg_w, ws = _matched_rows_args(None, box_levels, anchors, gt_boxes, None, gt_off, matches, num_fg, special, loss, gbox,
                                      reg_w, grad_prescale, lib.rn_box_iou_loss_workspace_bytes)
    with torch.cuda.device(a.dev), _timed("box_iou_loss", a.dev):
        check(lib.rn_box_iou_loss(a.arr(a.box), a.counts, a.L, a.code, a.B, _ptr(a.anchors), a.bstride, _ptr(a.gt_boxes), _ptr(gt_off),
                                  _ptr(matches), _ptr(special), _ptr(num_fg), reg_w, BOX_LOSS_KINDS[kind], float(weight),
                                  _ptr(grad_prescale), _ptr(loss), a.arr(gbox), _ptr(ws), ws.numel(), _stream(a.dev)), "rn_box_iou_loss")
    return loss


# ---- Quality Focal Loss ------------------------------------------------------------------------------------------------------
CLS_LOSSES = ("focal", "qfl")


def quality_focal_loss(cls_levels: Sequence[Tensor], box_levels: Sequence[Tensor], anchors: Tensor, gt_boxes: Tensor, gt_labels: Tensor,
                       gt_off: Tensor, matches: Tensor, num_fg: Tensor, special: Tensor, loss: Tensor, gcls: Optional[Sequence[Tensor]],
                       beta: float = 2.0, reg_w: Sequence[float] = (1.0, 1.0, 1.0, 1.0), logit_shift: float = 1.0,
                       grad_prescale: Optional[Tensor] = None) -> Tensor:
    """The soft-target term of Quality Focal Loss on the matched rows' label elements, BEHIND a ``loss_fwd_bwd_levels`` call made with
    ``alpha = 1, gamma = beta`` on the same stream (``rn_quality_focal_loss``; the rule: include/retinanet_hip.h, restated by
    ``losses.box_quality_reference`` and ``losses.quality_focal_loss_reference``).  Takes K3's outputs -- ``loss`` f32[2] and the
    ``gcls`` list (None: value only) -- and the matcher's three buffers, and updates IN PLACE: the label elements' sum is added to
    ``loss[0]`` and their one gradient element each is stored into ``gcls``; ``loss[1]`` and every other element keep what K3 wrote.
    ``cls_levels`` / ``box_levels``: the head's outputs, [B,A_l,K] / [B,A_l,4] in ``gcls``'s dtype; ``special`` (the flag words) is
    required: ``matches`` is read through them only.  ``grad_prescale`` as K3's.  No synchronisation, nothing cleared: capturable.
    Returns ``loss``."""
    beta = float(beta)
    if not (beta >= 0.0 and beta < float("inf")):
        raise ValueError(f"beta must be finite and >= 0, got {beta!r}")
    a, reg_w, ws = _matched_rows_args(cls_levels, box_levels, anchors, gt_boxes, gt_labels, gt_off, matches, num_fg, special,
                                      loss, gcls, reg_w, grad_prescale, lib.rn_quality_focal_loss_workspace_bytes)
    with torch.cuda.device(a.dev), _timed("quality_focal_loss", a.dev):
        check(lib.rn_quality_focal_loss(a.arr(a.cls), a.arr(a.box), a.counts, a.L, a.code, a.B, a.K, _ptr(a.anchors), a.bstride,
                                        _ptr(a.gt_boxes), _ptr(a.gt_labels), _ptr(gt_off), _ptr(matches), _ptr(special), _ptr(num_fg),
                                        reg_w, beta, float(logit_shift), _ptr(grad_prescale), _ptr(loss), a.arr(gcls), _ptr(ws),
                                        ws.numel(), _stream(a.dev)), "rn_quality_focal_loss")
    return loss


# ---- Task-aligned matcher ----------------------------------------------------------------------------------------------------
MATCHERS = ATSS_MATCHERS + ("tal",)
TAL_TOPK_MAX = 64
TAL_EXP_MAX = 8


def tal_list_keys() -> int:
    "The capacity of a ``rn_tal_match`` workgroup's candidate list: a box over more candidates is compacted on the way (for tests)."
    return int(lib.rn_tal_match_list_keys())


def tal_exponent(value, name: str) -> int:
    """``alpha`` / ``beta`` of the task-aligned metric as the int the kernel takes.  The metric is a fixed chain of fp32 products
    (the rule has no ``powf``, so that it can be restated bit for bit), hence integers in 0..8 only."""
    if isinstance(value, bool) or not isinstance(value, (int, float)) or float(value) != int(value):
        raise ValueError(f"{name} must be an integer: the task-aligned metric score^alpha * IoU^beta is evaluated as a chain of fp32 "
                         f"products, not with powf (ultralytics' alpha = 0.5 has no such form), got {value!r}")
    if not 0 <= int(value) <= TAL_EXP_MAX:
        raise ValueError(f"{name} must lie in 0..{TAL_EXP_MAX}, got {value!r}")
    return int(value)


def tal_topk(value) -> int:
    if isinstance(value, bool) or not isinstance(value, int) or not 1 <= value <= TAL_TOPK_MAX:
        raise ValueError(f"tal_topk must be an int in 1..{TAL_TOPK_MAX}, got {value!r}")
    return value


def tal_workspace(dev: torch.device, B: int, A: int, rows: int, L: int, topk: int) -> Tensor:
    """The (cached) workspace of ``tal_match`` for these shapes on the current stream: uint8, its conflict table zero.  Kept where
    ``atss_workspace`` keeps its own (``use_atss_workspaces`` inside a capture), sized for a power-of-two row capacity >= ``rows``."""
    return _assign_workspace(dev, ("tal", dev.index, B, A, L, int(topk)), rows,
                             lambda cap: lib.rn_tal_match_workspace_bytes(B, A, cap, L, int(topk)), "rn_tal_match")


def tal_match(cls_levels: Sequence[Tensor], box_levels: Sequence[Tensor], anchors: Tensor, gt_boxes: Tensor, gt_labels: Tensor,
              gt_off: Tensor, B: int, level_sizes: Sequence[int], cells, topk: int = 13, alpha: int = 1, beta: int = 6,
              reg_w: Sequence[float] = (1.0, 1.0, 1.0, 1.0), logit_shift: float = 1.0, want_num_fg: bool = True,
              want_special: bool = False, out: Optional[tuple] = None, flagged_only: bool = False,
              zeroed_num_fg: Optional[Tensor] = None, workspace: Optional[Tensor] = None, level_w: Optional[Sequence[int]] = None):
    """The task-aligned matcher (``rn_tal_match``; the rule: include/retinanet_hip.h, restated by ``box_utils.task_aligned_matcher``):
    per GT row the ``topk`` anchors with the largest ``score^alpha * IoU^beta`` among those whose centre lies inside the box, the
    score and the IoU taken from the head's outputs ``cls_levels[l]`` [B,A_l,K] / ``box_levels[l]`` [B,A_l,4] (read as constants).
    Results, ``out``, ``flagged_only``, ``zeroed_num_fg`` and ``workspace`` as ``atss_match``; ``level_sizes`` (anchors per level) must
    be the outputs'; ``cells`` = anchors per grid location (an int or one per level).  ``level_w`` (optional): grid columns per
    level -- the kernel then visits only the cells under each box instead of the whole level (same results for a grid anchor set).
    ``alpha`` / ``beta``: integers in 0..8.  No synchronisation; capturable."""
    topk, alpha, beta = tal_topk(topk), tal_exponent(alpha, "alpha"), tal_exponent(beta, "beta")
    _, cl, L, lkey = atss_layout(level_sizes, cells, topk)
    a = _LevelArgs(cls_levels, box_levels, anchors, gt_boxes, gt_labels, gt_off)
    if a.L != L or [int(c) for c in a.counts] != list(lkey[0]):
        raise ValueError(f"level sizes {lkey[0]} are not the head outputs' {[int(c) for c in a.counts]}")
    if a.B != int(B):
        raise ValueError(f"head outputs of {a.B} images for B = {B}")
    if a.gt_labels.shape[0] != a.gt_boxes.shape[0]:
        raise ValueError(f"{a.gt_labels.shape[0]} labels for {a.gt_boxes.shape[0]} GT boxes")
    lw = None
    if level_w is not None:
        if len(level_w) != L or any(int(w) < 0 or (int(w) > 0 and s % (int(w) * c)) for w, s, c in zip(level_w, lkey[0], lkey[1])):
            raise ValueError(f"level_w {list(level_w)}: one grid width per level that, times the cells, divides the level ({lkey[0]}, {lkey[1]})")
        lw = (C.c_int32 * L)(*[int(w) for w in level_w])
    dev, A, anc, bstride, gtb, (matches, num_fg, special), flags, ret = _match_args(
        a.anchors, a.gt_boxes, gt_off, a.B, want_num_fg, want_special, out, flagged_only, zeroed_num_fg)
    rows = int(gtb.shape[0])
    ws = workspace if workspace is not None else tal_workspace(dev, a.B, A, rows, L, topk)
    rw = (C.c_float * 4)(*[float(v) for v in reg_w])
    with torch.cuda.device(dev), _timed("tal_match", dev):
        check(lib.rn_tal_match(a.arr(a.cls), a.arr(a.box), a.counts, cl, lw, L, a.code, a.B, a.K, _ptr(anc), bstride, _ptr(gtb),
                               _ptr(a.gt_labels), _ptr(gt_off), topk, alpha, beta, rw, float(logit_shift), _ptr(matches), _ptr(num_fg),
                               _ptr(special), rows, flags, _ptr(ws), ws.numel(), _stream(dev)), "rn_tal_match")
    return ret


# ---- K2 + K3 in one launch -------------------------------------------------------------------------------------------------
# State words of rn_loss_match_fwd_bwd_levels (grid-barrier counter + per-image foreground counters): zero-filled ONCE, left
# zero-filled by every completed call, never shared by two streams (one buffer per device and stream).  A hipGraph capture gets
# its own buffer, allocated BEFORE the capture begins (``new_match_state`` / ``use_match_state``: a buffer allocated inside the
# capture would come with a zero-fill node that replays every step).
MATCH_STATE_IMAGES = 4096
RN_EUNSUPPORTED = -4
_MATCH_STATE = {}


def new_match_state(dev: torch.device) -> Tensor:
    return torch.zeros((16 + MATCH_STATE_IMAGES,), dtype=torch.int32, device=dev)


class use_match_state(_Override):
    "``with use_match_state(buf):`` -- fused loss calls on ``buf.device`` inside the block use ``buf`` (graph capture)."


def reset_match_state(dev: Optional[torch.device] = None) -> None:
    """Drop the cached state buffers (all devices, or ``dev``'s): the next loss call allocates zero-filled ones.  For after a POISONED call
    -- the in-kernel finalize met a launch whose workgroups did not all arrive (a faulted launch) and set the sticky word: every later
    call on that state returns NaN losses, loudly, instead of finishing early on stale counters."""
    for key in [k for k in _MATCH_STATE if dev is None or k[0] == torch.device(dev).index]:
        del _MATCH_STATE[key]


def _match_state(dev: torch.device) -> Tensor:
    if use_match_state.value is not None and use_match_state.value.device == dev:
        return use_match_state.value
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    st = _MATCH_STATE.get(key)
    if st is None:
        st = _MATCH_STATE[key] = new_match_state(dev)
    return st


def loss_match_fwd_bwd_levels(cls_levels: Sequence[Tensor], box_levels: Sequence[Tensor], anchors: Tensor, gt_boxes: Tensor,
                              gt_labels: Tensor, gt_off: Tensor, max_gt: int, fg_thr: float, bg_thr: float, params: RnLossParams,
                              want_grad: bool = True, want_matches: bool = False):
    """K2 + K3 in ONE launch (``rn_loss_match_fwd_bwd_levels``): the matcher runs in the loss kernel's prologue, ``matches`` is
    written only when ``want_matches``.  -> (loss f32[2], [grad_cls_l], [grad_box_l], num_fg i32[B], matches or None), or
    ``None`` when the library declines the shape (more than 64 GT boxes in an image, ranges that do not fit its lists): the
    caller then runs ``iou_match`` + ``loss_fwd_bwd_levels``.  ``max_gt``: the largest per-image GT count (host-known)."""
    if not fg_thr > bg_thr:
        raise AssertionError("match_thr must be greater than back_thr")   # box_utils.py:66
    a = _LevelArgs(cls_levels, box_levels, anchors, gt_boxes, gt_labels, gt_off)
    if max_gt > 64 or a.B > MATCH_STATE_IMAGES:
        return None
    out, gcls, gbox, ws = a.k3_outputs(want_grad)
    num_fg = torch.empty((a.B,), dtype=torch.int32, device=a.dev)
    matches = torch.empty((a.B, a.A), dtype=torch.int64, device=a.dev) if want_matches else None
    state = _match_state(a.dev)
    ev = _KernelEvents(a.dev)
    with torch.cuda.device(a.dev), _timed("loss_fwd_bwd" if want_grad else "loss_fwd", a.dev):
        rc = lib.rn_loss_match_fwd_bwd_levels(*a.k3_head(), int(max_gt), fg_thr, bg_thr, _ptr(matches), _ptr(num_fg), C.byref(params),
                                              _ptr(out), a.arr(gcls), a.arr(gbox), _ptr(ws), ws.numel(), _ptr(state), state.numel() * 4,
                                              _stream(a.dev), *ev.args)
        if rc == RN_EUNSUPPORTED:
            return None
        check(rc, "rn_loss_match_fwd_bwd_levels")
    ev.note("loss_stream_kernel" if want_grad else "loss_stream_kernel_fwd", "loss_stream_kernel_fused_match")
    return out, gcls, gbox, num_fg, matches


def scale_inplace(t: Tensor, scale: Tensor) -> Tensor:
    """t *= scale (device scalar, f32); a no-op on the device when scale == 1."""
    dev = _need_dev(t, scale)
    if not t.is_contiguous():
        raise ValueError("scale_inplace needs a contiguous tensor")
    scale = _c(scale.detach().to(torch.float32)).reshape(1)
    with torch.cuda.device(dev):
        check(lib.rn_scale_inplace(_ptr(t), _dtype_code(t), t.numel(), _ptr(scale), _stream(dev)), "rn_scale_inplace")
    return t


def scale_inplace_batched(tensors: Sequence[Tensor], scales: Sequence[Tensor]) -> None:
    """tensors[k] *= scales[k] (device scalars, f32[1]) for up to 16 contiguous tensors per launch, grouped by dtype; a no-op on
    the device where a scale is 1."""
    if not tensors:
        return
    dev = _need_dev(*tensors, *scales)
    scales = [_c(s.detach().to(torch.float32)).reshape(1) for s in scales]
    by_dtype = {}
    for t, s in zip(tensors, scales):
        if not t.is_contiguous():
            raise ValueError("scale_inplace_batched needs contiguous tensors")
        if t.numel():
            by_dtype.setdefault(t.dtype, []).append((t, s))
    with torch.cuda.device(dev):
        for dt, items in by_dtype.items():
            for i in range(0, len(items), 16):
                part = items[i:i + 16]
                n = len(part)
                check(lib.rn_scale_inplace_batched((C.c_void_p * n)(*[_ptr(t) for t, _ in part]), (C.c_int64 * n)(*[t.numel() for t, _ in part]),
                                                   (C.c_void_p * n)(*[_ptr(s) for _, s in part]), n, _dtype_code(part[0][0]), _stream(dev)),
                      "rn_scale_inplace_batched")


def image_hw_tensor(sizes: Sequence[Tuple[int, int]], device: torch.device) -> Tensor:
    host = torch.tensor([[int(h), int(w)] for h, w in sizes], dtype=torch.int32)
    return host.pin_memory().to(device, non_blocking=True)


def transform_batch(images: Sequence[Tensor], out_sizes: Sequence[Tuple[int, int]], mean: Sequence[float],
                    std: Sequence[float], Hp: int, Wp: int, out_dtype: torch.dtype = torch.float32,
                    channels_last: bool = False, flags: Optional[Tensor] = None, coef: Optional[Tensor] = None) -> Tensor:
    """T1: (x - mean) / std -> bilinear resize of image b to out_sizes[b] -> zero-padded batch
    ``[B, 3, Hp, Wp]`` (``out_dtype``; channels_last memory format on request) in one launch.
    images: CUDA f32 ``[3, h, w]`` tensors; Wp % 4 == 0.  ``flags`` (uint8 [>= B] on the images' device, ``hflip_draw``): image b is
    horizontally flipped first where flags[b] != 0 (``rn_transform_batch_flip``: bit-identical to the transform of ``img.flip(-1)``).
    ``coef`` (f32 [B, 8] = ``rn_color_coef`` per image, ``color_jitter_draw`` / ``color_mean``): the colour jitter applied to the raw
    pixels (``rn_transform_batch_color``)."""
    dev = _need_dev(*images)
    if flags is not None:
        _check_flags(flags, len(images), dev)
    if coef is not None:
        _check_coef(coef, len(images), dev)
    B = len(images)
    if B == 0 or len(out_sizes) != B:
        raise ValueError("need one output size per image")
    imgs = []
    for im in images:
        if im.dim() != 3 or im.shape[0] != 3 or im.dtype != torch.float32:
            raise ValueError(f"transform_batch expects f32 [3, h, w] images, got {tuple(im.shape)} {im.dtype}")
        imgs.append(im if im.is_contiguous() else im.contiguous())
    if out_dtype not in _DT:
        raise ValueError(f"unsupported output dtype {out_dtype}")
    out = torch.empty((B, 3, Hp, Wp), dtype=out_dtype, device=dev,
                      memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    ptrs = (C.c_void_p * B)(*[im.data_ptr() for im in imgs])
    in_hw = (C.c_int32 * (2 * B))(*[int(v) for im in imgs for v in im.shape[1:]])
    out_hw = (C.c_int32 * (2 * B))(*[int(v) for s in out_sizes for v in s])
    with torch.cuda.device(dev), _timed("transform_batch", dev):
        if coef is not None:
            check(lib.rn_transform_batch_color(ptrs, in_hw, None, 0, None, out_hw, None, B, (C.c_float * 3)(*mean), (C.c_float * 3)(*std),
                                               int(Hp), int(Wp), _ptr(out), _DT[out_dtype], int(bool(channels_last)), _ptr(flags),
                                               _ptr(coef), _stream(dev)), "rn_transform_batch_color")
        elif flags is None:
            check(lib.rn_transform_batch(ptrs, in_hw, out_hw, B, (C.c_float * 3)(*mean), (C.c_float * 3)(*std), int(Hp), int(Wp),
                                         _ptr(out), _DT[out_dtype], int(bool(channels_last)), _stream(dev)), "rn_transform_batch")
        else:
            check(lib.rn_transform_batch_flip(ptrs, in_hw, out_hw, B, (C.c_float * 3)(*mean), (C.c_float * 3)(*std), int(Hp), int(Wp),
                                              _ptr(out), _DT[out_dtype], int(bool(channels_last)), _ptr(flags), _stream(dev)),
                  "rn_transform_batch_flip")
    return out


def transform_batch_dev(images: Sequence[Tensor], out_hw: Tensor, mean: Sequence[float], std: Sequence[float], Hp: int, Wp: int,
                        out_dtype: torch.dtype = torch.float32, channels_last: bool = False, flags: Optional[Tensor] = None,
                        coef: Optional[Tensor] = None) -> Tensor:
    """``transform_batch`` with the output sizes on the device (``rn_transform_batch_dev``): ``out_hw`` int32 [B, 2] on the images'
    device, as ``short_side_draw`` writes it; ``Hp`` / ``Wp`` stay host values (a size above the canvas is clamped in the kernel).
    Bit-identical to ``transform_batch`` called with the same sizes on the host, with or without ``flags`` / ``coef``."""
    dev = _need_dev(*images, out_hw)
    if coef is not None:
        _check_coef(coef, len(images), dev)
    B = len(images)
    if B == 0:
        raise ValueError("need at least one image")
    if out_hw.dtype != torch.int32 or tuple(out_hw.shape) != (B, 2) or not out_hw.is_contiguous():
        raise ValueError(f"out_hw must be a contiguous int32 [{B}, 2] tensor, got {tuple(out_hw.shape)} {out_hw.dtype}")
    if flags is not None:
        _check_flags(flags, B, dev)
    imgs = []
    for im in images:
        if im.dim() != 3 or im.shape[0] != 3 or im.dtype != torch.float32:
            raise ValueError(f"transform_batch_dev expects f32 [3, h, w] images, got {tuple(im.shape)} {im.dtype}")
        imgs.append(im if im.is_contiguous() else im.contiguous())
    if out_dtype not in _DT:
        raise ValueError(f"unsupported output dtype {out_dtype}")
    out = torch.empty((B, 3, Hp, Wp), dtype=out_dtype, device=dev,
                      memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    ptrs = (C.c_void_p * B)(*[im.data_ptr() for im in imgs])
    in_hw = (C.c_int32 * (2 * B))(*[int(v) for im in imgs for v in im.shape[1:]])
    with torch.cuda.device(dev), _timed("transform_batch", dev):
        if coef is not None:
            check(lib.rn_transform_batch_color(ptrs, in_hw, None, 0, None, None, _ptr(out_hw), B, (C.c_float * 3)(*mean),
                                               (C.c_float * 3)(*std), int(Hp), int(Wp), _ptr(out), _DT[out_dtype], int(bool(channels_last)),
                                               _ptr(flags), _ptr(coef), _stream(dev)), "rn_transform_batch_color")
            return out
        check(lib.rn_transform_batch_dev(ptrs, in_hw, B, (C.c_float * 3)(*mean), (C.c_float * 3)(*std), int(Hp), int(Wp), _ptr(out),
                                         _DT[out_dtype], int(bool(channels_last)), _ptr(out_hw), _ptr(flags), _stream(dev)),
              "rn_transform_batch_dev")
    return out


# ---- train-time horizontal flip (augment.RandomHorizontalFlip) ----------------------------------------------------------------
# The state blocks of the draws below are made, written and read by ``draw_state`` (new / write / read with its layouts); the draw
# launchers validate theirs through ``draw_state.check``.
HFLIP_STATE_BYTES, SHORT_SIDE_STATE_BYTES, COLOR_JITTER_STATE_BYTES = HFLIP.nbytes, SHORT_SIDE.nbytes, COLOR_JITTER.nbytes
BBOX_CROP_STATE_BYTES, AFFINE_STATE_BYTES = BBOX_CROP.nbytes, AFFINE.nbytes


def _check_flags(flags: Tensor, B: int, dev: torch.device) -> None:
    if flags.dtype != torch.uint8 or flags.device != dev or flags.dim() != 1 or flags.numel() < B or not flags.is_contiguous():
        raise ValueError(f"flags must be a contiguous uint8 vector of >= {B} entries on {dev}, got {tuple(flags.shape)} {flags.dtype} "
                         f"on {flags.device}")


def hflip_draw(block: Tensor, B: int) -> Tensor:
    """``rn_hflip_draw``: flags uint8 [B] (1 = flip image b) drawn from the block's seed / counter / p, then the block's counter advances
    by one -- one launch on the current stream, no host synchronisation (capturable: each replay draws anew)."""
    dev = _need_dev(block)
    draw_state.check(HFLIP, block)
    B = int(B)
    if B <= 0:
        raise ValueError(f"B must be positive, got {B}")
    flags = torch.empty((B,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev), _timed("hflip_draw", dev):
        check(lib.rn_hflip_draw(_ptr(block), B, _ptr(flags), _stream(dev)), "rn_hflip_draw")
    return flags


# ---- train-time colour jitter (augment.ColorJitter) ----------------------------------------------------------------------------
COLOR_COEF_FLOATS = 8                  # rn_color_coef: f f32[4], mean f32, order i32, bc_mul f32, bc_add f32 (zero without brightness / contrast)


def _check_coef(coef: Tensor, B: int, dev: torch.device) -> None:
    if coef.dtype != torch.float32 or tuple(coef.shape) != (B, COLOR_COEF_FLOATS) or not coef.is_contiguous() or coef.device != dev:
        raise ValueError(f"coef must be a contiguous f32 [{B}, {COLOR_COEF_FLOATS}] tensor (rn_color_coef per image) on {dev}, got "
                         f"{tuple(coef.shape)} {coef.dtype} on {coef.device}")


def color_jitter_draw(block: Tensor, B: int) -> Tensor:
    """``rn_color_jitter_draw``: coef f32 [B, 8] (``rn_color_coef`` per image: four factors, mean = 0, the order as int32 bits in column
    5) drawn from the block, then the block's counter advances by one -- one launch on the current stream for any B, no host
    synchronisation (capturable: each replay draws anew)."""
    dev = _need_dev(block)
    draw_state.check(COLOR_JITTER, block)
    B = int(B)
    if B <= 0:
        raise ValueError(f"B must be positive, got {B}")
    coef = torch.empty((B, COLOR_COEF_FLOATS), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), _timed("color_jitter_draw", dev):
        check(lib.rn_color_jitter_draw(_ptr(block), B, _ptr(coef), _stream(dev)), "rn_color_jitter_draw")
    return coef


def color_mean(images, coef: Tensor, workspace: Optional[Tensor] = None) -> Tensor:
    """``rn_color_mean``: writes ``coef[b, 4]`` = the mean gray of image b as it is when its contrast's turn comes, for the images whose
    order holds a contrast (in place; returns ``coef``).  ``images``: CUDA f32 ``[3, h, w]`` tensors, or ``StagedImages``.  No atomics,
    a fixed order of every sum: two calls give the same bits.  ``workspace``: uint8, >= ``rn_color_mean_workspace_bytes(B)``."""
    staged = isinstance(images, StagedImages)
    dev = _need_dev(coef, *((images.arena, images.in_hw) if staged else images))
    B = images.B if staged else len(images)
    _check_coef(coef, B, dev)
    need = int(lib.rn_color_mean_workspace_bytes(B))
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
    _need_dev(workspace)
    with torch.cuda.device(dev), _timed("color_mean", dev):
        if staged:
            check(lib.rn_color_mean(None, None, _ptr(images.arena), images.slot, _ptr(images.in_hw), B, _ptr(coef), _ptr(workspace),
                                    int(workspace.numel() * workspace.element_size()), _stream(dev)), "rn_color_mean")
        else:
            imgs = []
            for im in images:
                if im.dim() != 3 or im.shape[0] != 3 or im.dtype != torch.float32:
                    raise ValueError(f"color_mean expects f32 [3, h, w] images, got {tuple(im.shape)} {im.dtype}")
                imgs.append(im if im.is_contiguous() else im.contiguous())
            ptrs = (C.c_void_p * B)(*[im.data_ptr() for im in imgs])
            in_hw = (C.c_int32 * (2 * B))(*[int(v) for im in imgs for v in im.shape[1:]])
            check(lib.rn_color_mean(ptrs, in_hw, None, 0, None, B, _ptr(coef), _ptr(workspace),
                                    int(workspace.numel() * workspace.element_size()), _stream(dev)), "rn_color_mean")
    return coef


# ---- train-time brightness / contrast (augment.RandomBrightnessContrast) -----------------------------------------------------------
BRIGHTNESS_CONTRAST_STATE_BYTES = draw_state.BRIGHTNESS_CONTRAST.nbytes
COLOR_BC_PRESENT, COLOR_BC_PENDING = 1 << 16, 1 << 17      # bits of column 5 (``order``): bc_mul / bc_add apply; bc_add still holds beta


def brightness_contrast_draw(block: Tensor, B: int, coef: Optional[Tensor] = None) -> Tensor:
    """``rn_brightness_contrast_draw``: ``bc_mul`` / ``bc_add`` (columns 6 and 7) and bits 16 / 17 of the order (column 5) of the
    ``rn_color_coef`` rows, drawn from the block, then the block's counter advances by one -- one launch on the current stream for any
    B, no host synchronisation (capturable: each replay draws anew).  ``coef``: the rows a ``color_jitter_draw`` wrote (in place; its
    six words stay), or None for fresh rows whose colour part is the identity.  Returns the rows."""
    dev = _need_dev(block)
    draw_state.check(draw_state.BRIGHTNESS_CONTRAST, block)
    B = int(B)
    if B <= 0:
        raise ValueError(f"B must be positive, got {B}")
    fresh = coef is None
    if fresh:
        coef = torch.empty((B, COLOR_COEF_FLOATS), dtype=torch.float32, device=dev)
    _check_coef(coef, B, dev)
    with torch.cuda.device(dev), _timed("brightness_contrast_draw", dev):
        check(lib.rn_brightness_contrast_draw(_ptr(block), B, _ptr(coef), int(fresh), _stream(dev)), "rn_brightness_contrast_draw")
    return coef


def brightness_contrast_mean(images, coef: Tensor, workspace: Optional[Tensor] = None, return_ref: bool = False):
    """``rn_brightness_contrast_mean``: for the rows whose bit 17 is set, ``bc_add`` = beta times the mean of all values of image b as
    it is after its colour operations, and the bit cleared (in place; returns ``coef``) -- launch it after ``color_mean``.  ``images``:
    CUDA f32 ``[3, h, w]`` tensors, or ``StagedImages``.  No atomics, a fixed order of every sum; a second call changes nothing.
    ``workspace``: uint8, >= ``rn_brightness_contrast_mean_workspace_bytes(B)``.  ``return_ref``: also the f32 [B] view of the workspace
    where the launch left the mean of every row it served (the other entries are not written)."""
    staged = isinstance(images, StagedImages)
    dev = _need_dev(coef, *((images.arena, images.in_hw) if staged else images))
    B = images.B if staged else len(images)
    _check_coef(coef, B, dev)
    need = int(lib.rn_brightness_contrast_mean_workspace_bytes(B))
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
    _need_dev(workspace)
    nbytes = int(workspace.numel() * workspace.element_size())
    with torch.cuda.device(dev), _timed("brightness_contrast_mean", dev):
        if staged:
            check(lib.rn_brightness_contrast_mean(None, None, _ptr(images.arena), images.slot, _ptr(images.in_hw), B, _ptr(coef),
                                                  _ptr(workspace), nbytes, _stream(dev)), "rn_brightness_contrast_mean")
        else:
            imgs = []
            for im in images:
                if im.dim() != 3 or im.shape[0] != 3 or im.dtype != torch.float32:
                    raise ValueError(f"brightness_contrast_mean expects f32 [3, h, w] images, got {tuple(im.shape)} {im.dtype}")
                imgs.append(im if im.is_contiguous() else im.contiguous())
            ptrs = (C.c_void_p * B)(*[im.data_ptr() for im in imgs])
            in_hw = (C.c_int32 * (2 * B))(*[int(v) for im in imgs for v in im.shape[1:]])
            check(lib.rn_brightness_contrast_mean(ptrs, in_hw, None, 0, None, B, _ptr(coef), _ptr(workspace), nbytes, _stream(dev)),
                  "rn_brightness_contrast_mean")
    if return_ref:
        at = int(lib.rn_color_mean_workspace_bytes(B))
        return coef, workspace.view(torch.uint8).reshape(-1)[at:at + 4 * B].view(torch.float32)
    return coef


def gt_flip_scale_many(boxes: Sequence[Tensor], widths: Sequence[float], ratios: Sequence[Tuple[float, float]], flags: Tensor) -> Tensor:
    """``resize_boxes`` of every image's boxes after the horizontal flip where ``flags[b]`` is set (x1' = W_b - x2, x2' = W_b - x1, fp32;
    ``widths[b]`` = W_b, the width before the resize; ``ratios[b]`` = (rh, rw)): ONE launch per 64 images (``rn_gt_flip_scale_many``)
    into a fresh f32 [sum T_b, 4] buffer, images in order.  Boxes that are not contiguous, aligned f32 on the flags' device are
    converted first."""
    dev = _need_dev(flags)
    B = len(boxes)
    if B == 0 or len(widths) != B or len(ratios) != B:
        raise ValueError(f"{B} box tensors, {len(widths)} widths, {len(ratios)} ratio pairs")
    _check_flags(flags, B, dev)
    bs = [_aligned(b.reshape(-1, 4).to(device=dev, dtype=torch.float32), 16) for b in boxes]
    counts = [int(b.shape[0]) for b in bs]
    out = torch.empty((sum(counts), 4), dtype=torch.float32, device=dev)
    flat = [float(v) for r in ratios for v in r]
    with torch.cuda.device(dev), _timed("gt_flip_scale_many", dev):
        check(lib.rn_gt_flip_scale_many((C.c_void_p * B)(*[_ptr(t).value for t in bs]), (C.c_int64 * B)(*counts), B,
                                        (C.c_float * B)(*[float(w) for w in widths]), (C.c_float * (2 * B))(*flat), _ptr(flags),
                                        _ptr(out), int(out.shape[0]), _stream(dev)), "rn_gt_flip_scale_many")
    return out


def gt_flip_scale_packed(gt: PackedGT, widths: Sequence[float], ratios: Sequence[Tuple[float, float]], flags: Tensor) -> PackedGT:
    """``gt_scale_packed`` with the horizontal flip of ``gt_flip_scale_many`` (``rn_gt_flip_scale_packed``), out of place; it launches
    whatever the ratios are (a flip changes the boxes at ratio 1 too)."""
    dev = _need_dev(gt.gt_boxes, gt.gt_off, flags)
    if len(ratios) != gt.B or len(widths) != gt.B:
        raise ValueError(f"{len(widths)} widths / {len(ratios)} ratio pairs for packed GT of {gt.B} images")
    _check_flags(flags, gt.B, dev)
    out = torch.empty_like(gt.gt_boxes)
    flat = [float(v) for r in ratios for v in r]
    with torch.cuda.device(dev), _timed("gt_flip_scale_packed", dev):
        check(lib.rn_gt_flip_scale_packed(_ptr(gt.gt_boxes), _ptr(out), _ptr(gt.gt_off), (C.c_float * gt.B)(*[float(w) for w in widths]),
                                          (C.c_float * len(flat))(*flat), _ptr(flags), gt.B, gt.rows, gt.cap_per_image, _stream(dev)),
              "rn_gt_flip_scale_packed")
    return gt.with_boxes(out)


# ---- multi-scale training: the short side drawn on the device (augment.RandomShortSide) ---------------------------------------
def short_side_draw(block: Tensor, in_hw: Sequence[Tuple[int, int]], max_size: int) -> Tuple[Tensor, Tensor]:
    """``rn_short_side_draw``: for the images of sizes ``in_hw`` ((h, w) host ints) the resized sizes int32 [B, 2] and the box ratios
    f32 [2B] = (rh, rw) per image, drawn from the block's seed / counter / sizes, then the block's counter advances by one -- one
    launch per 64 images on the current stream, no host synchronisation (capturable: each replay draws anew)."""
    dev = _need_dev(block)
    draw_state.check(SHORT_SIDE, block)
    B = len(in_hw)
    if B == 0:
        raise ValueError("need at least one image size")
    out_hw = torch.empty((B, 2), dtype=torch.int32, device=dev)
    ratios = torch.empty((2 * B,), dtype=torch.float32, device=dev)
    hw = (C.c_int32 * (2 * B))(*[int(v) for s in in_hw for v in s])
    with torch.cuda.device(dev), _timed("short_side_draw", dev):
        check(lib.rn_short_side_draw(_ptr(block), hw, int(max_size), B, _ptr(out_hw), _ptr(ratios), _stream(dev)), "rn_short_side_draw")
    return out_hw, ratios


def _check_ratios_dev(ratios: Tensor, B: int, dev: torch.device) -> None:
    if ratios.dtype != torch.float32 or ratios.device != dev or ratios.numel() != 2 * B or not ratios.is_contiguous():
        raise ValueError(f"ratios must be a contiguous f32 tensor of {2 * B} entries on {dev}, got {tuple(ratios.shape)} {ratios.dtype} "
                         f"on {ratios.device}")


def gt_flip_scale_many_dev(boxes: Sequence[Tensor], widths: Sequence[float], ratios: Tensor, flags: Optional[Tensor] = None) -> Tensor:
    """``gt_flip_scale_many`` with the ratios on the device (``ratios`` f32 [2B] = (rh, rw) per image, as ``short_side_draw`` writes
    them) and the flags optional (None: nothing flips) -- ``rn_gt_flip_scale_many_dev``, bit-identical given the same values."""
    dev = _need_dev(ratios, flags)
    B = len(boxes)
    if B == 0 or len(widths) != B:
        raise ValueError(f"{B} box tensors, {len(widths)} widths")
    _check_ratios_dev(ratios, B, dev)
    if flags is not None:
        _check_flags(flags, B, dev)
    bs = [_aligned(b.reshape(-1, 4).to(device=dev, dtype=torch.float32), 16) for b in boxes]
    counts = [int(b.shape[0]) for b in bs]
    out = torch.empty((sum(counts), 4), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), _timed("gt_flip_scale_many", dev):
        check(lib.rn_gt_flip_scale_many_dev((C.c_void_p * B)(*[_ptr(t).value for t in bs]), (C.c_int64 * B)(*counts), B,
                                            (C.c_float * B)(*[float(w) for w in widths]), _ptr(ratios), _ptr(flags),
                                            _ptr(out), int(out.shape[0]), _stream(dev)), "rn_gt_flip_scale_many_dev")
    return out


def gt_flip_scale_packed_dev(gt: PackedGT, widths: Sequence[float], ratios: Tensor, flags: Optional[Tensor] = None) -> PackedGT:
    "``gt_flip_scale_packed`` with the ratios on the device and the flags optional (``rn_gt_flip_scale_packed_dev``), out of place."
    dev = _need_dev(gt.gt_boxes, gt.gt_off, ratios, flags)
    if len(widths) != gt.B:
        raise ValueError(f"{len(widths)} widths for packed GT of {gt.B} images")
    _check_ratios_dev(ratios, gt.B, dev)
    if flags is not None:
        _check_flags(flags, gt.B, dev)
    out = torch.empty_like(gt.gt_boxes)
    with torch.cuda.device(dev), _timed("gt_flip_scale_packed", dev):
        check(lib.rn_gt_flip_scale_packed_dev(_ptr(gt.gt_boxes), _ptr(out), _ptr(gt.gt_off), (C.c_float * gt.B)(*[float(w) for w in widths]),
                                              _ptr(ratios), _ptr(flags), gt.B, gt.rows, gt.cap_per_image, _stream(dev)),
              "rn_gt_flip_scale_packed_dev")
    return gt.with_boxes(out)


# ---- images of varying sizes in a fixed arena (graph.CapturedTrainStep, image capacity mode) ----------------------------------
class StagedImages:
    """The images of a batch in a fixed-size device arena (``graph.CapturedTrainStep``'s image capacity mode): ``arena`` f32 [B, slot]
    -- image b dense at the start of row b, ``[3][h_b][w_b]`` with its own strides -- and ``in_hw`` i32 [B, 2] = its (h, w), as
    ``image_stage`` writes them.  The kernels read every input size from ``in_hw``; the host keeps the bounds: ``slot`` (floats per
    image, 3 x the pixel class) and ``canvas`` (the padded (Hp, Wp) of the batch's canvas class, set by whoever owns the arena).
    ``hw`` is the host's list of the (h, w) staged last and ``bounds`` the per-image sizes after the resize that whoever staged them
    worked out from it (None: the transform works them out): for canvas and bound arithmetic only, no kernel argument is derived
    from either.  Floats [3 h_b w_b, slot) of a row hold whatever they held before: no kernel reads them."""
    __slots__ = ("arena", "in_hw", "B", "slot", "hw", "bounds", "canvas")

    def __init__(self, arena: Tensor, in_hw: Tensor, canvas: Optional[Tuple[int, int]] = None):
        if arena.dim() != 2 or arena.dtype != torch.float32 or not arena.is_contiguous():
            raise ValueError(f"arena must be a contiguous f32 [B, slot] tensor, got {tuple(arena.shape)} {arena.dtype}")
        if in_hw.dtype != torch.int32 or tuple(in_hw.shape) != (arena.shape[0], 2) or not in_hw.is_contiguous() or in_hw.device != arena.device:
            raise ValueError(f"in_hw must be a contiguous int32 [{arena.shape[0]}, 2] tensor on {arena.device}")
        self.arena, self.in_hw = arena, in_hw
        self.B, self.slot = int(arena.shape[0]), int(arena.shape[1])
        self.hw: List[Tuple[int, int]] = []
        self.bounds: Optional[List[Tuple[int, int]]] = None
        self.canvas = None if canvas is None else (int(canvas[0]), int(canvas[1]))

    @property
    def device(self) -> torch.device:
        return self.arena.device

    def __len__(self) -> int:
        return self.B

    @classmethod
    def empty(cls, B: int, pixel_class: int, dev: torch.device, canvas: Optional[Tuple[int, int]] = None) -> "StagedImages":
        "An arena for B images of at most ``pixel_class`` pixels each (uninitialised: ``image_stage`` fills it)."
        return cls(torch.empty((int(B), 3 * int(pixel_class)), dtype=torch.float32, device=dev),
                   torch.empty((int(B), 2), dtype=torch.int32, device=dev), canvas)


def new_image_arena(B: int, pixel_class: int, dev: torch.device, canvas: Optional[Tuple[int, int]] = None) -> StagedImages:
    "``StagedImages.empty``: the arena a signature of the image capacity mode owns (B slots of 3 x ``pixel_class`` fp32)."
    return StagedImages.empty(B, pixel_class, dev, canvas)


def image_stage(images: Sequence[Tensor], out: StagedImages, bounds: Optional[Sequence[Tuple[int, int]]] = None) -> StagedImages:
    """The images (CUDA f32 ``[3, h_b, w_b]`` on ``out``'s device) into ``out``'s arena, ``in_hw`` = their sizes: one launch per 64
    images (``rn_image_stage``) on the current stream; no host copy, no synchronisation.  Strided images are made dense first.
    ValueError for another dtype or layout (this op takes f32 CHW only: uint8 images, planes or interleaved, go through
    ``image_stage_u8`` below, which fills the same arena), a zero size or an image above the slot.
    ``bounds``: the per-image sizes after the resize, when the caller has them (kept as ``out.bounds`` for the transform)."""
    dev = _need_dev(out.arena, *images)
    B = len(images)
    if B != out.B:
        raise ValueError(f"{B} images for an arena of {out.B} slots")
    imgs, hw = [], []
    for im in images:
        if im.dim() != 3 or im.shape[0] != 3 or im.dtype != torch.float32:
            raise ValueError(f"image_stage expects f32 [3, h, w] images, got {tuple(im.shape)} {im.dtype}")
        h, w = int(im.shape[1]), int(im.shape[2])
        if h <= 0 or w <= 0 or 3 * h * w > out.slot:
            raise ValueError(f"a {h} x {w} image does not fit an arena slot of {out.slot} floats")
        imgs.append(im if im.is_contiguous() else im.contiguous())
        hw.append((h, w))
    with torch.cuda.device(dev), _timed("image_stage", dev):
        check(lib.rn_image_stage((C.c_void_p * B)(*[im.data_ptr() for im in imgs]), (C.c_int32 * (2 * B))(*[v for s in hw for v in s]), B,
                                 _ptr(out.arena), out.slot, _ptr(out.in_hw), _stream(dev)), "rn_image_stage")
    if bounds is not None and len(bounds) != B:
        raise ValueError(f"{len(bounds)} bounds for {B} images")
    out.hw, out.bounds = hw, (None if bounds is None else [(int(h), int(w)) for h, w in bounds])
    return out


U8_PLANES, U8_INTERLEAVED = 0, 1          # rn_image_stage_u8's layout codes


def _u8_image(im: Tensor, who: str) -> Tuple[Tensor, int, Tuple[int, int]]:
    """One uint8 ``[3, h, w]`` image -> (a dense tensor, its layout code, (h, w)).  The layout is read from the strides: contiguous is
    planes; strides ``(1, 3 w, 3)`` -- ``torch.from_numpy(hwc).permute(2, 0, 1)``, which ``.to(device)`` preserves -- are interleaved
    (the stride of a dimension of size 1 is free); anything else is made contiguous (planes)."""
    if im.dim() != 3 or im.shape[0] != 3 or im.dtype != torch.uint8:
        raise ValueError(f"{who} expects uint8 [3, h, w] images, got {tuple(im.shape)} {im.dtype}")
    h, w = int(im.shape[1]), int(im.shape[2])
    if im.is_contiguous():
        return im, U8_PLANES, (h, w)
    s = im.stride()
    if h > 0 and w > 0 and s[0] == 1 and (h == 1 or s[1] == 3 * w) and (w == 1 or s[2] == 3):
        return im, U8_INTERLEAVED, (h, w)
    return im.contiguous(), U8_PLANES, (h, w)


def _u8_check(im: Tensor, who: str) -> None:
    "``_u8_image``'s dtype / shape check plus: no empty image (the conversions; the stager words that as \"does not fit\")."
    if im.dim() != 3 or im.shape[0] != 3 or im.dtype != torch.uint8:
        raise ValueError(f"{who} expects uint8 [3, h, w] images, got {tuple(im.shape)} {im.dtype}")
    if im.shape[1] <= 0 or im.shape[2] <= 0:
        raise ValueError(f"{who}: an empty {int(im.shape[1])} x {int(im.shape[2])} image")


def _image_stage_u8(imgs: Sequence[Tensor], layouts: Sequence[int], hw: Sequence[Tuple[int, int]], arena: Tensor, slot: int, in_hw: Tensor,
                    dev: torch.device) -> None:
    B = len(imgs)
    with torch.cuda.device(dev), _timed("image_stage_u8", dev):
        check(lib.rn_image_stage_u8((C.c_void_p * B)(*[im.data_ptr() for im in imgs]), (C.c_int32 * (2 * B))(*[v for s in hw for v in s]),
                                    (C.c_int32 * B)(*layouts), B, _ptr(arena), slot, _ptr(in_hw), _stream(dev)), "rn_image_stage_u8")


def image_stage_u8(images: Sequence[Tensor], out: StagedImages, bounds: Optional[Sequence[Tuple[int, int]]] = None) -> StagedImages:
    """``image_stage`` for the images a decoder gives: CUDA uint8 ``[3, h_b, w_b]`` tensors on ``out``'s device, planes (contiguous) or
    interleaved (strides ``(1, 3 w, 3)``: an HWC array permuted to the code base's shape), converted on the way into the same fp32
    arena (``rn_image_stage_u8``): slot b holds ``float(v) / 255`` -- the correctly rounded quotient, bit for bit what ``image_stage``
    leaves for ``im.to(float32) / 255`` computed on the CPU.  One launch per 64 images on the current stream; no host copy, no
    synchronisation; other strides are made contiguous first.  ValueError for another dtype or shape, a zero size, an image above
    the slot or a wrong count; nothing is written then."""
    dev = _need_dev(out.arena, *images)
    B = len(images)
    if B != out.B:
        raise ValueError(f"{B} images for an arena of {out.B} slots")
    if bounds is not None and len(bounds) != B:
        raise ValueError(f"{len(bounds)} bounds for {B} images")
    imgs, layouts, hw = [], [], []
    for im in images:
        im, layout, (h, w) = _u8_image(im, "image_stage_u8")
        if h <= 0 or w <= 0 or 3 * h * w > out.slot:
            raise ValueError(f"a {h} x {w} image does not fit an arena slot of {out.slot} floats")
        imgs.append(im)
        layouts.append(layout)
        hw.append((h, w))
    _image_stage_u8(imgs, layouts, hw, out.arena, out.slot, out.in_hw, dev)
    out.hw, out.bounds = hw, (None if bounds is None else [(int(h), int(w)) for h, w in bounds])
    return out


def images_u8_to_f32(images: Sequence[Tensor]) -> List[Tensor]:
    """uint8 ``[3, h, w]`` images (planes or interleaved, as ``image_stage_u8`` takes them) -> dense fp32 ``[3, h, w]`` images in [0, 1],
    ``float(v) / 255`` with ONE correctly rounded division: the conversion of ``image_stage_u8`` for images that are not staged.  CUDA
    images: one ``rn_image_stage_u8`` call per 64 images into a fresh buffer (slot: 3 x the largest ``h w``, rounded up to a multiple
    of 4), the results are views of it.  CPU images: ``im.to(float32) / 255`` -- a true division; both give the same bits.  (Never
    ``x.div(255)`` on the device: torch computes that with the rounded reciprocal, which is off by one bit for 126 of the 256 bytes.)"""
    images = list(images)
    if not images:
        return []
    if all(not im.is_cuda for im in images):
        for im in images:
            _u8_check(im, "images_u8_to_f32")
        return [(im.to(torch.float32) / 255).contiguous() for im in images]
    dev = _need_dev(*images)
    imgs, layouts, hw = [], [], []
    for im in images:
        _u8_check(im, "images_u8_to_f32")
        im, layout, (h, w) = _u8_image(im, "images_u8_to_f32")
        imgs.append(im)
        layouts.append(layout)
        hw.append((h, w))
    B = len(imgs)
    slot = (3 * max(h * w for h, w in hw) + 3) // 4 * 4
    arena = torch.empty((B, slot), dtype=torch.float32, device=dev)
    in_hw = torch.empty((B, 2), dtype=torch.int32, device=dev)
    for lo in range(0, B, 64):
        hi = min(lo + 64, B)
        _image_stage_u8(imgs[lo:hi], layouts[lo:hi], hw[lo:hi], arena[lo:hi], slot, in_hw[lo:hi], dev)
    return [arena[b, : 3 * h * w].view(3, h, w) for b, (h, w) in enumerate(hw)]


def resize_plan_dev(block: Optional[Tensor], in_hw: Tensor, short: Optional[int], max_size: int) -> Tuple[Tensor, Tensor]:
    """``rn_resize_plan_dev``: ``short_side_draw`` with the input sizes on the device (``in_hw`` int32 [B, 2], as ``image_stage`` writes
    it) -> (resized sizes int32 [B, 2], box ratios f32 [2B]).  With ``block`` (an ``rn_short_side_state``) the short sides are drawn
    as ``short_side_draw`` draws them and the block's counter advances by one; with ``block=None`` every image gets ``short``.
    One launch for any B on the current stream, no host synchronisation (capturable)."""
    dev = _need_dev(in_hw if block is None else block)
    if block is not None:
        draw_state.check(SHORT_SIDE, block)
    if in_hw.dtype != torch.int32 or in_hw.dim() != 2 or in_hw.shape[1] != 2 or not in_hw.is_contiguous() or in_hw.device != dev:
        raise ValueError(f"in_hw must be a contiguous int32 [B, 2] tensor on {dev}, got {tuple(in_hw.shape)} {in_hw.dtype} on {in_hw.device}")
    B = int(in_hw.shape[0])
    if B == 0:
        raise ValueError("need at least one image size")
    if block is None and (short is None or int(short) != short or int(short) <= 0):
        raise ValueError(f"without a state block the short side must be a positive integer, got {short!r}")
    out_hw = torch.empty((B, 2), dtype=torch.int32, device=dev)
    ratios = torch.empty((2 * B,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), _timed("resize_plan_dev", dev):
        check(lib.rn_resize_plan_dev(_ptr(block), _ptr(in_hw), 0 if block is not None else int(short), int(max_size), B, _ptr(out_hw),
                                     _ptr(ratios), _stream(dev)), "rn_resize_plan_dev")
    return out_hw, ratios


def transform_batch_var(staged: StagedImages, out_hw: Tensor, mean: Sequence[float], std: Sequence[float], Hp: int, Wp: int,
                        out_dtype: torch.dtype = torch.float32, channels_last: bool = False, flags: Optional[Tensor] = None,
                        coef: Optional[Tensor] = None) -> Tensor:
    """``transform_batch_dev`` on staged images (``rn_transform_batch_var``): image b from the arena's slot b, its size from
    ``staged.in_hw`` and its output size from ``out_hw`` (int32 [B, 2], ``resize_plan_dev``), all read on the device; a size no slot
    can hold leaves the image all padding.  Bit-identical to ``transform_batch`` called with the same sizes and canvas on the host."""
    dev = _need_dev(staged.arena, staged.in_hw, out_hw)
    B = staged.B
    if out_hw.dtype != torch.int32 or tuple(out_hw.shape) != (B, 2) or not out_hw.is_contiguous():
        raise ValueError(f"out_hw must be a contiguous int32 [{B}, 2] tensor, got {tuple(out_hw.shape)} {out_hw.dtype}")
    if flags is not None:
        _check_flags(flags, B, dev)
    if coef is not None:
        _check_coef(coef, B, dev)
    if out_dtype not in _DT:
        raise ValueError(f"unsupported output dtype {out_dtype}")
    out = torch.empty((B, 3, Hp, Wp), dtype=out_dtype, device=dev,
                      memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    with torch.cuda.device(dev), _timed("transform_batch", dev):
        if coef is not None:
            check(lib.rn_transform_batch_color(None, None, _ptr(staged.arena), staged.slot, _ptr(staged.in_hw), None, _ptr(out_hw), B,
                                               (C.c_float * 3)(*mean), (C.c_float * 3)(*std), int(Hp), int(Wp), _ptr(out), _DT[out_dtype],
                                               int(bool(channels_last)), _ptr(flags), _ptr(coef), _stream(dev)), "rn_transform_batch_color")
            return out
        check(lib.rn_transform_batch_var(_ptr(staged.arena), staged.slot, _ptr(staged.in_hw), _ptr(out_hw), B, (C.c_float * 3)(*mean),
                                         (C.c_float * 3)(*std), int(Hp), int(Wp), _ptr(out), _DT[out_dtype], int(bool(channels_last)),
                                         _ptr(flags), _stream(dev)), "rn_transform_batch_var")
    return out


def gt_flip_scale_packed_var(gt: PackedGT, in_hw: Tensor, ratios: Tensor, flags: Optional[Tensor] = None) -> PackedGT:
    """``gt_flip_scale_packed_dev`` with the original widths on the device too (``in_hw`` int32 [B, 2], ``StagedImages.in_hw``) --
    ``rn_gt_flip_scale_packed_var``, out of place, bit-identical given the same values."""
    dev = _need_dev(gt.gt_boxes, gt.gt_off, in_hw, ratios, flags)
    if in_hw.dtype != torch.int32 or tuple(in_hw.shape) != (gt.B, 2) or not in_hw.is_contiguous():
        raise ValueError(f"in_hw must be a contiguous int32 [{gt.B}, 2] tensor, got {tuple(in_hw.shape)} {in_hw.dtype}")
    _check_ratios_dev(ratios, gt.B, dev)
    if flags is not None:
        _check_flags(flags, gt.B, dev)
    out = torch.empty_like(gt.gt_boxes)
    with torch.cuda.device(dev), _timed("gt_flip_scale_packed", dev):
        check(lib.rn_gt_flip_scale_packed_var(_ptr(gt.gt_boxes), _ptr(out), _ptr(gt.gt_off), _ptr(in_hw), _ptr(ratios), _ptr(flags), gt.B,
                                              gt.rows, gt.cap_per_image, _stream(dev)), "rn_gt_flip_scale_packed_var")
    return gt.with_boxes(out)


# ---- train-time bbox-safe random crop (augment.BBoxSafeRandomCrop): a second staging pass ------------------------------------
def bbox_crop_draw(block: Tensor, in_hw: Tensor, gt: PackedGT) -> Tuple[Tensor, Tensor, Tensor]:
    """``rn_bbox_crop_draw``: per image the crop rectangle drawn from the block's seed / counter / p around the union of its boxes ->
    (rect int32 [B, 4] = (y0, x0, ch, cw), crop_hw int32 [B, 2] = (ch, cw), the boxes shifted by (x0, y0) in a fresh f32 [rows, 4]
    buffer; rows outside the images' ranges unwritten), then the block's counter advances by one.  ``in_hw``: int32 [B, 2] on the
    device (``StagedImages.in_hw``).  One wave per image plus the counter's single-wave launch, on the current stream, no host
    synchronisation (capturable: each replay draws anew)."""
    dev = _need_dev(block, in_hw, gt.gt_boxes, gt.gt_off)
    draw_state.check(BBOX_CROP, block)
    if in_hw.dtype != torch.int32 or tuple(in_hw.shape) != (gt.B, 2) or not in_hw.is_contiguous():
        raise ValueError(f"in_hw must be a contiguous int32 [{gt.B}, 2] tensor, got {tuple(in_hw.shape)} {in_hw.dtype}")
    if gt.gt_boxes.dtype != torch.float32 or not gt.gt_boxes.is_contiguous() or gt.gt_boxes.data_ptr() % 16:
        raise ValueError("packed GT boxes must be a contiguous, 16-byte aligned f32 [rows, 4] tensor")
    rect = torch.empty((gt.B, 4), dtype=torch.int32, device=dev)
    crop_hw = torch.empty((gt.B, 2), dtype=torch.int32, device=dev)
    out = torch.empty_like(gt.gt_boxes)
    with torch.cuda.device(dev), _timed("bbox_crop_draw", dev):
        check(lib.rn_bbox_crop_draw(_ptr(block), _ptr(gt.gt_boxes), _ptr(gt.gt_off), _ptr(in_hw), gt.B, _ptr(rect), _ptr(crop_hw), _ptr(out),
                                    gt.rows, _stream(dev)), "rn_bbox_crop_draw")
    return rect, crop_hw, out


def image_crop_stage(staged: StagedImages, rect: Tensor, crop_hw: Tensor, out: Optional[StagedImages] = None) -> StagedImages:
    """``rn_image_crop_stage``: image b's window ``rect[b]`` = (y0, x0, ch, cw) of ``staged``, dense at the start of slot b of a second
    arena whose sizes are ``crop_hw`` (int32 [B, 2]; the tensor is kept, not copied) -- a ``StagedImages`` like any other, bit-identical
    to staging ``img[:, y0:y0+ch, x0:x0+cw]``.  ``out``: an arena to write into (its ``in_hw`` is ignored), else one with ``staged``'s
    slot is allocated here.  The host-side ``hw``, ``bounds`` and ``canvas`` are carried over: the host does not know the rectangles.
    One launch on the current stream, a fixed grid, no host synchronisation (capturable)."""
    dev = _need_dev(staged.arena, staged.in_hw, rect, crop_hw)
    B = staged.B
    for name, t, cols in (("rect", rect, 4), ("crop_hw", crop_hw, 2)):
        if t.dtype != torch.int32 or tuple(t.shape) != (B, cols) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous int32 [{B}, {cols}] tensor, got {tuple(t.shape)} {t.dtype}")
    arena = torch.empty_like(staged.arena) if out is None else out.arena
    if arena.device != dev or arena.shape[0] != B or arena.data_ptr() == staged.arena.data_ptr():
        raise ValueError(f"the output arena must be another arena of {B} slots on {dev}")
    res = StagedImages(arena, crop_hw, staged.canvas)
    with torch.cuda.device(dev), _timed("image_crop_stage", dev):
        check(lib.rn_image_crop_stage(_ptr(staged.arena), staged.slot, _ptr(staged.in_hw), _ptr(rect), B, _ptr(arena), res.slot,
                                      _stream(dev)), "rn_image_crop_stage")
    res.hw, res.bounds = list(staged.hw), (None if staged.bounds is None else list(staged.bounds))
    return res


def bbox_crop_staged(crop, staged: StagedImages, packed: PackedGT) -> Tuple[StagedImages, PackedGT]:
    """The bbox-safe random crop of a staged batch (``crop``: an ``augment.BBoxSafeRandomCrop``): ``bbox_crop_draw`` from the object's
    device block, then ``image_crop_stage`` into an arena allocated here, like the other intermediates of a step -> (the cropped
    ``StagedImages``, ``packed.with_boxes(the shifted boxes)``).  The rectangles stay on the device as ``crop.rect``."""
    if packed.B != staged.B:
        raise ValueError(f"packed GT of {packed.B} images for an arena of {staged.B}")
    rect, crop_hw, boxes = bbox_crop_draw(crop.device_block(staged.device), staged.in_hw, packed)
    crop.rect = rect
    return image_crop_stage(staged, rect, crop_hw), packed.with_boxes(boxes)


# ---- train-time shift / scale / rotate (augment.ShiftScaleRotate): a second staging pass --------------------------------------
AFFINE_COEF_WORDS = 16                 # rn_affine_coef: m f32[6], inv f32[6], applied i32, kept i32, reserved i32[2]


def affine_coef_views(coef: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    "(m f32 [B, 6], inv f32 [B, 6], applied i32 [B], kept i32 [B]): views of an ``rn_affine_coef`` tensor (int32 [B, 16])."
    return coef[:, 0:6].view(torch.float32), coef[:, 6:12].view(torch.float32), coef[:, 12], coef[:, 13]


def affine_draw(block: Tensor, in_hw: Tensor, gt: PackedGT) -> Tuple[Tensor, PackedGT]:
    """``rn_affine_draw``: per image the matrices drawn from the block, and the rows of ``gt`` that survive them, packed ->
    (coef int32 [B, 16] = ``rn_affine_coef`` per image, read it through ``affine_coef_views``; a ``PackedGT`` of fresh boxes, labels
    and offsets that shares ``gt.num_fg``; rows past its ``gt_off[B]`` are unwritten), then the block's counter advances by one.
    ``in_hw``: int32 [B, 2] on the device (``StagedImages.in_hw``).  Three launches on the current stream, no atomics, no host
    synchronisation (capturable: each replay draws anew)."""
    dev = _need_dev(block, in_hw, gt.gt_boxes, gt.gt_labels, gt.gt_off)
    draw_state.check(AFFINE, block)
    if in_hw.dtype != torch.int32 or tuple(in_hw.shape) != (gt.B, 2) or not in_hw.is_contiguous():
        raise ValueError(f"in_hw must be a contiguous int32 [{gt.B}, 2] tensor, got {tuple(in_hw.shape)} {in_hw.dtype}")
    if gt.gt_boxes.dtype != torch.float32 or not gt.gt_boxes.is_contiguous() or gt.gt_boxes.data_ptr() % 16:
        raise ValueError("packed GT boxes must be a contiguous, 16-byte aligned f32 [rows, 4] tensor")
    if gt.gt_labels.dtype != torch.int64 or not gt.gt_labels.is_contiguous() or gt.gt_labels.numel() != gt.rows:
        raise ValueError(f"packed GT labels must be a contiguous int64 [{gt.rows}] tensor")
    coef = torch.empty((gt.B, AFFINE_COEF_WORDS), dtype=torch.int32, device=dev)
    out = gt.with_rows(torch.empty_like(gt.gt_boxes), torch.empty_like(gt.gt_labels), torch.empty_like(gt.gt_off))
    with torch.cuda.device(dev), _timed("affine_draw", dev):
        check(lib.rn_affine_draw(_ptr(block), _ptr(gt.gt_boxes), _ptr(gt.gt_labels), _ptr(gt.gt_off), _ptr(in_hw), gt.B, _ptr(coef),
                                 _ptr(out.gt_boxes), _ptr(out.gt_labels), _ptr(out.gt_off), gt.rows, _stream(dev)), "rn_affine_draw")
    return coef, out


def image_warp_stage(staged: StagedImages, coef: Tensor, out: Optional[StagedImages] = None) -> StagedImages:
    """``rn_image_warp_stage``: image b of ``staged`` gathered through ``coef[b]``'s inverse matrix (bilinear, reflect-101) into slot b
    of a second arena with the same sizes -- ``staged.in_hw`` itself is kept, not copied; an image whose ``applied`` is 0 is copied
    bit for bit.  ``out``: an arena to write into (its ``in_hw`` is ignored), else one with ``staged``'s slot is allocated here.  The
    host-side ``hw``, ``bounds`` and ``canvas`` are carried over.  One launch on the current stream, a fixed grid, no host
    synchronisation (capturable)."""
    dev = _need_dev(staged.arena, staged.in_hw, coef)
    B = staged.B
    if coef.dtype != torch.int32 or tuple(coef.shape) != (B, AFFINE_COEF_WORDS) or not coef.is_contiguous():
        raise ValueError(f"coef must be a contiguous int32 [{B}, {AFFINE_COEF_WORDS}] tensor (rn_affine_coef per image), got "
                         f"{tuple(coef.shape)} {coef.dtype}")
    arena = torch.empty_like(staged.arena) if out is None else out.arena
    if arena.device != dev or arena.shape[0] != B or arena.data_ptr() == staged.arena.data_ptr():
        raise ValueError(f"the output arena must be another arena of {B} slots on {dev}")
    res = StagedImages(arena, staged.in_hw, staged.canvas)
    with torch.cuda.device(dev), _timed("image_warp_stage", dev):
        check(lib.rn_image_warp_stage(_ptr(staged.arena), staged.slot, _ptr(staged.in_hw), _ptr(coef), B, _ptr(arena), res.slot,
                                      _stream(dev)), "rn_image_warp_stage")
    res.hw, res.bounds = list(staged.hw), (None if staged.bounds is None else list(staged.bounds))
    return res


def shift_scale_rotate_staged(ssr, staged: StagedImages, packed: PackedGT) -> Tuple[StagedImages, PackedGT]:
    """The shift / scale / rotate of a staged batch (``ssr``: an ``augment.ShiftScaleRotate``): ``affine_draw`` from the object's device
    block, then ``image_warp_stage`` into an arena allocated here, like the other intermediates of a step -> (the warped
    ``StagedImages``, the ``PackedGT`` of the rows that survive).  The coefficients stay on the device as ``ssr.coef``."""
    if packed.B != staged.B:
        raise ValueError(f"packed GT of {packed.B} images for an arena of {staged.B}")
    coef, gt = affine_draw(ssr.device_block(staged.device), staged.in_hw, packed)
    ssr.coef = coef
    return image_warp_stage(staged, coef), gt


BOX_DECODES = ("reference", "standard")                        # RN_BOX_DECODE_REFERENCE / RN_BOX_DECODE_STANDARD, by index


def _decode_code(decode: str) -> int:
    if decode not in BOX_DECODES:
        raise ValueError(f"decode must be one of {BOX_DECODES}, got {decode!r}")
    return BOX_DECODES.index(decode)


def decode_clip(deltas: Tensor, anchors: Tensor, image_hw: Optional[Tensor],
                reg_w: Sequence[float] = (1.0, 1.0, 1.0, 1.0), decode: str = "reference") -> Tensor:
    """K4.  deltas [B,A,4] or [A,4]; image_hw i32 [B,2] (device) or None.  -> f32 boxes, same leading shape.
    ``decode``: "reference" (sizes from ``exp(dx)``, ``exp(dy)``: the reference's quirk Q4) or "standard" (sizes from ``dw``, ``dh``
    clipped at ``BOX_XFORM_CLIP``: the inverse of ``bbox_2_activ``; the numbered rule is in include/retinanet_hip.h)."""
    kind = _decode_code(decode)
    dev = _need_dev(deltas, anchors, image_hw)
    squeeze = deltas.dim() == 2
    d = _c(deltas[None] if squeeze else deltas)
    B, A, _ = d.shape
    anchors, bstride = _anchor_args(anchors, B, A)
    out = torch.empty((B, A, 4), dtype=torch.float32, device=dev)
    rw = (C.c_float * 4)(*reg_w)
    with torch.cuda.device(dev):
        check(lib.rn_decode_clip_kind(_ptr(d), _dtype_code(d), B, A, _ptr(anchors), bstride, _ptr(image_hw), rw, kind,
                                      _ptr(out), _stream(dev)), "rn_decode_clip_kind")
    return out[0] if squeeze else out


def nms_segments(boxes: Tensor, scores: Tensor, seg_off: Tensor, iou_thr: float) -> Tuple[Tensor, Tensor]:
    """K6 at the op boundary (torchvision.ops.nms batched over segments).
    boxes f32 [N,4], scores f32 [N], seg_off i32 [S+1] (device).
    -> (keep i64 [N] (per segment: indices relative to the segment start, score order), keep_count i32 [S])."""
    dev = _need_dev(boxes, scores, seg_off)
    boxes = _c(boxes.float()).reshape(-1, 4)
    scores = _c(scores.float()).reshape(-1)
    N, S = boxes.shape[0], seg_off.numel() - 1
    keep = torch.empty((max(N, 1),), dtype=torch.int64, device=dev)
    count = torch.empty((S,), dtype=torch.int32, device=dev)
    ws_bytes = lib.rn_nms_workspace_bytes(N, S)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.rn_nms_segments(_ptr(boxes), _ptr(scores), _ptr(seg_off), S, N, iou_thr, _ptr(keep), _ptr(count),
                                  _ptr(ws), ws_bytes, _stream(dev)), "rn_nms_segments")
    return keep[:N], count


NMS_KINDS = ("hard", "soft_linear", "soft_gaussian")            # RN_NMS_HARD / RN_NMS_SOFT_LINEAR / RN_NMS_SOFT_GAUSSIAN, by index


def _nms_params(nms: str, sigma: float, min_score: float, max_keep: Optional[int] = None) -> RnNmsParams:
    if nms not in NMS_KINDS:
        raise ValueError(f"nms must be one of {NMS_KINDS}, got {nms!r}")
    return RnNmsParams(NMS_KINDS.index(nms), float(sigma), float(min_score), int(max_keep) if max_keep else 0)


def soft_nms_segments(boxes: Tensor, scores: Tensor, seg_off: Tensor, iou_thr: float, method: str, sigma: float = 0.5,
                      min_score: float = 1e-3, max_keep: Optional[int] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """Soft-NMS (the rule next to K6 in include/retinanet_hip.h; ``box_utils.soft_nms_reference``) batched over segments, with
    ``nms_segments``' inputs.  ``method``: "soft_linear" (scores of boxes overlapping a picked one by more than ``iou_thr`` are
    multiplied by 1 - IoU) or "soft_gaussian" (by exp(-IoU^2 / ``sigma``), no threshold); a segment ends when its best remaining
    score is not above ``min_score`` or ``max_keep`` (None: no cap) entries are kept.  Scores are expected >= 0; not checked.
    -> (keep i64 [N] (per segment: indices relative to the segment start, in pick order), keep_scores f32 [N] (the rescored values
    at the same positions, 0 elsewhere), keep_count i32 [S])."""
    if method == "hard":
        raise ValueError('method must be "soft_linear" or "soft_gaussian": the hard kind is nms_segments')
    params = _nms_params(method, sigma, min_score, max_keep)
    dev = _need_dev(boxes, scores, seg_off)
    boxes = _c(boxes.float()).reshape(-1, 4)
    scores = _c(scores.float()).reshape(-1)
    N, S = boxes.shape[0], seg_off.numel() - 1
    keep = torch.empty((max(N, 1),), dtype=torch.int64, device=dev)
    keep_scores = torch.empty((max(N, 1),), dtype=torch.float32, device=dev)
    count = torch.empty((S,), dtype=torch.int32, device=dev)
    ws_bytes = lib.rn_nms_workspace_bytes(N, S)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.rn_soft_nms_segments(_ptr(boxes), _ptr(scores), _ptr(seg_off), S, N, iou_thr, C.byref(params), _ptr(keep),
                                       _ptr(keep_scores), _ptr(count), _ptr(ws), ws_bytes, _stream(dev)), "rn_soft_nms_segments")
    return keep[:N], keep_scores[:N], count


def nms(boxes: Tensor, scores: Tensor, iou_threshold: float) -> Tensor:
    """Drop-in for ``torchvision.ops.nms(boxes, scores, iou_threshold) -> int64[k]`` (one segment).
    Reading the kept count is the one host sync, exactly as in the op it replaces."""
    n = boxes.shape[0]
    if n == 0:
        return torch.empty((0,), dtype=torch.int64, device=boxes.device)
    off = torch.tensor([0, n], dtype=torch.int32, device=boxes.device)
    keep, count = nms_segments(boxes, scores, off, iou_threshold)
    return keep[: int(count.item())]


def detect(cls: Tensor, deltas: Tensor, anchors, image_sizes: Sequence[Tuple[int, int]], score_thr: float,
           min_box: float, nms_thr: float, max_det: int, reg_w: Sequence[float] = (1.0, 1.0, 1.0, 1.0),
           max_candidates: Optional[int] = None, decode: str = "reference", nms: str = "hard", nms_sigma: float = 0.5,
           nms_min_score: float = 1e-3) -> List[dict]:
    """K4-K7 for a batch: -> [{"boxes" f32[n,4], "scores" f32[n], "labels" i64[n]}], n <= max_det.
    ``decode``: the box decode of the chain, one of ``BOX_DECODES`` (``decode_clip``).  ``nms``: the chain's NMS, one of ``NMS_KINDS``
    (``detect_levels``).

    One host sync at the end (the ragged result sizes have to reach Python, as in the
    reference's list-of-dicts contract).  If an image has more candidates than the workspace
    was sized for, the call is repeated once with the exact worst case (A*K)."""
    return detect_levels([cls], [deltas], anchors, image_sizes, score_thr, min_box, nms_thr, max_det, reg_w, max_candidates,
                         decode=decode, nms=nms, nms_sigma=nms_sigma, nms_min_score=nms_min_score)


def detect_levels(cls_levels: Sequence[Tensor], box_levels: Sequence[Tensor], anchors, image_sizes: Sequence[Tuple[int, int]],
                  score_thr: float, min_box: float, nms_thr: float, max_det: int,
                  reg_w: Sequence[float] = (1.0, 1.0, 1.0, 1.0), max_candidates: Optional[int] = None,
                  enqueue_only: Optional[list] = None, image_hw_dev: Optional[Tensor] = None, padded: bool = False,
                  decode: str = "reference", nms: str = "hard", nms_sigma: float = 0.5, nms_min_score: float = 1e-3):
    """``detect`` on per-level head outputs (cls_levels[l] [B,A_l,K], box_levels[l] [B,A_l,4]) without
    concatenating them; identical results to ``detect(torch.cat(cls_levels, 1), torch.cat(box_levels, 1), ...)``.
    ``image_hw_dev`` (int32 [B, 2] on the outputs' device, e.g. ``resize_plan_dev``'s sizes): the image sizes the boxes are clipped to,
    used instead of an upload of ``image_sizes`` (which may then be None).  ``padded``: enqueue the chain ONCE and return the padded
    device outputs ``(out_boxes [B, max_det, 4], out_scores, out_labels, meta i32 [2, B] = counts | status)`` without reading
    anything back -- no synchronisation and no retry: ``status[b] != 0`` tells the caller that ``max_candidates`` (an int, None for the
    default, or "all" for the worst case A * K) was too small for image b.  ``decode``: the box decode, one of ``BOX_DECODES``
    (``decode_clip``); every form of the call -- padded, enqueue-only, the overflow retry -- runs the chain with it.
    ``nms``: the per-class NMS, one of ``NMS_KINDS`` -- "hard" (greedy NMS at ``nms_thr``: the reference's, the same launches as
    before the kinds existed), "soft_linear" (Soft-NMS with ``nms_thr`` as the linear threshold) or "soft_gaussian" (``nms_sigma``);
    the soft kinds end a class at ``nms_min_score`` and return the rescored values as ``scores`` (``soft_nms_segments``; the rule is
    next to K6 in the header).  Every form of the call runs the chain with it."""
    kind = _decode_code(decode)
    nms_params = _nms_params(nms, nms_sigma, nms_min_score)
    L = len(cls_levels)
    if L == 0 or L > _lib.RN_MAX_LEVELS or len(box_levels) != L:
        raise ValueError("need 1..8 levels of (cls, box) outputs")
    dev = _need_dev(*cls_levels, *box_levels)
    dt = cls_levels[0].dtype
    for c, d in zip(cls_levels, box_levels):
        if c.dim() != 3 or d.dim() != 3 or c.shape[:2] != d.shape[:2] or d.shape[-1] != 4 or c.dtype != dt \
                or c.shape[0] != cls_levels[0].shape[0] or c.shape[2] != cls_levels[0].shape[2]:
            raise ValueError(f"bad head output shapes {tuple(c.shape)} / {tuple(d.shape)}")
    cls_levels = [_c(c) for c in cls_levels]
    box_levels = [_c(d if d.dtype == dt else d.to(dt)) for d in box_levels]
    B, _, K = cls_levels[0].shape
    counts = [int(c.shape[1]) for c in cls_levels]
    A = sum(counts)
    if not isinstance(anchors, Tensor):
        first = anchors[0]
        anchors = first if all(a is first or a.data_ptr() == first.data_ptr() for a in anchors) else torch.stack(list(anchors))
    anchors, bstride = _anchor_args(anchors.to(dev), B, A)
    if image_hw_dev is not None:
        if image_hw_dev.dtype != torch.int32 or tuple(image_hw_dev.shape) != (B, 2) or not image_hw_dev.is_contiguous() \
                or image_hw_dev.device != dev:
            raise ValueError(f"image_hw_dev must be a contiguous int32 [{B}, 2] tensor on {dev}, got {tuple(image_hw_dev.shape)} "
                             f"{image_hw_dev.dtype} on {image_hw_dev.device}")
        hw = image_hw_dev
    else:
        hw = image_hw_tensor(image_sizes, dev)
    params = RnDetectParams(score_thr, min_box, nms_thr, int(max_det), (C.c_float * 4)(*reg_w))
    if isinstance(max_candidates, str):
        if max_candidates != "all":
            raise ValueError(f"max_candidates: expected an int, None or 'all', got {max_candidates!r}")
        cap = A * K
    else:
        cap = int(max_candidates) if max_candidates else min(A * K, 1 << 18)
    out_boxes = torch.empty((B, max_det, 4), dtype=torch.float32, device=dev)
    out_scores = torch.empty((B, max_det), dtype=torch.float32, device=dev)
    out_labels = torch.empty((B, max_det), dtype=torch.int64, device=dev)
    meta = torch.empty((2, B), dtype=torch.int32, device=dev)          # [0] = count, [1] = status
    arr = lambda ts: (C.c_void_p * L)(*[t.data_ptr() for t in ts])
    while True:
        ws_bytes = lib.rn_detect_workspace_bytes(B, A, K, cap)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)

        def enqueue():
            check(lib.rn_detect_levels_nms(arr(cls_levels), arr(box_levels), (C.c_int64 * L)(*counts), L, _dtype_code(cls_levels[0]),
                                           B, K, _ptr(anchors), bstride, _ptr(hw), C.byref(params), kind, C.byref(nms_params), cap,
                                           _ptr(out_boxes), _ptr(out_scores), _ptr(out_labels), _ptr(meta[0]), _ptr(meta[1]), _ptr(ws),
                                           ws_bytes, _stream(dev)), "rn_detect_levels_nms")
        if enqueue_only is not None:          # (bench.py: the chain's launches as a closure -- for a hipGraph capture -- instead of running them)
            enqueue_only.append(enqueue)
            enqueue_only.append((out_boxes, out_scores, out_labels, meta, ws, hw, anchors, cls_levels, box_levels))     # keep-alive
            return []
        with torch.cuda.device(dev), _timed("detect", dev):
            enqueue()
        if padded:                            # (graph.CapturedPredict: the outputs stay on the device, rn_detect_finish_var reads them)
            return out_boxes, out_scores, out_labels, meta
        meta_h = meta.cpu()                                              # the one sync
        if not bool(meta_h[1].any()) or cap >= A * K:
            break
        cap = A * K
    counts = meta_h[0].tolist()
    return [{"boxes": out_boxes[b, :n], "scores": out_scores[b, :n], "labels": out_labels[b, :n]}
            for b, n in enumerate(counts)]


# ---- the end of predict on the device (graph.CapturedPredict) ------------------------------------------------------------------
def _up16(v: int) -> int:
    return (int(v) + 15) & ~15


def detect_result_layout(B: int, max_det: int) -> dict:
    """Byte offsets of ``rn_detect_finish_var``'s result block (``include/retinanet_hip.h``): counts i32[B] at 0, status i32[B],
    then -- each on a 16-byte boundary -- boxes f32[B][max_det][4], scores f32[B][max_det], labels i64[B][max_det]; ``total`` =
    ``rn_detect_result_bytes(B, max_det)``."""
    B, max_det = int(B), int(max_det)
    if B <= 0 or max_det <= 0:
        raise ValueError(f"need B >= 1 and max_det >= 1, got {B}, {max_det}")
    rows = B * max_det
    boxes = _up16(8 * B)
    scores = boxes + 16 * rows
    labels = _up16(scores + 4 * rows)
    return {"counts": 0, "status": 4 * B, "boxes": boxes, "scores": scores, "labels": labels, "total": _up16(labels + 8 * rows)}


def detect_result_views(block: Tensor, B: int, max_det: int) -> dict:
    """Typed views of a result block (a uint8 tensor of ``detect_result_layout(B, max_det)["total"]`` bytes, on any device):
    counts / status int32 [B], boxes f32 [B, max_det, 4], scores f32 [B, max_det], labels int64 [B, max_det]."""
    lay = detect_result_layout(B, max_det)
    if block.dtype != torch.uint8 or block.dim() != 1 or block.numel() != lay["total"] or not block.is_contiguous():
        raise ValueError(f"a result block for B={B}, max_det={max_det} is a contiguous uint8 tensor of {lay['total']} bytes, "
                         f"got {tuple(block.shape)} {block.dtype}")
    rows = int(B) * int(max_det)
    part = lambda name, nbytes, dt: block[lay[name]:lay[name] + nbytes].view(dt)
    return {"counts": part("counts", 4 * B, torch.int32), "status": part("status", 4 * B, torch.int32),
            "boxes": part("boxes", 16 * rows, torch.float32).view(B, max_det, 4),
            "scores": part("scores", 4 * rows, torch.float32).view(B, max_det),
            "labels": part("labels", 8 * rows, torch.int64).view(B, max_det)}


def detect_result_dicts(block: Tensor, B: int, max_det: int) -> List[dict]:
    "A result block (host or device) as ``Retinanet.predict``'s list of dicts: views of the block, one host read of the counts."
    v = detect_result_views(block, B, max_det)
    counts = [min(max(int(n), 0), int(max_det)) for n in v["counts"].tolist()]
    return [{"boxes": v["boxes"][b, :n], "scores": v["scores"][b, :n], "labels": v["labels"][b, :n]} for b, n in enumerate(counts)]


def detect_finish_reference(out_boxes, out_scores, out_labels, out_count, out_status, in_hw, out_hw):
    """``rn_detect_finish_var`` restated in numpy (the tests' yardstick): the same block, byte for byte, as a uint8 array.  The two
    roundings are the kernel's: fp32 ratio = fp32(original) / fp32(resized), then one fp32 multiply per coordinate."""
    import numpy as np
    boxes = np.ascontiguousarray(out_boxes, dtype=np.float32)
    B, max_det = int(boxes.shape[0]), int(boxes.shape[1])
    lay = detect_result_layout(B, max_det)
    count = np.asarray(out_count, dtype=np.int32).reshape(B)
    in_hw, out_hw = np.asarray(in_hw, dtype=np.int32).reshape(B, 2), np.asarray(out_hw, dtype=np.int32).reshape(B, 2)
    rb = np.zeros((B, max_det, 4), np.float32)
    rs = np.zeros((B, max_det), np.float32)
    rl = np.zeros((B, max_det), np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = in_hw.astype(np.float32) / out_hw.astype(np.float32)              # [B, 2] = (rh, rw)
        for b in range(B):
            n = min(max(int(count[b]), 0), max_det)
            rh, rw = ratio[b]
            rb[b, :n] = boxes[b, :n] * np.array([rw, rh, rw, rh], np.float32)
            rs[b, :n] = np.asarray(out_scores, dtype=np.float32)[b, :n]
            rl[b, :n] = np.asarray(out_labels, dtype=np.int64)[b, :n]
    block = np.zeros(lay["total"], np.uint8)
    for name, arr in (("counts", count), ("status", np.asarray(out_status, dtype=np.int32).reshape(B)), ("boxes", rb), ("scores", rs),
                      ("labels", rl)):
        raw = np.frombuffer(np.ascontiguousarray(arr).tobytes(), np.uint8)
        block[lay[name]:lay[name] + raw.size] = raw
    return block


def detect_finish_var(out_boxes: Tensor, out_scores: Tensor, out_labels: Tensor, meta: Tensor, in_hw: Tensor, out_hw: Tensor,
                      out: Optional[Tensor] = None) -> Tensor:
    """``rn_detect_finish_var``: ``transform.postprocess`` on the device.  The padded outputs of ``detect_levels(padded=True)`` (``meta``
    int32 [2, B] = counts | status), the original sizes ``in_hw`` (int32 [B, 2], ``StagedImages.in_hw``) and the resized ones
    ``out_hw`` (``resize_plan_dev``) -> ONE result block (uint8 [``detect_result_layout``'s total]; ``out``: written in place when
    given) holding counts, status and the rescaled boxes / scores / labels with every row past an image's count zeroed.  One launch
    for any B on the current stream, no synchronisation (capturable)."""
    dev = _need_dev(out_boxes, out_scores, out_labels, meta, in_hw, out_hw, out)
    if out_boxes.dim() != 3 or out_boxes.shape[2] != 4 or out_boxes.dtype != torch.float32 or not out_boxes.is_contiguous():
        raise ValueError(f"out_boxes must be a contiguous f32 [B, max_det, 4] tensor, got {tuple(out_boxes.shape)} {out_boxes.dtype}")
    B, max_det = int(out_boxes.shape[0]), int(out_boxes.shape[1])
    if B == 0 or max_det == 0:
        raise ValueError("need at least one image and one row per image")
    for name, t, dt, shape in (("out_scores", out_scores, torch.float32, (B, max_det)), ("out_labels", out_labels, torch.int64, (B, max_det)),
                               ("meta", meta, torch.int32, (2, B)), ("in_hw", in_hw, torch.int32, (B, 2)), ("out_hw", out_hw, torch.int32, (B, 2))):
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dt} {list(shape)} tensor, got {tuple(t.shape)} {t.dtype}")
    total = detect_result_layout(B, max_det)["total"]
    if out is None:
        out = torch.empty((total,), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or out.dim() != 1 or out.numel() != total or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 tensor of {total} bytes, got {tuple(out.shape)} {out.dtype}")
    with torch.cuda.device(dev), _timed("detect_finish", dev):
        check(lib.rn_detect_finish_var(_ptr(out_boxes), _ptr(out_scores), _ptr(out_labels), _ptr(meta[0]), _ptr(meta[1]), _ptr(in_hw),
                                       _ptr(out_hw), B, max_det, _ptr(out), total, _stream(dev)), "rn_detect_finish_var")
    return out


# --------------------------------------------------------------------------- #
# COCO bbox AP on the device (coco_eval.DeviceBBoxEval, csrc/eval.hip)
def _eval_arg(name: str, t: Tensor, dtype: torch.dtype, shape: Tuple[int, ...]) -> None:
    if not isinstance(t, Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        got = f"{tuple(t.shape)} {t.dtype}" if isinstance(t, Tensor) else type(t).__name__
        raise ValueError(f"{name} must be a contiguous {dtype} {list(shape)} tensor, got {got}")


def _eval_dims(iou_thrs: Tensor, area_rng: Tensor) -> Tuple[int, int]:
    T, A = int(iou_thrs.numel()), int(area_rng.shape[0]) if area_rng.dim() == 2 else -1
    _eval_arg("iou_thrs", iou_thrs, torch.float64, (T,))
    _eval_arg("area_rng", area_rng, torch.float64, (A, 2))
    if not (1 <= T <= 32 and 1 <= A <= 8 and A * T <= 64):
        raise ValueError(f"need 1 <= T <= 32 thresholds and 1 <= A <= 8 area ranges with A * T <= 64 (the masks are 64 bits), got T={T}, A={A}")
    return T, A


def eval_match(dt_boxes: Tensor, gt_xywh: Tensor, gt_area: Tensor, gt_crowd: Tensor, pairs: Tensor, iou_thrs: Tensor, area_rng: Tensor,
               max_det: int = 100) -> Tuple[Tensor, Tensor, Tensor]:
    """``rn_eval_match``: ``BBoxEval._evaluate_img`` for every (image, category) pair at once.  ``dt_boxes`` f32 [D, 4] xyxy, grouped by
    pair and sorted by descending score inside a pair; ``gt_xywh`` f64 [G, 4], ``gt_area`` f64 [G], ``gt_crowd`` uint8 [G], grouped by
    pair; ``pairs`` int32 [P, 4] = (dt begin, dt end, gt begin, gt end); ``iou_thrs`` f64 [T], ``area_rng`` f64 [A, 2] ->
    (matched int64 [D], ignored int64 [D]: bit ``a * T + t``; gt_ignored uint8 [G]: bit ``a``).  One launch on the current stream,
    no atomics, no host synchronisation."""
    D, G, P = int(dt_boxes.shape[0]), int(gt_area.shape[0]), int(pairs.shape[0])
    _eval_arg("dt_boxes", dt_boxes, torch.float32, (D, 4))
    _eval_arg("gt_xywh", gt_xywh, torch.float64, (G, 4))
    _eval_arg("gt_area", gt_area, torch.float64, (G,))
    _eval_arg("gt_crowd", gt_crowd, torch.uint8, (G,))
    _eval_arg("pairs", pairs, torch.int32, (P, 4))
    T, A = _eval_dims(iou_thrs, area_rng)
    if int(max_det) < 1:
        raise ValueError(f"max_det must be >= 1, got {max_det}")
    dev = _need_dev(dt_boxes, gt_xywh, gt_area, gt_crowd, pairs, iou_thrs, area_rng)
    dt_boxes = _aligned(dt_boxes, 16)
    matched = torch.empty((D,), dtype=torch.int64, device=dev)
    ignored = torch.empty((D,), dtype=torch.int64, device=dev)
    gt_ignored = torch.empty((G,), dtype=torch.uint8, device=dev)
    gt_state = torch.empty((G,), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev), _timed("eval_match", dev):
        check(lib.rn_eval_match(_ptr(dt_boxes), D, _ptr(gt_xywh), _ptr(gt_area), _ptr(gt_crowd), G, _ptr(pairs), P, _ptr(iou_thrs), T,
                                _ptr(area_rng), A, int(max_det), _ptr(matched), _ptr(ignored), _ptr(gt_ignored), _ptr(gt_state),
                                _stream(dev)), "rn_eval_match")
    return matched, ignored, gt_ignored


def eval_accumulate(matched: Tensor, ignored: Tensor, rank: Tensor, cat_off: Tensor, npig: Tensor, rec_thrs: Tensor, max_dets: Tensor,
                    T: int) -> Tuple[Tensor, Tensor]:
    """``rn_eval_accumulate``: the precision / recall arrays of ``BBoxEval.evaluate``.  ``matched`` / ``ignored`` int64 [N] and ``rank``
    int32 [N]: per category its detections sorted by descending score (stable over "image id ascending, then rank"), category k at
    ``[cat_off[k], cat_off[k + 1])`` (``cat_off`` int64 [K + 1]); ``npig`` int64 [K, A]; ``rec_thrs`` f64 [R]; ``max_dets`` int32 [M];
    ``T``: the number of thresholds in the masks -> (precision f64 [T, R, K, A, M], recall f64 [T, K, A, M]).  One launch on the
    current stream, no atomics, no host synchronisation."""
    N, K, R, M = int(matched.numel()), int(cat_off.numel()) - 1, int(rec_thrs.numel()), int(max_dets.numel())
    A = int(npig.shape[1]) if npig.dim() == 2 else -1
    _eval_arg("matched", matched, torch.int64, (N,))
    _eval_arg("ignored", ignored, torch.int64, (N,))
    _eval_arg("rank", rank, torch.int32, (N,))
    _eval_arg("cat_off", cat_off, torch.int64, (K + 1,))
    _eval_arg("npig", npig, torch.int64, (K, A))
    _eval_arg("rec_thrs", rec_thrs, torch.float64, (R,))
    _eval_arg("max_dets", max_dets, torch.int32, (M,))
    T = int(T)
    if K < 0 or not (1 <= T <= 32 and 1 <= A <= 8 and A * T <= 64) or M < 1 or not 1 <= R <= 1024:
        raise ValueError(f"need K >= 0, 1 <= T <= 32, 1 <= A <= 8, A * T <= 64, M >= 1 and 1 <= R <= 1024, got K={K}, T={T}, A={A}, M={M}, R={R}")
    dev = _need_dev(matched, ignored, rank, cat_off, npig, rec_thrs, max_dets)
    precision = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
    recall = torch.empty((T, K, A, M), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev), _timed("eval_accumulate", dev):
        check(lib.rn_eval_accumulate(_ptr(matched), _ptr(ignored), _ptr(rank), N, _ptr(cat_off), _ptr(npig), _ptr(rec_thrs), R, _ptr(max_dets), M,
                                     T, K, A, _ptr(precision), _ptr(recall), _stream(dev)), "rn_eval_accumulate")
    return precision, recall
