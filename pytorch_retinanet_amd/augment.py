"""Train-time augmentation decided on the device.

The reference trains with one augmentation, a random horizontal flip with p = 0.5 (``hparams.yaml`` ``transforms``:
``albumentations.HorizontalFlip``; ``RandomHorizontalFlip(prob=0.5)`` for COCO), applied per image on the host before the model's
transform.  ``RandomHorizontalFlip`` here does the same inside the model's transform (``GeneralizedRCNNTransform.hflip``):

* the decision for the B images of a batch is one tiny launch (``rn_hflip_draw``) that reads seed / counter / p from a device block
  this object owns and advances the counter, so a train step captured into a hipGraph draws new flips at every replay;
* the flip itself is folded into the transform kernel's gather (``rn_transform_batch_flip``) and the box resize
  (``rn_gt_flip_scale_many`` / ``rn_gt_flip_scale_packed``).

The draw for image b at counter value n is a pure function of (seed, n, b, p) -- ``draw`` restates it in Python, and it is what CPU
tensors use.  Eager steps and graph replays advance the same counter, so the stream of decisions does not depend on how a step ran.

``RandomShortSide`` is multi-scale training -- torchvision's ``min_size`` tuple: one short side per image and step -- made the same
way (``GeneralizedRCNNTransform.scale_jitter``).  A short side drawn on the host changes the padded canvas from step to step, so
nearly every batch is a new graph signature and the step stays on the eager path.  Here the canvas is fixed: the host sizes it for
the largest candidate, and the sizes themselves are drawn on the device inside the step (``rn_short_side_draw``), read by the
transform kernel (``rn_transform_batch_dev``) and the box kernels (``rn_gt_flip_scale_many_dev`` / ``_packed_dev``) from device
memory.  The price is deliberate: the conv stack processes the whole canvas whatever was drawn, so a small draw saves no compute.

``ColorJitter`` is the photometric half (``GeneralizedRCNNTransform.color_jitter``): torchvision's ``ColorJitter`` -- brightness,
contrast, saturation and hue in a random order, each with a factor drawn from its range -- on fp32 RGB images in [0, 1].  The pin is
torchvision 0.8's TENSOR algorithm (``transforms.functional_tensor``; ``apply_color_ops`` below restates it in torch).  albumentations'
``ColorJitter`` takes the same arguments but works on uint8 through OpenCV, so its results differ slightly; an hparams entry naming
either maps onto this class.  Per image one launch draws ``rn_color_coef`` (four factors and the order: ``rn_color_jitter_draw``), one
pair of launches computes the contrast's mean gray when a contrast is enabled (``rn_color_mean``), and the operations run inside the
transform kernel on every source pixel it reads (``rn_transform_batch_color``) -- all inside the captured step, each replay a new draw.

``BBoxSafeRandomCrop`` is the geometric augmentation detection users add next (``GeneralizedRCNNTransform.crop``): albumentations'
``BBoxSafeRandomCrop`` with ``erosion_rate = 0`` in intent, on integer pixels -- not bit-compatible with albumentations' float rounding.
It drops no box, so the GT counts and offsets of a captured step do not change.  On staged images with packed GT it is a second
staging pass: ``rn_bbox_crop_draw`` draws a rectangle per image around the union of its boxes and shifts the boxes,
``rn_image_crop_stage`` copies each window densely into a second arena, and everything downstream runs unchanged on that arena --
bit-identical to running on the sliced tensors.  Other inputs draw the same rectangles on the host (one synchronisation on CUDA).

``ShiftScaleRotate`` is the second transform of the reference's published recipe (``demo.ipynb``: ``HorizontalFlip``,
``ShiftScaleRotate``, ``RandomBrightnessContrast``): albumentations' ``ShiftScaleRotate`` with bilinear interpolation and the reflect-101
border in intent, not bit for bit.  It is a second staging pass as well -- ``rn_affine_draw`` draws a matrix per image and packs the GT
rows that survive it (rows can disappear: the offsets change), ``rn_image_warp_stage`` gathers each image into a second arena -- and
its Python restatement (``draw_coefs``, ``warp_boxes``, ``warp_image``) serves every other input on the host.

``RandomBrightnessContrast`` is the third (``GeneralizedRCNNTransform.brightness_contrast``): albumentations' ``alpha x + beta ref`` on
fp32 RGB in [0, 1], with the LUT's clip and without its uint8 quantisation.  Its two coefficients per image ride in the colour jitter's
``rn_color_coef`` rows (``rn_brightness_contrast_draw``; by-mean: ``rn_brightness_contrast_mean``) and the transform kernel applies them
behind the jitter's operations.  It is opt-in from the hparams (``SimpleTrainer(device_brightness_contrast=True)``).
"""
import logging
import math
from typing import Callable, Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import draw_state
from .draw_state import COLOR_IDENTITY, COLOR_OPS, SHORT_SIDE_MAX

__all__ = ["RandomHorizontalFlip", "RandomShortSide", "ColorJitter", "BBoxSafeRandomCrop", "ShiftScaleRotate", "RandomBrightnessContrast",
           "hflip_u", "apply_color_ops", "apply_brightness_contrast"]

_M64 = 2 ** 64 - 1


def hflip_u(seed: int, counter: int, b: int) -> float:
    "The uniform in [0, 1) (24 bits) behind image b's decision at ``counter`` (``csrc/augment.hip``)."
    z = (seed ^ (counter * 0x9E3779B97F4A7C15) ^ ((b + 1) * 0xD1B54A32D192ED03)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return (z >> 40) * 2.0 ** -24


def _ops():
    "The kernel launchers, imported at first use: the restatements and the host draws of this module need no device."
    from . import ops
    return ops


def _check_p(p) -> float:
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"flip probability must be in [0, 1], got {p}")
    return float(np.float32(p))


class _DrawStream:
    """What the augmentations below share: a stream of draws (seed, counter) and, from the first CUDA batch on, the device block that a
    draw kernel reads and whose counter it advances (``_layout``: its ``draw_state`` table; ``_fields()``: its fields besides seed and
    counter, from this object's settings).  A captured step holds the block's address, so it is created once, outside any capture,
    and never replaced; a replay advances the device counter, not ``_counter``, so ``counter`` reads it back; and a setting is
    written as its own fields only (``_write``): the block is never rebuilt from host values."""
    _layout: draw_state.Layout

    def __init__(self, seed: int):
        self.base_seed = int(seed) & _M64
        self._seed, self._counter = self.base_seed, 0
        self._block: Optional[Tensor] = None          # the state block on the device of the first CUDA batch (kept for good)

    def _fields(self) -> Dict[str, object]:
        raise NotImplementedError

    def _device_block(self, device: torch.device) -> Tensor:
        "The block on the CUDA ``device``, created at the first call (which must not be inside a capture)."
        device = torch.device(device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._block is None:
            self._block = draw_state.new(self._layout, device, seed=self._seed, counter=self._counter, **self._fields())
        elif self._block.device != device:
            # (a captured step holds the block's address: it is never replaced while this object lives)
            raise RuntimeError(f"{type(self).__name__}: its state lives on {self._block.device}, not {device}; use one object per device")
        return self._block

    def _write(self, **fields) -> None:
        "Settings into the device block, if there is one (no re-capture needed; not inside a capture)."
        if self._block is not None:
            draw_state.write(self._layout, self._block, **fields)

    def _host_draw(self, draw: Callable):
        "``draw(n)`` at the next counter value n, and the counter advanced by one -- on the device too, with a block (a synchronisation)."
        n = self.counter
        out = draw(n)
        self._counter = n + 1
        self._write(counter=n + 1)
        return out

    @property
    def seed(self) -> int:
        return self._seed

    def reseed(self, seed: int, counter: int = 0) -> None:
        "Start a new stream of draws (seed, counter); not inside a capture."
        self._seed, self._counter = int(seed) & _M64, int(counter)
        self._write(seed=self._seed, counter=self._counter)

    def set_rank(self, rank: int) -> None:
        """One stream per data-parallel rank: seed = ``base_seed`` (the constructor's) + rank, the counter kept.  Without it every rank
        would make the same draws at the same batch positions."""
        self.reseed((self.base_seed + int(rank)) & _M64, self.counter)

    @property
    def counter(self) -> int:
        "Batches drawn so far (with the device block: one read-back, i.e. a synchronisation)."
        if self._block is not None:
            return int(draw_state.read(self._layout, self._block)[1])
        return self._counter

    def state_dict(self) -> Dict[str, object]:
        return {"seed": self._seed, "counter": self.counter}

    def load_state_dict(self, state: Dict[str, object]) -> None:
        self.reseed(int(state["seed"]), int(state["counter"]))


class _ProbStream(_DrawStream):
    "A stream whose draws apply with probability ``p``, a field of its block."

    def __init__(self, p: float, seed: int):
        super().__init__(seed)
        self._p = _check_p(p)

    def _fields(self) -> Dict[str, object]:
        return {"p": self._p}

    @property
    def p(self) -> float:
        return self._p

    @p.setter
    def p(self, value: float) -> None:
        "A new probability: written into the device block (no re-capture needed; not inside a capture)."
        self._p = _check_p(value)
        self._write(p=self._p)

    def state_dict(self) -> Dict[str, object]:
        return {**super().state_dict(), "p": self._p}

    def load_state_dict(self, state: Dict[str, object]) -> None:
        self.p = state["p"]
        super().load_state_dict(state)


class RandomHorizontalFlip(_ProbStream):
    """Flip each training image (and its boxes: x1' = W - x2, x2' = W - x1) with probability ``p``.  Install it as
    ``net.transform.hflip``; it acts only in training mode and only when targets are given.  Not an ``nn.Module``: it adds no key
    to the model's state dict.  ``seed``: the stream of decisions (``SimpleTrainer`` adds the rank under ``torch.distributed``)."""
    _layout = draw_state.HFLIP

    def __init__(self, p: float = 0.5, seed: int = 0):
        super().__init__(p, seed)
        self.flags: Optional[Tensor] = None           # the last batch's decisions (uint8 [B]; device or CPU)

    def __repr__(self) -> str:
        return f"RandomHorizontalFlip(p={self._p}, seed={self._seed})"

    # -- the decisions --------------------------------------------------------------------------------------------------
    @staticmethod
    def draw_flags(seed: int, counter: int, B: int, p: float) -> List[bool]:
        "Pure-Python restatement of ``rn_hflip_draw``: image b flips when u(seed, counter, b) < p (fp32 compare)."
        p32 = float(np.float32(p))
        return [hflip_u(int(seed) & _M64, int(counter), b) < p32 for b in range(int(B))]

    def draw(self, counter: int, B: int) -> List[bool]:
        "The decisions this object makes for a batch of B images at ``counter`` (no state change)."
        return self.draw_flags(self._seed, counter, B, self._p)

    def next_flags(self, B: int, device: torch.device) -> Tensor:
        """The next batch's decisions, uint8 [B] on ``device``, and the counter advanced by one.  CUDA: one ``rn_hflip_draw`` launch
        (capturable; the block is created at the first call, which must not be inside a capture); CPU: the Python restatement."""
        device = torch.device(device)
        if device.type != "cuda":
            if self._block is not None:
                raise RuntimeError("RandomHorizontalFlip: its state lives on the GPU; draw CPU batches from a fresh object")
            flags = torch.tensor(self._host_draw(lambda n: self.draw(n, B)), dtype=torch.uint8)
        else:
            flags = _ops().hflip_draw(self._device_block(device), B)
        self.flags = flags
        return flags


SHORT_SIDE_SALT = 0x5CA1E5CA1E5CA1E5      # xor-ed into the seed: a flip and a jitter that share a seed must not tie small sizes to flipped images


def short_side_hw(h: int, w: int, short: float, max_size: float) -> Tuple[int, int]:
    """The size ``GeneralizedRCNNTransform`` resizes an h x w image to for the short side ``short``: ``_scale_for`` and the two floors
    of ``resize``, in double and in their order of operations (``csrc/augment.hip`` does the same on the device)."""
    lo, hi = float(min(h, w)), float(max(h, w))
    scale = float(short) / lo
    if hi * scale > float(max_size):
        scale = float(max_size) / hi
    return int(math.floor(h * scale)), int(math.floor(w * scale))


class RandomShortSide(_DrawStream):
    """Resize each training image to a short side drawn from ``sizes`` (torchvision's ``min_size`` tuple), one draw per image and step,
    made on the device.  Install it as ``net.transform.scale_jitter``; it acts only in training mode and only when targets are given,
    and while it is installed the transform's own host-side draw from ``min_size`` is not consulted in training.  Not an
    ``nn.Module``: it adds no key to the model's state dict.  At most 16 sizes.  The padded canvas is sized for the largest entry
    the object was built with (``canvas_short``), whatever is drawn: one captured graph serves every scale, and small draws save
    no compute.  ``seed``: the stream of draws (``SimpleTrainer`` adds the rank under ``torch.distributed``)."""
    _layout = draw_state.SHORT_SIDE

    def __init__(self, sizes: Sequence[int], seed: int = 0):
        super().__init__(seed)
        self._sizes = self._check_sizes(sizes)
        self.canvas_short = max(self._sizes)          # the canvas bound: fixed for good (a captured step holds the canvas)
        self.sizes_drawn: Optional[Tensor] = None     # the last batch's sizes after the resize (int32 [B, 2]; device or CPU)
        self.ratios_drawn: Optional[Tensor] = None    # the last batch's box ratios (f32 [2B] = (rh, rw) per image; device or CPU)

    @staticmethod
    def _check_sizes(sizes) -> Tuple[int, ...]:
        sizes = tuple(sizes) if isinstance(sizes, (list, tuple)) else (sizes,)
        if not 1 <= len(sizes) <= SHORT_SIDE_MAX:
            raise ValueError(f"need 1..{SHORT_SIDE_MAX} short sides, got {len(sizes)}")
        if any(isinstance(v, bool) or int(v) != v or int(v) <= 0 for v in sizes):
            raise ValueError(f"short sides must be positive integers, got {sizes}")
        return tuple(int(v) for v in sizes)

    def _fields(self) -> Dict[str, object]:
        return {"sizes": self._sizes}

    def __repr__(self) -> str:
        return f"RandomShortSide(sizes={self._sizes}, seed={self._seed})"

    # -- the draws ------------------------------------------------------------------------------------------------------
    @staticmethod
    def draw_short_sides(seed: int, counter: int, B: int, sizes: Sequence[int]) -> List[int]:
        "Pure-Python restatement of the choice in ``rn_short_side_draw``: image b gets sizes[min(int(u * n), n - 1)]."
        n = len(sizes)
        salted = (int(seed) & _M64) ^ SHORT_SIDE_SALT
        # (u has 24 bits and n <= 16: u * n is exact in fp32, and so in double)
        return [int(sizes[min(int(hflip_u(salted, int(counter), b) * n), n - 1)]) for b in range(int(B))]

    def draw_short(self, counter: int, B: int) -> List[int]:
        "The short sides this object draws for a batch of B images at ``counter`` (no state change)."
        return self.draw_short_sides(self._seed, counter, B, self._sizes)

    def draw(self, counter: int, in_hw_list: Sequence[Tuple[int, int]], max_size: float) -> List[Tuple[int, int]]:
        """The sizes after the resize, (nh, nw) per image, this object draws at ``counter`` for images of sizes ``in_hw_list`` under the
        transform's ``max_size`` (no state change): the restatement of ``rn_short_side_draw``.  The box ratios that go with them are
        ``ratios(in_hw_list, sizes)``."""
        shorts = self.draw_short(counter, len(in_hw_list))
        return [short_side_hw(int(h), int(w), s, max_size) for (h, w), s in zip(in_hw_list, shorts)]

    @staticmethod
    def ratios(in_hw_list: Sequence[Tuple[int, int]], out_hw_list: Sequence[Tuple[int, int]]) -> List[Tuple[float, float]]:
        "The fp32 box ratios (rh, rw) per image: new / original, both rounded to fp32 first (``transform._ratios``)."
        return [(float(np.float32(nh) / np.float32(h)), float(np.float32(nw) / np.float32(w)))
                for (h, w), (nh, nw) in zip(in_hw_list, out_hw_list)]

    def bound(self, h: int, w: int, max_size: float) -> Tuple[int, int]:
        """An upper bound of every size a draw can give an h x w image: what ``canvas_short`` gives it, and -- the floor of a product
        one ulp below an integer can make a smaller short side give one pixel more -- never less than any current candidate does."""
        hw = [short_side_hw(h, w, s, max_size) for s in (self.canvas_short,) + self._sizes]
        return max(v[0] for v in hw), max(v[1] for v in hw)

    def next_sizes(self, in_hw_list: Sequence[Tuple[int, int]], max_size: float, device: torch.device) -> Tuple[Tensor, Tensor]:
        """The next batch's sizes (int32 [B, 2]) and box ratios (f32 [2B]) on ``device``, and the counter advanced by one.  CUDA: one
        ``rn_short_side_draw`` launch per 64 images (capturable; the block is created at the first call, which must not be inside a
        capture); CPU: the Python restatement."""
        device = torch.device(device)
        in_hw_list = [(int(h), int(w)) for h, w in in_hw_list]
        if device.type != "cuda":
            if self._block is not None:
                raise RuntimeError("RandomShortSide: its state lives on the GPU; draw CPU batches from a fresh object")
            hw = self._host_draw(lambda n: self.draw(n, in_hw_list, max_size))
            sizes = torch.tensor(hw, dtype=torch.int32).reshape(-1, 2)
            ratios = torch.tensor(self.ratios(in_hw_list, hw), dtype=torch.float32).reshape(-1)
        else:
            if int(max_size) != max_size:
                raise ValueError(f"the device draw takes an integer max_size, got {max_size}")
            sizes, ratios = _ops().short_side_draw(self._device_block(device), in_hw_list, int(max_size))
        self.sizes_drawn, self.ratios_drawn = sizes, ratios
        return sizes, ratios

    def next_sizes_dev(self, in_hw: Tensor, max_size: float) -> Tuple[Tensor, Tensor]:
        """``next_sizes`` for images whose sizes only the device holds (``in_hw`` int32 [B, 2] on a CUDA device, as ``ops.image_stage``
        writes it: the image capacity mode of ``graph.CapturedTrainStep``): one ``rn_resize_plan_dev`` launch for any B (capturable).
        The same stream of draws: at counter n it gives what ``draw(n, sizes, max_size)`` gives for the sizes ``in_hw`` holds, and
        the counter advances by one."""
        if int(max_size) != max_size:
            raise ValueError(f"the device draw takes an integer max_size, got {max_size}")
        if in_hw.device.type != "cuda":
            raise RuntimeError("RandomShortSide.next_sizes_dev: the sizes must be on the GPU (there is no CPU fallback)")
        sizes, ratios = _ops().resize_plan_dev(self._device_block(in_hw.device), in_hw, None, int(max_size))
        self.sizes_drawn, self.ratios_drawn = sizes, ratios
        return sizes, ratios

    # -- settings and state ---------------------------------------------------------------------------------------------
    @property
    def sizes(self) -> Tuple[int, ...]:
        return self._sizes

    @sizes.setter
    def sizes(self, value: Sequence[int]) -> None:
        """New candidates: written into the device block (no re-capture needed; not inside a capture).  None may exceed
        ``canvas_short``: the canvas -- part of every captured step -- would have to grow."""
        value = self._check_sizes(value)
        if max(value) > self.canvas_short:
            raise ValueError(f"short side {max(value)} exceeds {self.canvas_short}, the largest this object was built with: the padded "
                             "canvas would change; install a new RandomShortSide instead")
        self._sizes = value
        self._write(sizes=self._sizes)

    def state_dict(self) -> Dict[str, object]:
        return {**super().state_dict(), "sizes": list(self._sizes)}

    def load_state_dict(self, state: Dict[str, object]) -> None:
        self.sizes = state["sizes"]
        super().load_state_dict(state)


# ---- colour jitter -----------------------------------------------------------------------------------------------------
COLOR_SKIP = 0xF
COLOR_SALT_APPLY, COLOR_SALT_ORDER = 0xC0104A11C0104A11, 0x04DE404DE404DE45
COLOR_SALT_FACTOR = (0xB416B416B416B417, 0xC0274A57C0274A57, 0x5A7C5A7C5A7C5A7D, 0x40E040E040E040E1)
_PERMS = None


def color_order(idx: int, enabled_mask: int = 0xF) -> int:
    "The idx-th permutation of (0, 1, 2, 3) in lexicographic order as four nibbles (nibble k = the k-th operation; disabled -> 0xF)."
    global _PERMS
    if _PERMS is None:
        import itertools
        _PERMS = list(itertools.permutations(range(4)))
    return sum(((op if (enabled_mask >> op) & 1 else COLOR_SKIP) << (4 * k)) for k, op in enumerate(_PERMS[idx]))


def order_ops(order: int) -> List[int]:
    "The operation ids an ``order`` applies, in application order (the 0xF nibbles dropped)."
    return [(order >> (4 * k)) & 0xF for k in range(4) if (order >> (4 * k)) & 0xF != COLOR_SKIP]


def _gray(r: Tensor, g: Tensor, b: Tensor) -> Tensor:
    c = r.new_tensor([0.2989, 0.587, 0.114])
    return c[0] * r + c[1] * g + c[2] * b


def _blend(x: Tensor, other, f: Tensor) -> Tensor:
    return (f * x + (1.0 - f) * other).clamp(0.0, 1.0)


def _hue(img: Tensor, f: Tensor) -> Tensor:
    r, g, b = img.unbind(0)
    one, six = img.new_tensor(1.0), img.new_tensor(6.0)
    maxc, minc = img.max(0).values, img.min(0).values
    eq = maxc == minc
    cr = maxc - minc
    s = cr / torch.where(eq, one, maxc)
    d = torch.where(eq, one, cr)
    rc, gc, bc = (maxc - r) / d, (maxc - g) / d, (maxc - b) / d
    h0 = torch.where(maxc == r, bc - gc, torch.where(maxc == g, 2.0 + rc - bc, 4.0 + gc - rc))
    h = torch.fmod(h0 / six + 1.0, one)
    v = maxc
    h = h + f
    h = h - torch.floor(h)
    h6 = h * 6.0
    fl = torch.floor(h6)
    ff = h6 - fl
    i = torch.remainder(fl.to(torch.int32), 6)
    p = (v * (1.0 - s)).clamp(0.0, 1.0)
    q = (v * (1.0 - s * ff)).clamp(0.0, 1.0)
    t = (v * (1.0 - s * (1.0 - ff))).clamp(0.0, 1.0)

    def pick(c0, c1, c2, c3, c4, c5):
        return torch.where(i == 0, c0, torch.where(i == 1, c1, torch.where(i == 2, c2, torch.where(i == 3, c3, torch.where(i == 4, c4, c5)))))
    return torch.stack((pick(v, q, p, p, t, v), pick(t, v, v, q, p, p), pick(p, p, t, v, v, q)))


def color_mean_of(image: Tensor) -> float:
    "The contrast's mean: the gray values (fp32) of an fp32 ``[3, h, w]`` image summed in double, over h w, rounded to fp32."
    gray = _gray(*image.unbind(0))
    return float(np.float32(float(gray.to(torch.float64).sum()) / float(gray.numel())))


def apply_color_ops(image: Tensor, factors: Sequence[float], order: int, mean: Optional[float] = None) -> Tensor:
    """torchvision 0.8's tensor ColorJitter arithmetic on one fp32 RGB ``[3, h, w]`` image in [0, 1] (what the transform kernel runs per
    pixel, ``csrc/rn_color.hpp``): the operations of ``order`` with ``factors`` (indexed by operation id), every step one fp32 rounding.
    ``mean``: the contrast's mean gray when the caller has it, else computed here (``color_mean_of`` on the image as it is then)."""
    if image.dim() != 3 or image.shape[0] != 3 or image.dtype != torch.float32:
        raise ValueError(f"the colour jitter takes fp32 RGB [3, h, w] images in [0, 1], got {tuple(image.shape)} {image.dtype}")
    x = image
    for op in order_ops(order):
        f = x.new_tensor(float(factors[op]))
        if op == 0:
            x = (x * f).clamp(0.0, 1.0)
        elif op == 1:
            x = _blend(x, x.new_tensor(color_mean_of(x) if mean is None else float(mean)), f)
        elif op == 2:
            x = _blend(x, _gray(*x.unbind(0))[None], f)
        else:
            x = _hue(x, f)
    return x


class ColorJitter(_ProbStream):
    """torchvision's ``ColorJitter`` for fp32 RGB training images in [0, 1], drawn and applied on the device.  ``brightness`` /
    ``contrast`` / ``saturation``: a number v for factors in [max(0, 1 - v), 1 + v] or a pair (lo, hi); ``hue``: v for [-v, v] with
    0 <= v <= 0.5 or a pair inside [-0.5, 0.5]; 0 or None disables an operation.  With probability ``p`` an image is jittered: its
    enabled operations run in an order drawn from the 24 permutations, each with a factor drawn uniformly from its range.  Install it
    as ``net.transform.color_jitter``; it acts only in training mode and only when targets are given, on the raw image (before the
    normalisation, the resize and the flip).  Not an ``nn.Module``: it adds no key to the model's state dict.  ``seed``: the stream of
    draws (``SimpleTrainer`` adds the rank under ``torch.distributed``)."""
    _layout = draw_state.COLOR_JITTER

    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0, p: float = 1.0, seed: int = 0):
        self._ranges = [self._check_range(n, v) for n, v in zip(COLOR_OPS, (brightness, contrast, saturation, hue))]
        super().__init__(p, seed)
        self._built_mask = self.enabled_mask          # what the launches of a captured step were chosen for (fixed once a block exists)
        self.coef: Optional[Tensor] = None            # the last device batch's rn_color_coef rows (f32 [B, 8])
        self.drawn: Optional[List[Tuple[Tuple[float, ...], int]]] = None     # the last host-drawn batch's (factors, order)

    @staticmethod
    def _check_range(name: str, value) -> Optional[Tuple[float, float]]:
        "-> (lo, hi) as fp32 values, or None for a disabled operation (torchvision's ``_check_input``)."
        hue = name == "hue"
        if value is None:
            return None
        if isinstance(value, (list, tuple)):
            if len(value) != 2:
                raise ValueError(f"{name} must be a number or a pair (lo, hi), got {value!r}")
            lo, hi = float(value[0]), float(value[1])
        else:
            v = float(value)
            if v < 0:
                raise ValueError(f"{name} must not be negative, got {value!r}")
            lo, hi = (-v, v) if hue else (max(0.0, 1.0 - v), 1.0 + v)
        bound = (-0.5, 0.5) if hue else (0.0, float("inf"))
        if not bound[0] <= lo <= hi <= bound[1]:
            raise ValueError(f"{name} range ({lo}, {hi}) must be ordered and inside [{bound[0]}, {bound[1]}]")
        lo, hi = float(np.float32(lo)), float(np.float32(hi))
        centre = 0.0 if hue else 1.0
        return None if lo == hi == centre else (lo, hi)

    def __repr__(self) -> str:
        body = ", ".join(f"{n}={r}" for n, r in zip(COLOR_OPS, self._ranges))
        return f"ColorJitter({body}, p={self._p}, seed={self._seed})"

    # -- the draws ------------------------------------------------------------------------------------------------------
    @property
    def enabled_mask(self) -> int:
        return sum(1 << k for k, r in enumerate(self._ranges) if r is not None)

    def _lo_hi(self) -> Tuple[List[float], List[float]]:
        "The block's lo / hi: a disabled operation holds its identity factor twice."
        lo = [r[0] if r is not None else COLOR_IDENTITY[k] for k, r in enumerate(self._ranges)]
        hi = [r[1] if r is not None else COLOR_IDENTITY[k] for k, r in enumerate(self._ranges)]
        return lo, hi

    def _fields(self) -> Dict[str, object]:
        lo, hi = self._lo_hi()
        return {"p": self._p, "lo": lo, "hi": hi, "enabled_mask": self.enabled_mask}

    @staticmethod
    def draw_coefs(seed: int, counter: int, B: int, p: float, lo: Sequence[float], hi: Sequence[float],
                   enabled_mask: int) -> List[Tuple[Tuple[float, ...], int]]:
        """Pure-Python restatement of ``rn_color_jitter_draw``, bit for bit: per image (factors, order) -- the four factors as fp32
        values, ``order`` the four nibbles (0xFFFF when the p draw leaves the image alone)."""
        seed, counter, f32 = int(seed) & _M64, int(counter), np.float32
        p32 = f32(p)
        out = []
        for b in range(int(B)):
            applied = f32(hflip_u(seed ^ COLOR_SALT_APPLY, counter, b)) < p32
            idx = min(int(f32(hflip_u(seed ^ COLOR_SALT_ORDER, counter, b)) * f32(24.0)), 23)
            order = color_order(idx, enabled_mask) if applied else 0xFFFF
            fac = tuple(float(f32(lo[k]) + f32(hflip_u(seed ^ COLOR_SALT_FACTOR[k], counter, b)) * (f32(hi[k]) - f32(lo[k]))) for k in range(4))
            out.append((fac, order))
        return out

    def draw(self, counter: int, B: int) -> List[Tuple[Tuple[float, ...], int]]:
        "The (factors, order) this object draws for a batch of B images at ``counter`` (no state change)."
        lo, hi = self._lo_hi()
        return self.draw_coefs(self._seed, counter, B, self._p, lo, hi, self.enabled_mask)

    def next_draw(self, B: int) -> List[Tuple[Tuple[float, ...], int]]:
        """The next batch's (factors, order) on the HOST, and the counter advanced by one: what CPU tensors and images the fused
        transform does not take use (``apply_color_ops``).  With a device block the counter is read back and written (a
        synchronisation); not inside a capture."""
        self.drawn = self._host_draw(lambda n: self.draw(n, B))
        return self.drawn

    def next_coef(self, images) -> Tensor:
        """The next batch's ``rn_color_coef`` rows (f32 [B, 8]) on the images' device, and the counter advanced by one: one
        ``rn_color_jitter_draw`` launch and, when a contrast is enabled, ``rn_color_mean`` over the images (capturable; the block is
        created at the first call, which must not be inside a capture).  ``images``: CUDA f32 ``[3, h, w]`` tensors or
        ``ops.StagedImages``."""
        ops = _ops()
        staged = isinstance(images, ops.StagedImages)
        device, B = (images.device, images.B) if staged else (images[0].device, len(images))
        if device.type != "cuda":
            raise RuntimeError("ColorJitter.next_coef draws on the GPU; CPU batches use next_draw()")
        if self._block is None:
            self._built_mask = self.enabled_mask
        coef = ops.color_jitter_draw(self._device_block(device), B)
        if self._built_mask & 2:                       # (a contrast that was never enabled launches nothing)
            ops.color_mean(images, coef)
        self.coef = coef
        return coef

    # -- settings and state ---------------------------------------------------------------------------------------------
    def _range(self, k: int) -> Optional[Tuple[float, float]]:
        return self._ranges[k]

    def _set_range(self, k: int, value) -> None:
        """A new range: written into the device block (no re-capture needed; not inside a capture).  Enabling an operation the object
        was built without changes which kernels a step launches, so it is refused once the block exists."""
        r = self._check_range(COLOR_OPS[k], value)
        if self._block is not None and r is not None and not (self._built_mask >> k) & 1:
            raise ValueError(f"ColorJitter: {COLOR_OPS[k]} was disabled when this object's device state was created; enabling it changes "
                             "which kernels a (captured) step launches -- install a new ColorJitter instead")
        self._ranges[k] = r
        lo, hi = self._lo_hi()
        self._write(lo=lo, hi=hi, enabled_mask=self.enabled_mask)

    brightness = property(lambda self: self._range(0), lambda self, v: self._set_range(0, v))
    contrast = property(lambda self: self._range(1), lambda self, v: self._set_range(1, v))
    saturation = property(lambda self: self._range(2), lambda self, v: self._set_range(2, v))
    hue = property(lambda self: self._range(3), lambda self, v: self._set_range(3, v))

    def state_dict(self) -> Dict[str, object]:
        state = super().state_dict()
        state.update({n: (None if r is None else list(r)) for n, r in zip(COLOR_OPS, self._ranges)})
        return state

    def load_state_dict(self, state: Dict[str, object]) -> None:
        for k, n in enumerate(COLOR_OPS):
            self._set_range(k, state[n])
        super().load_state_dict(state)


# ---- brightness / contrast ------------------------------------------------------------------------------------------------
BC_SALT_APPLY, BC_SALT_CONTRAST, BC_SALT_BRIGHTNESS = 0xB7C0A991B7C0A991, 0xC0A7C0A7C0A7C0A7, 0xB419B419B419B419
COLOR_BC_PRESENT, COLOR_BC_PENDING = 1 << 16, 1 << 17      # bits of rn_color_coef.order above the four nibbles


def image_mean_of(image: Tensor) -> float:
    "Step 3's mean: all values of an fp32 ``[3, h, w]`` image summed in double, over 3 h w, rounded to fp32."
    return float(np.float32(float(image.to(torch.float64).sum()) / float(image.numel())))


def apply_brightness_contrast(image: Tensor, alpha: float, beta: float, ref: Optional[float] = None) -> Tensor:
    """Steps 3-5 of the rule of ``rn_brightness_contrast_draw`` (``include/retinanet_hip.h``) on one fp32 RGB ``[3, h, w]`` image in
    [0, 1], in torch: ``clamp(alpha * x + beta * ref, 0, 1)``, one fp32 rounding per operation.  ``ref``: 1 for ``brightness_by_max``,
    the image mean when the caller has it, or None to compute it here (``image_mean_of``)."""
    if image.dim() != 3 or image.shape[0] != 3 or image.dtype != torch.float32:
        raise ValueError(f"brightness / contrast takes fp32 RGB [3, h, w] images in [0, 1], got {tuple(image.shape)} {image.dtype}")
    ref = image_mean_of(image) if ref is None else float(ref)
    add = np.float32(beta) * np.float32(ref)
    return (image.new_tensor(float(np.float32(alpha))) * image + image.new_tensor(float(add))).clamp(0.0, 1.0)


def _bc_limit(v, name: str) -> Tuple[float, float]:
    "``_limit`` with every given number checked first: min / max would hide a NaN in a pair."
    for x in (v if isinstance(v, (list, tuple)) else (v,)):
        if isinstance(x, bool) or not math.isfinite(float(x)):
            raise ValueError(f"{name} must be finite numbers, got {v!r}")
    return _limit(v, name)


class RandomBrightnessContrast(_ProbStream):
    """albumentations' ``RandomBrightnessContrast`` for fp32 RGB training images in [0, 1], drawn and applied on the device, with
    albumentations' argument meanings and defaults: a scalar limit v is the range (-v, v), a pair is taken as given.  With probability
    ``p`` an image becomes ``clamp(alpha * x + beta * ref, 0, 1)`` with ``alpha`` drawn from ``1 + contrast_limit``, ``beta`` from
    ``brightness_limit`` and ``ref`` = 1 (``brightness_by_max``: the value range) or the mean of all of the image's values.  The
    numbered rule of ``rn_brightness_contrast_draw`` in ``include/retinanet_hip.h`` is the definition; ``draw_coefs`` and
    ``apply_brightness_contrast`` restate it.  The deviation from albumentations: there the reference's uint8 images go through a
    256-entry LUT and the result is truncated to uint8; here the arithmetic is fp32 on [0, 1] with the LUT's clip and without its
    quantisation -- the same intent, not the same bits.  ``ColorJitter`` does not cover this transform: torchvision's brightness is a
    pure multiply and its contrast blends towards the mean gray.

    Install it as ``net.transform.brightness_contrast``; it acts only in training mode and only when targets are given, on the raw image
    after the crop, the warp and the colour jitter's operations and before the normalisation, the resize and the flip.  On the fused
    paths the coefficients ride in the colour jitter's ``rn_color_coef`` rows (``rn_brightness_contrast_draw``; with
    ``brightness_by_max=False`` one more pass over the images, ``rn_brightness_contrast_mean``) and the transform kernel applies them
    to every source pixel it reads -- inside the captured step, each replay a new draw.  ``p`` and the limits can be rewritten between
    replays; ``brightness_by_max`` decides which kernels a step launches and is fixed once the device block exists.  Not an
    ``nn.Module``: it adds no key to the model's state dict.  ``seed``: the stream of draws (``SimpleTrainer`` adds the rank under
    ``torch.distributed``)."""
    _layout = draw_state.BRIGHTNESS_CONTRAST

    def __init__(self, brightness_limit=0.2, contrast_limit=0.2, brightness_by_max: bool = True, p: float = 0.5, seed: int = 0):
        super().__init__(p, seed)
        self._brightness, self._contrast = _bc_limit(brightness_limit, "brightness_limit"), _bc_limit(contrast_limit, "contrast_limit")
        self._by_max = bool(brightness_by_max)
        self.coef: Optional[Tensor] = None            # the last device batch's rn_color_coef rows (f32 [B, 8])
        self.drawn: Optional[List[Tuple[bool, float, float]]] = None      # the last host-drawn batch's (applied, alpha, beta)

    def __repr__(self) -> str:
        return (f"RandomBrightnessContrast(brightness_limit={self._brightness}, contrast_limit={self._contrast}, "
                f"brightness_by_max={self._by_max}, p={self._p}, seed={self._seed})")

    def _fields(self) -> Dict[str, object]:
        return {"p": self._p, "brightness": self._brightness, "contrast": self._contrast, "by_max": self._by_max}

    # -- the draws ------------------------------------------------------------------------------------------------------
    @staticmethod
    def draw_coefs(seed: int, counter: int, B: int, p: float, brightness: Sequence[float], contrast: Sequence[float]) -> List[Tuple[bool, float, float]]:
        """Pure-Python restatement of steps 1 and 2 of ``rn_brightness_contrast_draw``, bit for bit: per image (applied, alpha, beta),
        the two as fp32 values, drawn whatever ``applied`` is.  ``brightness`` / ``contrast``: (lo, hi) of beta and of alpha - 1."""
        seed, counter, f32 = int(seed) & _M64, int(counter), np.float32
        p32, (blo, bhi), (clo, chi) = f32(p), (f32(v) for v in brightness), (f32(v) for v in contrast)
        out = []
        for b in range(int(B)):
            applied = bool(f32(hflip_u(seed ^ BC_SALT_APPLY, counter, b)) < p32)
            alpha = f32(1.0) + (clo + f32(hflip_u(seed ^ BC_SALT_CONTRAST, counter, b)) * (chi - clo))
            beta = blo + f32(hflip_u(seed ^ BC_SALT_BRIGHTNESS, counter, b)) * (bhi - blo)
            out.append((applied, float(alpha), float(beta)))
        return out

    def draw(self, counter: int, B: int) -> List[Tuple[bool, float, float]]:
        "The (applied, alpha, beta) this object draws for a batch of B images at ``counter`` (no state change)."
        return self.draw_coefs(self._seed, counter, B, self._p, self._brightness, self._contrast)

    def next_draw(self, B: int) -> List[Tuple[bool, float, float]]:
        """The next batch's (applied, alpha, beta) on the HOST, and the counter advanced by one: what CPU tensors and images the fused
        transform does not take use (``apply_brightness_contrast``).  With a device block the counter is read back and written (a
        synchronisation); not inside a capture."""
        self.drawn = self._host_draw(lambda n: self.draw(n, B))
        return self.drawn

    def next_coef(self, images, coef: Optional[Tensor] = None) -> Tensor:
        """The next batch's ``rn_color_coef`` rows (f32 [B, 8]) on the images' device, and the counter advanced by one: one
        ``rn_brightness_contrast_draw`` launch into ``coef`` -- the rows a ``ColorJitter.next_coef`` returned, contrast mean included
        -- or into fresh identity rows, and with ``brightness_by_max=False`` ``rn_brightness_contrast_mean`` over the images
        (capturable; the block is created at the first call, which must not be inside a capture).  ``images``: CUDA f32 ``[3, h, w]``
        tensors or ``ops.StagedImages``."""
        ops = _ops()
        staged = isinstance(images, ops.StagedImages)
        device, B = (images.device, images.B) if staged else (images[0].device, len(images))
        if device.type != "cuda":
            raise RuntimeError("RandomBrightnessContrast.next_coef draws on the GPU; CPU batches use next_draw()")
        coef = ops.brightness_contrast_draw(self._device_block(device), B, coef)
        if not self._by_max:                           # (by-max launches nothing more: ref = 1)
            ops.brightness_contrast_mean(images, coef)
        self.coef = coef
        return coef

    # -- settings and state ---------------------------------------------------------------------------------------------
    @property
    def brightness_limit(self) -> Tuple[float, float]:
        return self._brightness

    @property
    def contrast_limit(self) -> Tuple[float, float]:
        return self._contrast

    @property
    def brightness_by_max(self) -> bool:
        return self._by_max

    @brightness_by_max.setter
    def brightness_by_max(self, value: bool) -> None:
        "Which kernels a step launches depends on it, so a change is refused once the device block exists."
        value = bool(value)
        if self._block is not None and value != self._by_max:
            raise ValueError(f"RandomBrightnessContrast: brightness_by_max was {self._by_max} when this object's device state was created; "
                             "changing it changes which kernels a (captured) step launches -- install a new RandomBrightnessContrast instead")
        self._by_max = value

    def set_limits(self, brightness_limit=None, contrast_limit=None) -> None:
        "New ranges (the ones not given stay): written into the device block (no re-capture needed; not inside a capture)."
        if brightness_limit is not None:
            self._brightness = _bc_limit(brightness_limit, "brightness_limit")
        if contrast_limit is not None:
            self._contrast = _bc_limit(contrast_limit, "contrast_limit")
        self._write(brightness=self._brightness, contrast=self._contrast)

    def state_dict(self) -> Dict[str, object]:
        return {**super().state_dict(), "brightness_limit": list(self._brightness), "contrast_limit": list(self._contrast),
                "brightness_by_max": self._by_max}

    def load_state_dict(self, state: Dict[str, object]) -> None:
        self.brightness_by_max = state["brightness_by_max"]
        self.set_limits(tuple(state["brightness_limit"]), tuple(state["contrast_limit"]))
        super().load_state_dict(state)


# ---- bbox-safe random crop ------------------------------------------------------------------------------------------------
CROP_SALT_APPLY =0xC409C409C409C40B                                 # include/retinanet_hip.h: rn_bbox_crop_draw, step 1
CROP_SALT_LEFT, CROP_SALT_TOP, CROP_SALT_RIGHT, CROP_SALT_BOTTOM = 0x1EF71EF71EF71EF7, 0x70B070B070B070B1, 0x4167416741674169, 0xB077B077B077B079
_I32_MIN, _I32_MAX = -2 ** 31, 2 ** 31 - 1


def _sat_int(f) -> int:
    "int(f) for a finite fp32 value, saturating at the int32 range (the kernel's conversion)."
    f = float(f)
    return _I32_MIN if f <= -2147483648.0 else (_I32_MAX if f >= 2147483648.0 else int(f))


def _clamp(v: int, lo: int, hi: int) -> int:
    return lo if v < lo else (hi if v > hi else v)


def _crop_axis(u_lo: float, u_hi: float, u1: int, u2: int, n: int) -> Tuple[int, int]:
    "(start, end) of the crop on one axis of length n around the union [u1, u2): fp32 multiplies, truncation (step 4)."
    f32 = np.float32
    a, c = int(f32(u_lo) * f32(u1 + 1)), int(f32(u_hi) * f32(n - u2 + 1))
    return min(a, u1), u2 + min(c, n - u2)


class BBoxSafeRandomCrop(_ProbStream):
    """With probability ``p`` crop each training image to a random window that contains all of its boxes, and shift the boxes with it:
    albumentations' ``BBoxSafeRandomCrop`` with ``erosion_rate = 0`` in intent -- each margin is drawn uniformly between the image edge
    and the union of the boxes -- on integer pixels.  No box that lies inside the image is ever cut and none is dropped, so the GT
    counts do not change.  It is NOT bit-compatible with albumentations' float rounding; ``draw_rects`` is the definition (the numbered
    rule of ``rn_bbox_crop_draw`` in ``include/retinanet_hip.h``).  The crop keeps the orientation (a landscape image stays landscape:
    the short axis of the window is widened if need be), so a batch stays inside its canvas class.  An image without boxes, with a
    non-finite box or of size 0 is left alone.

    Install it as ``net.transform.crop``; it acts only in training mode and only when targets are given, before the flip, the colour
    jitter and the resize.  On staged images with packed GT (``graph.CapturedTrainStep(image_capacity=..., gt_capacity=...)``) the
    rectangles are drawn on the device from the boxes (``rn_bbox_crop_draw``) and each window is copied into a second arena
    (``rn_image_crop_stage``), inside the captured step, each replay a new draw; ``CapturedTrainStep`` needs ``image_capacity`` for it.
    Every other input (CPU tensors, CUDA lists) takes the same stream of rectangles from ``draw_rects`` on the HOST: the boxes and the
    counter are read back, which on CUDA is one synchronisation per step.  Not an ``nn.Module``: it adds no key to the model's state
    dict.  ``seed``: the stream of draws (``SimpleTrainer`` adds the rank under ``torch.distributed``)."""
    _layout = draw_state.BBOX_CROP

    def __init__(self, p: float = 1.0, seed: int = 0):
        super().__init__(p, seed)
        self.rect: Optional[Tensor] = None            # the last device batch's rectangles (int32 [B, 4] = (y0, x0, ch, cw))
        self.rects: Optional[List[Tuple[int, int, int, int]]] = None      # the last host-drawn batch's rectangles

    def __repr__(self) -> str:
        return f"BBoxSafeRandomCrop(p={self._p}, seed={self._seed})"

    # -- the draws ------------------------------------------------------------------------------------------------------
    @staticmethod
    def draw_rects(seed: int, counter: int, in_hw: Sequence[Tuple[int, int]], boxes_per_image, p: float) -> List[Tuple[int, int, int, int]]:
        """Pure-Python restatement of ``rn_bbox_crop_draw``, exactly: per image the rectangle (y0, x0, ch, cw).  ``boxes_per_image[b]``:
        image b's boxes, anything ``numpy.asarray`` turns into fp32 [T, 4] = (x1, y1, x2, y2) (a CPU tensor, an array, a list; None or
        empty for no boxes)."""
        seed, counter, f32 = int(seed) & _M64, int(counter), np.float32
        p32 = f32(p)
        out = []
        for b, (h, w) in enumerate(in_hw):
            h, w = int(h), int(w)
            if h < 1 or w < 1:
                out.append((0, 0, 0, 0))
                continue
            bx = boxes_per_image[b]
            bx = np.zeros((0, 4), f32) if bx is None else np.asarray(bx, dtype=f32).reshape(-1, 4)
            identity = (0, 0, h, w)
            if bx.shape[0] == 0 or not f32(hflip_u(seed ^ CROP_SALT_APPLY, counter, b)) < p32:
                out.append(identity)
                continue
            # (numpy's min / max propagate a NaN, as the kernel's flag does)
            ext = (bx[:, 0].min(), bx[:, 1].min(), bx[:, 2].max(), bx[:, 3].max())
            if not all(np.isfinite(v) for v in ext):
                out.append(identity)
                continue
            ux1, uy1 = _clamp(_sat_int(np.floor(ext[0])), 0, w - 1), _clamp(_sat_int(np.floor(ext[1])), 0, h - 1)
            ux2, uy2 = _clamp(_sat_int(np.ceil(ext[2])), ux1 + 1, w), _clamp(_sat_int(np.ceil(ext[3])), uy1 + 1, h)
            x0, xe = _crop_axis(hflip_u(seed ^ CROP_SALT_LEFT, counter, b), hflip_u(seed ^ CROP_SALT_RIGHT, counter, b), ux1, ux2, w)
            y0, ye = _crop_axis(hflip_u(seed ^ CROP_SALT_TOP, counter, b), hflip_u(seed ^ CROP_SALT_BOTTOM, counter, b), uy1, uy2, h)
            cw, ch = xe - x0, ye - y0
            if h <= w and ch > cw:
                x0, cw = max(0, min(x0 - (ch - cw) // 2, w - ch)), ch
            elif h > w and cw > ch:
                y0, ch = max(0, min(y0 - (cw - ch) // 2, h - cw)), cw
            out.append((y0, x0, ch, cw))
        return out

    def draw(self, counter: int, in_hw: Sequence[Tuple[int, int]], boxes_per_image) -> List[Tuple[int, int, int, int]]:
        "The rectangles this object draws at ``counter`` for images of sizes ``in_hw`` with these boxes (no state change)."
        return self.draw_rects(self._seed, counter, in_hw, boxes_per_image, self._p)

    @staticmethod
    def bound(h: int, w: int, short: int, max_size: int) -> Tuple[int, int]:
        """An upper bound of the size after the resize of every crop of an h x w image: the crop keeps the orientation, so its short
        side becomes at most ``short`` -- the largest short side that can be drawn -- and its long side at most ``max_size``."""
        return (int(short), int(max_size)) if int(h) <= int(w) else (int(max_size), int(short))

    def next_rects(self, in_hw: Sequence[Tuple[int, int]], boxes_per_image) -> List[Tuple[int, int, int, int]]:
        """The next batch's rectangles on the HOST, and the counter advanced by one: what CPU tensors and CUDA lists use.  The boxes
        are read on the host (CUDA tensors are copied back: a synchronisation) and, with a device block, so is the counter; not
        inside a capture."""
        boxes = [None if b is None else (b.detach().cpu().numpy() if isinstance(b, Tensor) else b) for b in boxes_per_image]
        self.rects = self._host_draw(lambda n: self.draw(n, in_hw, boxes))
        return self.rects

    def device_block(self, device: torch.device) -> Tensor:
        """The ``rn_bbox_crop_state`` block on ``device`` that ``ops.bbox_crop_staged`` draws from, created at the first call (which
        must not be inside a capture) and kept for good: a captured step holds its address."""
        if torch.device(device).type != "cuda":
            raise RuntimeError("BBoxSafeRandomCrop: the device draw runs on the GPU; CPU batches use next_rects()")
        return self._device_block(device)


def _entries(entries) -> Iterator[Tuple[str, dict]]:
    "(class name, params) of every entry of an hparams ``transforms`` list: a dict with ``class_name`` / ``params``, or a bare name."
    for e in entries or []:
        yield (str(e.get("class_name", "")), dict(e.get("params") or {})) if isinstance(e, dict) else (str(e), {})


def _named(entries, names: Sequence[str], what: str, log) -> Iterator[Tuple[str, dict]]:
    "The first entry whose class name is one of ``names``; every further one is skipped with a warning."
    seen = False
    for name, params in _entries(entries):
        if name not in names:
            continue
        if seen:
            log.warning("transforms: a second %s (%s) is skipped", what, name)
            continue
        seen = True
        yield name, params


def _entry_p(params: dict, default: float) -> float:
    "An entry's probability: ``always_apply: true`` means 1."
    return 1.0 if params.get("always_apply") else float(params.get("p", default))


def _as_limit(v):
    "An entry's limit as the classes take it: YAML's list as a tuple (a range), a scalar as it is."
    return tuple(v) if isinstance(v, (list, tuple)) else v


_BBOX_CROP_NAMES = ("albumentations.BBoxSafeRandomCrop", "BBoxSafeRandomCrop")


def bbox_crop_from_transforms(entries, seed: int = 0, log=None) -> Optional[BBoxSafeRandomCrop]:
    """The bbox-safe random crop an hparams ``transforms`` list asks for, or None.  ``albumentations.BBoxSafeRandomCrop`` (``p``
    defaults to 1.0, albumentations' own default; ``always_apply: true`` means p = 1) maps onto ``BBoxSafeRandomCrop``, which works on
    integer pixels and is not bit-compatible with albumentations.  A non-zero ``erosion_rate`` is warned about and treated as 0.
    ``RandomSizedBBoxSafeCrop`` and every other crop are not this one: ``from_transforms`` skips them with its warning."""
    log = log or logging.getLogger(__name__)
    found = None
    for name, params in _named(entries, _BBOX_CROP_NAMES, "bbox-safe crop", log):
        if float(params.get("erosion_rate", 0.0) or 0.0) != 0.0:
            log.warning("transforms: %s erosion_rate=%s is not implemented and is treated as 0 (the crop never cuts into the union of "
                        "the boxes)", name, params.get("erosion_rate"))
        found = BBoxSafeRandomCrop(p=_entry_p(params, 1.0), seed=seed)
    return found


# ---- shift / scale / rotate -----------------------------------------------------------------------------------------------
AFFINE_SALT_APPLY = 0xA551A551A551A551                               # include/retinanet_hip.h: rn_affine_draw, step 1
AFFINE_SALT_ANGLE, AFFINE_SALT_SCALE, AFFINE_SALT_DX, AFFINE_SALT_DY = 0xA4613A4613A46135, 0x5CA7E5CA7E5CA7E5, 0xD0C5D0C5D0C5D0C5, 0xD1E7D1E7D1E7D1E7
AFFINE_MIN_DET = 1e-12                                               # step 2: below it the image is left alone
_IDENTITY6 = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def _limit(v, name: str, bias: float = 0.0) -> Tuple[float, float]:
    "albumentations' to_tuple: a scalar v is the range (-v, v), a pair is taken as given; ``bias`` is added to both ends; fp32 values."
    if isinstance(v, (list, tuple)):
        if len(v) != 2:
            raise ValueError(f"{name} must be a number or a pair, got {v!r}")
        lo, hi = float(v[0]), float(v[1])
    else:
        lo, hi = -float(v), float(v)
    lo, hi = float(np.float32(min(lo, hi) + bias)), float(np.float32(max(lo, hi) + bias))
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError(f"{name} must be finite, got {v!r}")
    return lo, hi


class AffineCoefs:
    """What ``rn_affine_draw`` writes per image, on the host: ``m`` and ``inv`` fp32 numpy [B, 6] (the forward matrix
    (m00, m01, m02, m10, m11, m12) and its inverse), ``applied`` a list of bools."""
    __slots__ = ("m", "inv", "applied")

    def __init__(self, m, inv, applied):
        self.m, self.inv = np.asarray(m, dtype=np.float32).reshape(-1, 6), np.asarray(inv, dtype=np.float32).reshape(-1, 6)
        self.applied = [bool(a) for a in applied]

    @classmethod
    def from_device(cls, coef: Tensor) -> "AffineCoefs":
        "From an ``rn_affine_coef`` tensor (``ops.affine_draw``, ``ShiftScaleRotate.coef``): one device->host copy."
        raw = coef.detach().cpu().contiguous().numpy()
        return cls(raw[:, 0:6].copy().view(np.float32), raw[:, 6:12].copy().view(np.float32), raw[:, 12] != 0)


def _boxes_f32(bx) -> np.ndarray:
    if bx is None:
        return np.zeros((0, 4), np.float32)
    if isinstance(bx, Tensor):
        bx = bx.detach().cpu().numpy()
    return np.asarray(bx, dtype=np.float32).reshape(-1, 4)


def _warp_rows(m, h: int, w: int, min_visibility, bx: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    "Step 3 of ``rn_affine_draw`` on fp32 rows [T, 4] -> (the clamped boxes [T, 4], keep bool [T]); numpy fp32, one rounding per operation."
    f32 = np.float32
    m = [f32(v) for v in m]
    xs, ys = (bx[:, 0], bx[:, 2], bx[:, 2], bx[:, 0]), (bx[:, 1], bx[:, 1], bx[:, 3], bx[:, 3])
    with np.errstate(all="ignore"):
        X = [(m[0] * x + m[1] * y) + m[2] for x, y in zip(xs, ys)]
        Y = [(m[3] * x + m[4] * y) + m[5] for x, y in zip(xs, ys)]
        finite = np.ones(bx.shape[0], bool)
        for v in X + Y:
            finite &= np.isfinite(v)

        def fold(vals, better):                                        # min(p, q) = q < p ? q : p (max: >), folded from the left
            acc = vals[0]
            for q in vals[1:]:
                acc = np.where(better(q, acc), q, acc)
            return acc

        X1, X2, Y1, Y2 = fold(X, np.less), fold(X, np.greater), fold(Y, np.less), fold(Y, np.greater)
        clamp = lambda v, top: np.where(v < f32(0), f32(0), np.where(v > f32(top), f32(top), v)).astype(f32)
        out = np.stack([clamp(X1, w), clamp(Y1, h), clamp(X2, w), clamp(Y2, h)], 1).astype(f32)
        au = (X2 - X1) * (Y2 - Y1)
        cw, ch = out[:, 2] - out[:, 0], out[:, 3] - out[:, 1]
        keep = finite & (cw > 0) & (ch > 0) & (cw * ch >= f32(min_visibility) * au)
    return out, keep


class ShiftScaleRotate(_ProbStream):
    """With probability ``p`` move each training image by a random shift, scale and rotation about its centre (bilinear
    interpolation, reflect-101 border) and take its boxes along: albumentations' ``ShiftScaleRotate`` in intent, with its argument
    meanings and defaults -- a scalar limit v is the range (-v, v), a pair is taken as given; the angle is in degrees, the scale is drawn
    from ``1 + scale_limit`` (which must stay > 0: ``ValueError``) and the two shifts, fractions of the width and the height, both from
    ``shift_limit``.  A box becomes the bounding box of its four moved corners, clipped to the image; it is dropped when nothing of it
    is left or when less than ``min_visibility`` of its area is.  It is NOT bit-compatible with albumentations (OpenCV's ``warpAffine``
    uses fixed-point weights, albumentations' box code depends on its version): ``draw_coefs``, ``warp_boxes`` and ``warp_image``
    restate the numbered rule of ``rn_affine_draw`` / ``rn_image_warp_stage`` in ``include/retinanet_hip.h``, and that rule is the
    definition.  One deviation is stated there: an image whose boxes would ALL be dropped is left alone, so no image loses all of
    its GT.  Other interpolations and border modes are not implemented.

    Install it as ``net.transform.shift_scale_rotate``; it acts only in training mode and only when targets are given, after the crop
    and before the flip, the colour jitter and the resize.  On staged images with packed GT
    (``graph.CapturedTrainStep(image_capacity=..., gt_capacity=...)``) the matrices are drawn on the device (``rn_affine_draw``, which
    also packs the surviving rows), and each image is warped into a second arena (``rn_image_warp_stage``), inside the captured step,
    each replay a new draw.  Every other input (CPU tensors, CUDA lists) takes the same stream of draws from the restatement on the
    HOST: the boxes and the counter are read back, which on CUDA is one synchronisation per step; double-precision ``sin`` / ``cos``
    may differ between host and device in the last bit, so the two paths agree to an fp32 step of a matrix entry, not always bit
    for bit.  Not an ``nn.Module``: it adds no key to the model's state dict.  ``seed``: the stream of draws (``SimpleTrainer`` adds
    the rank under ``torch.distributed``)."""
    _layout = draw_state.AFFINE

    def __init__(self, shift_limit=0.0625, scale_limit=0.1, rotate_limit=45, p: float = 0.5, min_visibility: float = 0.0, seed: int = 0):
        super().__init__(p, seed)
        self._set_ranges(shift_limit, scale_limit, rotate_limit, min_visibility)
        self.coef: Optional[Tensor] = None            # the last device batch's rn_affine_coef (int32 [B, 16]; AffineCoefs.from_device)
        self.coefs: Optional[AffineCoefs] = None      # the last host-drawn batch's coefficients

    def _set_ranges(self, shift_limit, scale_limit, rotate_limit, min_visibility) -> None:
        shift, scale, angle = _limit(shift_limit, "shift_limit"), _limit(scale_limit, "scale_limit", 1.0), _limit(rotate_limit, "rotate_limit")
        if not scale[0] > 0.0:
            raise ValueError(f"1 + scale_limit must stay > 0, got the scale range {scale}")
        mv = float(min_visibility)
        if not 0.0 <= mv <= 1.0:
            raise ValueError(f"min_visibility must be in [0, 1], got {min_visibility}")
        self.shift_limit, self.scale_range, self.rotate_limit, self.min_visibility = shift, scale, angle, float(np.float32(mv))

    @property
    def ranges(self) -> Tuple[Tuple[float, ...], Tuple[float, ...]]:
        "(lo, hi) of (angle, scale, dx, dy): what the device block holds."
        r = (self.rotate_limit, self.scale_range, self.shift_limit, self.shift_limit)
        return tuple(v[0] for v in r), tuple(v[1] for v in r)

    def _fields(self) -> Dict[str, object]:
        lo, hi = self.ranges
        return {"p": self._p, "min_visibility": self.min_visibility, "lo": lo, "hi": hi}

    def __repr__(self) -> str:
        return (f"ShiftScaleRotate(shift_limit={self.shift_limit}, scale_limit={tuple(float(np.float32(v - 1.0)) for v in self.scale_range)}, "
                f"rotate_limit={self.rotate_limit}, p={self._p}, min_visibility={self.min_visibility}, seed={self._seed})")

    # -- the restatement ------------------------------------------------------------------------------------------------
    @staticmethod
    def draw_coefs(seed: int, counter: int, in_hw: Sequence[Tuple[int, int]], boxes_per_image, p: float, lo: Sequence[float],
                   hi: Sequence[float], min_visibility: float = 0.0) -> AffineCoefs:
        """Restatement of ``rn_affine_draw``'s steps 1 and 2 (and the all-dropped rule of step 3): the draws in fp32, the matrices in
        float64 numpy rounded to fp32 once.  ``lo`` / ``hi``: the ranges of (angle, scale, dx, dy).  ``boxes_per_image[b]``: image b's
        boxes, anything ``numpy.asarray`` turns into fp32 [T, 4] (None or empty for no boxes)."""
        seed, counter, f32, f64 = int(seed) & _M64, int(counter), np.float32, np.float64
        p32 = f32(p)
        ms, invs, flags = [], [], []
        for b, (h, w) in enumerate(in_hw):
            h, w = int(h), int(w)
            applied = f32(hflip_u(seed ^ AFFINE_SALT_APPLY, counter, b)) < p32
            angle, scale, dx, dy = (f32(lo[k]) + f32(hflip_u(seed ^ salt, counter, b)) * (f32(hi[k]) - f32(lo[k]))
                                    for k, salt in enumerate((AFFINE_SALT_ANGLE, AFFINE_SALT_SCALE, AFFINE_SALT_DX, AFFINE_SALT_DY)))
            with np.errstate(all="ignore"):
                t = f64(angle) * f64(np.pi) / f64(180.0)
                ca, sb = f64(scale) * np.cos(t), f64(scale) * np.sin(t)
                cx, cy = (f64(w) - 1.0) / 2.0, (f64(h) - 1.0) / 2.0
                tx, ty = ((1.0 - ca) * cx - sb * cy) + f64(dx) * f64(w), (sb * cx + (1.0 - ca) * cy) + f64(dy) * f64(h)
                det = ca * ca + sb * sb
                i00, i01, i10, i11 = ca / det, -sb / det, sb / det, ca / det
                m = np.array([ca, sb, tx, -sb, ca, ty], f64).astype(f32)
                inv = np.array([i00, i01, -(i00 * tx + i01 * ty), i10, i11, -(i10 * tx + i11 * ty)], f64).astype(f32)
            ok = bool(applied) and h >= 1 and w >= 1 and bool(det >= AFFINE_MIN_DET) and bool(np.isfinite(m).all() and np.isfinite(inv).all())
            if ok:
                bx = _boxes_f32(boxes_per_image[b] if boxes_per_image is not None else None)
                if bx.shape[0] > 0 and not _warp_rows(m, h, w, min_visibility, bx)[1].any():
                    ok = False                                         # (no image loses all of its GT)
            if not ok:
                m, inv = np.array(_IDENTITY6, f32), np.array(_IDENTITY6, f32)
            ms.append(m), invs.append(inv), flags.append(ok)
        return AffineCoefs(np.stack(ms) if ms else np.zeros((0, 6), f32), np.stack(invs) if invs else np.zeros((0, 6), f32), flags)

    @staticmethod
    def warp_boxes(coefs: AffineCoefs, in_hw: Sequence[Tuple[int, int]], boxes_per_image, labels_per_image=None,
                   min_visibility: float = 0.0):
        """Restatement of steps 3 and 4 for given coefficients: per image (boxes fp32 tensor [T', 4], labels tensor [T'] or None) --
        the kept rows in order, moved and clipped; an image with ``applied`` false keeps its rows bit for bit."""
        out = []
        for b, (h, w) in enumerate(in_hw):
            bx = _boxes_f32(boxes_per_image[b])
            lb = None if labels_per_image is None else labels_per_image[b]
            if coefs.applied[b] and bx.shape[0] > 0:
                moved, keep = _warp_rows(coefs.m[b], int(h), int(w), min_visibility, bx)
                bx = moved[keep]
                if lb is not None:
                    lb = lb[torch.from_numpy(keep).to(lb.device)] if isinstance(lb, Tensor) else np.asarray(lb)[keep]
            out.append((torch.from_numpy(np.ascontiguousarray(bx)), lb))
        return out

    @staticmethod
    def warp_image(img: Tensor, inv: Sequence[float], applied: bool = True) -> Tensor:
        """Restatement of step 5 on a [3, h, w] fp32 tensor (CPU or CUDA) out of torch elementwise operations in the kernel's order, one
        rounding each: the image gathered through ``inv`` = (i00, i01, i02, i10, i11, i12), bilinear, reflect-101.  ``applied`` false:
        the image itself."""
        if not applied:
            return img
        h, w = int(img.shape[-2]), int(img.shape[-1])
        i = [torch.tensor(float(np.float32(v)), dtype=torch.float32, device=img.device) for v in inv]
        ys = torch.arange(h, dtype=torch.float32, device=img.device).reshape(h, 1)
        xs = torch.arange(w, dtype=torch.float32, device=img.device).reshape(1, w)
        big = torch.tensor(2.0 ** 30, dtype=torch.float32, device=img.device)

        def sat(s):
            s = torch.where(s >= -big, s, -big)
            return torch.where(s <= big, s, big)

        def reflect(idx, n):
            if n == 1:
                return torch.zeros_like(idx)
            period = 2 * (n - 1)
            t = torch.remainder(idx, period)
            return torch.where(t < n, t, period - t)

        sx, sy = sat((i[0] * xs + i[1] * ys) + i[2]), sat((i[3] * xs + i[4] * ys) + i[5])
        flx, fly = torch.floor(sx), torch.floor(sy)
        fx, fy = sx - flx, sy - fly
        x0, y0 = flx.to(torch.int64), fly.to(torch.int64)
        xa, xb, ya, yb = reflect(x0, w), reflect(x0 + 1, w), reflect(y0, h), reflect(y0 + 1, h)
        flat = img.reshape(img.shape[0], h * w)
        p00, p01, p10, p11 = (flat[:, (yy * w + xx).reshape(-1)].reshape(img.shape) for yy, xx in ((ya, xa), (ya, xb), (yb, xa), (yb, xb)))
        gx, gy = 1.0 - fx, 1.0 - fy
        return (p00 * gx + p01 * fx) * gy + (p10 * gx + p11 * fx) * fy

    def draw(self, counter: int, in_hw: Sequence[Tuple[int, int]], boxes_per_image) -> AffineCoefs:
        "The coefficients this object draws at ``counter`` for images of sizes ``in_hw`` with these boxes (no state change)."
        lo, hi = self.ranges
        return self.draw_coefs(self._seed, counter, in_hw, boxes_per_image, self._p, lo, hi, self.min_visibility)

    def next_coefs(self, in_hw: Sequence[Tuple[int, int]], boxes_per_image) -> AffineCoefs:
        """The next batch's coefficients on the HOST, and the counter advanced by one: what CPU tensors and CUDA lists use.  The boxes
        are read on the host (CUDA tensors are copied back: a synchronisation) and, with a device block, so is the counter; not
        inside a capture."""
        boxes = [_boxes_f32(b) for b in boxes_per_image]
        self.coefs = self._host_draw(lambda n: self.draw(n, in_hw, boxes))
        return self.coefs

    def device_block(self, device: torch.device) -> Tensor:
        """The ``rn_affine_state`` block on ``device`` that ``ops.shift_scale_rotate_staged`` draws from, created at the first call
        (which must not be inside a capture) and kept for good: a captured step holds its address."""
        if torch.device(device).type != "cuda":
            raise RuntimeError("ShiftScaleRotate: the device draw runs on the GPU; CPU batches use next_coefs()")
        return self._device_block(device)

    def set_limits(self, shift_limit=None, scale_limit=None, rotate_limit=None, min_visibility=None) -> None:
        "New ranges (the ones not given stay): written into the device block (no re-capture needed; not inside a capture)."
        scale_now = tuple(float(np.float32(v - 1.0)) for v in self.scale_range)
        self._set_ranges(self.shift_limit if shift_limit is None else shift_limit, scale_now if scale_limit is None else scale_limit,
                         self.rotate_limit if rotate_limit is None else rotate_limit,
                         self.min_visibility if min_visibility is None else min_visibility)
        lo, hi = self.ranges
        self._write(min_visibility=self.min_visibility, lo=lo, hi=hi)


_SHIFT_SCALE_ROTATE_NAMES = ("albumentations.ShiftScaleRotate", "ShiftScaleRotate")
# (parameter, the values that mean albumentations' default): cv2.INTER_LINEAR = 1, cv2.BORDER_REFLECT_101 = 4
_SSR_FIXED = (("interpolation", (None, 1, "cv2.INTER_LINEAR")), ("border_mode", (None, 4, "cv2.BORDER_REFLECT_101")), ("value", (None,)), ("shift_limit_x", (None,)), ("shift_limit_y", (None,)))


def shift_scale_rotate_from_transforms(entries, seed: int = 0, log=None) -> Optional[ShiftScaleRotate]:
    """The shift / scale / rotate an hparams ``transforms`` list asks for, or None.  ``albumentations.ShiftScaleRotate`` and a bare
    ``ShiftScaleRotate`` (``shift_limit`` 0.0625, ``scale_limit`` 0.1, ``rotate_limit`` 45, ``p`` 0.5: albumentations' defaults;
    ``always_apply: true`` means p = 1) map onto ``ShiftScaleRotate``, which is bilinear with the reflect-101 border and not
    bit-compatible with albumentations.  A non-default ``interpolation``, ``border_mode``, ``value``, ``shift_limit_x`` or
    ``shift_limit_y`` is warned about and ignored; a second entry is skipped with a warning."""
    log = log or logging.getLogger(__name__)
    found = None
    for name, params in _named(entries, _SHIFT_SCALE_ROTATE_NAMES, "shift / scale / rotate", log):
        for key, defaults in _SSR_FIXED:
            if params.get(key) not in defaults:
                log.warning("transforms: %s %s=%s is not implemented and is ignored (bilinear interpolation, the reflect-101 border and "
                            "one shift_limit for both axes are)", name, key, params.get(key))
        found = ShiftScaleRotate(shift_limit=_as_limit(params.get("shift_limit", 0.0625)), scale_limit=_as_limit(params.get("scale_limit", 0.1)),
                                 rotate_limit=_as_limit(params.get("rotate_limit", 45)), p=_entry_p(params, 0.5), seed=seed)
    return found


_COLOR_JITTER_NAMES = ("albumentations.ColorJitter", "torchvision.transforms.ColorJitter", "ColorJitter")


def color_jitter_from_transforms(entries, seed: int = 0, log=None) -> Optional[ColorJitter]:
    """The colour jitter an hparams ``transforms`` list asks for, or None.  ``albumentations.ColorJitter`` (brightness, contrast,
    saturation and hue default to 0.2, ``p`` to 0.5; ``always_apply: true`` means p = 1) and ``torchvision.transforms.ColorJitter`` /
    a bare ``ColorJitter`` (each default 0, p = 1) map onto ``ColorJitter``, whose arithmetic is torchvision's tensor algorithm:
    albumentations works on uint8 through OpenCV and differs slightly.  Other entries are ``from_transforms``' business."""
    log = log or logging.getLogger(__name__)
    found = None
    for name, params in _named(entries, _COLOR_JITTER_NAMES, "colour jitter", log):
        alb = name.startswith("albumentations.")
        default = 0.2 if alb else 0
        found = ColorJitter(p=_entry_p(params, 0.5 if alb else 1.0), seed=seed, **{n: _as_limit(params.get(n, default)) for n in COLOR_OPS})
    return found


_BRIGHTNESS_CONTRAST_NAMES = ("albumentations.RandomBrightnessContrast", "RandomBrightnessContrast")


def brightness_contrast_from_transforms(entries, seed: int = 0, log=None) -> Optional[RandomBrightnessContrast]:
    """The brightness / contrast an hparams ``transforms`` list asks for, or None.  ``albumentations.RandomBrightnessContrast`` and a
    bare ``RandomBrightnessContrast`` (``brightness_limit`` 0.2, ``contrast_limit`` 0.2, ``brightness_by_max`` true, ``p`` 0.5:
    albumentations' defaults; ``always_apply: true`` means p = 1) map onto ``RandomBrightnessContrast``, which works on fp32 without the
    uint8 LUT's quantisation and is not bit-compatible with albumentations.  A second entry is skipped with a warning.  The mapping is
    opt-in: ``SimpleTrainer(device_brightness_contrast=True)`` or ``trainer.device_brightness_contrast`` in the hparams calls it."""
    log = log or logging.getLogger(__name__)
    found = None
    for name, params in _named(entries, _BRIGHTNESS_CONTRAST_NAMES, "brightness / contrast", log):
        found = RandomBrightnessContrast(brightness_limit=_as_limit(params.get("brightness_limit", 0.2)),
                                         contrast_limit=_as_limit(params.get("contrast_limit", 0.2)),
                                         brightness_by_max=bool(params.get("brightness_by_max", True)), p=_entry_p(params, 0.5), seed=seed)
    return found


# (slot of the transform, the class names its mapper owns, the mapper) for every slot but the flip's.  A new mapper registers here, once:
# ``from_transforms`` leaves these entries to their mappers instead of calling them unsupported, and ``RetinaNetModel.prepare_data``
# installs what the mappers return.
SLOT_MAPPERS = (("brightness_contrast", _BRIGHTNESS_CONTRAST_NAMES, brightness_contrast_from_transforms),
                ("color_jitter", _COLOR_JITTER_NAMES, color_jitter_from_transforms),
                ("crop", _BBOX_CROP_NAMES, bbox_crop_from_transforms),
                ("shift_scale_rotate", _SHIFT_SCALE_ROTATE_NAMES, shift_scale_rotate_from_transforms))
_NAME_OWNER = {name: slot for slot, names, _ in SLOT_MAPPERS for name in names}


def from_transforms(entries, seed: int = 0, log=None, brightness_contrast: bool = False) -> Optional[RandomHorizontalFlip]:
    """The flip an hparams ``transforms`` list asks for (reference ``hparams.yaml:55-58``), or None.  ``albumentations.HorizontalFlip``
    (``p``, default 0.5; ``always_apply: true`` means p = 1) and ``RandomHorizontalFlip`` (``prob``, default 0.5; any module path) map
    onto ``RandomHorizontalFlip``.  albumentations itself is not used: every other entry is skipped with one warning naming it.
    ``brightness_contrast``: the caller maps a ``RandomBrightnessContrast`` entry itself (``brightness_contrast_from_transforms``: the
    ``device_brightness_contrast`` switch), so it is not warned about here."""
    log = log or logging.getLogger(__name__)
    found = None
    for name, params in _entries(entries):
        short = name.rsplit(".", 1)[-1]
        if name in ("albumentations.HorizontalFlip", "HorizontalFlip"):
            p = _entry_p(params, 0.5)
        elif short == "RandomHorizontalFlip":
            p = float(params.get("prob", params.get("p", 0.5)))
        elif name in _NAME_OWNER and (brightness_contrast or _NAME_OWNER[name] != "brightness_contrast"):
            continue                                   # the slot's own mapper maps it (SLOT_MAPPERS)
        elif name in _NAME_OWNER:
            log.warning("transforms: %s is skipped: it is implemented on the GPU (augment.RandomBrightnessContrast) but stays off unless "
                        "SimpleTrainer(device_brightness_contrast=True) or trainer.device_brightness_contrast in the hparams installs it", name)
            continue
        else:
            log.warning("transforms: %s is not supported (albumentations is not available; only the horizontal flip, ColorJitter, "
                        "BBoxSafeRandomCrop and ShiftScaleRotate are implemented, on the GPU): skipped", name)
            continue
        if found is not None:
            log.warning("transforms: a second horizontal flip (%s) is skipped", name)
            continue
        found = RandomHorizontalFlip(p=p, seed=seed)
    return found
