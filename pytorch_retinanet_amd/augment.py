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
"""
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

__all__ = ["RandomHorizontalFlip", "RandomShortSide", "hflip_u"]

_M64 = 2 ** 64 - 1


def hflip_u(seed: int, counter: int, b: int) -> float:
    "The uniform in [0, 1) (24 bits) behind image b's decision at ``counter`` (``csrc/augment.hip``)."
    z = (seed ^ (counter * 0x9E3779B97F4A7C15) ^ ((b + 1) * 0xD1B54A32D192ED03)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return (z >> 40) * 2.0 ** -24


class RandomHorizontalFlip:
    """Flip each training image (and its boxes: x1' = W - x2, x2' = W - x1) with probability ``p``.  Install it as
    ``net.transform.hflip``; it acts only in training mode and only when targets are given.  Not an ``nn.Module``: it adds no key
    to the model's state dict.  ``seed``: the stream of decisions (``SimpleTrainer`` adds the rank under ``torch.distributed``)."""

    def __init__(self, p: float = 0.5, seed: int = 0):
        self.base_seed = int(seed) & _M64
        self._p, self._seed, self._counter = self._check_p(p), self.base_seed, 0
        self._block: Optional[Tensor] = None          # rn_hflip_state on the device of the first CUDA batch (kept for good)
        self.flags: Optional[Tensor] = None           # the last batch's decisions (uint8 [B]; device or CPU)

    @staticmethod
    def _check_p(p) -> float:
        p = float(p)
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"flip probability must be in [0, 1], got {p}")
        return float(np.float32(p))

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
            flags = torch.tensor(self.draw(self._counter, B), dtype=torch.uint8)
            self._counter += 1
        else:
            from . import ops
            if device.index is None:
                device = torch.device("cuda", torch.cuda.current_device())
            if self._block is None:
                self._block = ops.hflip_state(device, self._seed, self._counter, self._p)
            elif self._block.device != device:
                # (a captured step holds the block's address: it is never replaced while this object lives)
                raise RuntimeError(f"RandomHorizontalFlip: its state lives on {self._block.device}, not {device}; use one object per device")
            flags = ops.hflip_draw(self._block, B)
        self.flags = flags
        return flags

    # -- settings and state ---------------------------------------------------------------------------------------------
    @property
    def p(self) -> float:
        return self._p

    @p.setter
    def p(self, value: float) -> None:
        "A new probability: written into the device block (no re-capture needed; not inside a capture)."
        self._p = self._check_p(value)
        if self._block is not None:
            from . import ops
            ops.hflip_state_write(self._block, p=self._p)

    @property
    def seed(self) -> int:
        return self._seed

    def reseed(self, seed: int, counter: int = 0) -> None:
        "Start a new stream of decisions (seed, counter); not inside a capture."
        self._seed, self._counter = int(seed) & _M64, int(counter)
        if self._block is not None:
            from . import ops
            ops.hflip_state_write(self._block, seed=self._seed, counter=self._counter)

    def set_rank(self, rank: int) -> None:
        """One stream per data-parallel rank: seed = ``base_seed`` (the constructor's) + rank, the counter kept.  Without it every rank
        would flip the same batch positions."""
        self.reseed((self.base_seed + int(rank)) & _M64, self.counter)

    @property
    def counter(self) -> int:
        "Batches drawn so far (with the device block: one read-back, i.e. a synchronisation)."
        if self._block is not None:
            from . import ops
            return int(ops.hflip_state_read(self._block)[1])
        return self._counter

    def state_dict(self) -> Dict[str, object]:
        return {"seed": self._seed, "counter": self.counter, "p": self._p}

    def load_state_dict(self, state: Dict[str, object]) -> None:
        self._p = self._check_p(state["p"])
        self.reseed(int(state["seed"]), int(state["counter"]))
        if self._block is not None:
            from . import ops
            ops.hflip_state_write(self._block, p=self._p)


SHORT_SIDE_SALT = 0x5CA1E5CA1E5CA1E5      # xor-ed into the seed: a flip and a jitter that share a seed must not tie small sizes to flipped images
SHORT_SIDE_MAX = 16                       # candidate short sides a device block holds (include/retinanet_hip.h: RN_SHORT_SIDE_MAX)


def short_side_hw(h: int, w: int, short: float, max_size: float) -> Tuple[int, int]:
    """The size ``GeneralizedRCNNTransform`` resizes an h x w image to for the short side ``short``: ``_scale_for`` and the two floors
    of ``resize``, in double and in their order of operations (``csrc/augment.hip`` does the same on the device)."""
    lo, hi = float(min(h, w)), float(max(h, w))
    scale = float(short) / lo
    if hi * scale > float(max_size):
        scale = float(max_size) / hi
    return int(math.floor(h * scale)), int(math.floor(w * scale))


class RandomShortSide:
    """Resize each training image to a short side drawn from ``sizes`` (torchvision's ``min_size`` tuple), one draw per image and step,
    made on the device.  Install it as ``net.transform.scale_jitter``; it acts only in training mode and only when targets are given,
    and while it is installed the transform's own host-side draw from ``min_size`` is not consulted in training.  Not an
    ``nn.Module``: it adds no key to the model's state dict.  At most 16 sizes.  The padded canvas is sized for the largest entry
    the object was built with (``canvas_short``), whatever is drawn: one captured graph serves every scale, and small draws save
    no compute.  ``seed``: the stream of draws (``SimpleTrainer`` adds the rank under ``torch.distributed``)."""

    def __init__(self, sizes: Sequence[int], seed: int = 0):
        self.base_seed = int(seed) & _M64
        self._sizes = self._check_sizes(sizes)
        self.canvas_short = max(self._sizes)          # the canvas bound: fixed for good (a captured step holds the canvas)
        self._seed, self._counter = self.base_seed, 0
        self._block: Optional[Tensor] = None          # rn_short_side_state on the device of the first CUDA batch (kept for good)
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
            hw = self.draw(self._counter, in_hw_list, max_size)
            sizes = torch.tensor(hw, dtype=torch.int32).reshape(-1, 2)
            ratios = torch.tensor(self.ratios(in_hw_list, hw), dtype=torch.float32).reshape(-1)
            self._counter += 1
        else:
            from . import ops
            if int(max_size) != max_size:
                raise ValueError(f"the device draw takes an integer max_size, got {max_size}")
            if device.index is None:
                device = torch.device("cuda", torch.cuda.current_device())
            if self._block is None:
                self._block = ops.short_side_state(device, self._seed, self._counter, self._sizes)
            elif self._block.device != device:
                # (a captured step holds the block's address: it is never replaced while this object lives)
                raise RuntimeError(f"RandomShortSide: its state lives on {self._block.device}, not {device}; use one object per device")
            sizes, ratios = ops.short_side_draw(self._block, in_hw_list, int(max_size))
        self.sizes_drawn, self.ratios_drawn = sizes, ratios
        return sizes, ratios

    def next_sizes_dev(self, in_hw: Tensor, max_size: float) -> Tuple[Tensor, Tensor]:
        """``next_sizes`` for images whose sizes only the device holds (``in_hw`` int32 [B, 2] on a CUDA device, as ``ops.image_stage``
        writes it: the image capacity mode of ``graph.CapturedTrainStep``): one ``rn_resize_plan_dev`` launch for any B (capturable).
        The same stream of draws: at counter n it gives what ``draw(n, sizes, max_size)`` gives for the sizes ``in_hw`` holds, and
        the counter advances by one."""
        from . import ops
        if int(max_size) != max_size:
            raise ValueError(f"the device draw takes an integer max_size, got {max_size}")
        device = in_hw.device
        if device.type != "cuda":
            raise RuntimeError("RandomShortSide.next_sizes_dev: the sizes must be on the GPU (there is no CPU fallback)")
        if self._block is None:
            self._block = ops.short_side_state(device, self._seed, self._counter, self._sizes)
        elif self._block.device != device:
            raise RuntimeError(f"RandomShortSide: its state lives on {self._block.device}, not {device}; use one object per device")
        sizes, ratios = ops.resize_plan_dev(self._block, in_hw, None, int(max_size))
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
        if self._block is not None:
            from . import ops
            ops.short_side_state_write(self._block, sizes=self._sizes)

    @property
    def seed(self) -> int:
        return self._seed

    def reseed(self, seed: int, counter: int = 0) -> None:
        "Start a new stream of draws (seed, counter); not inside a capture."
        self._seed, self._counter = int(seed) & _M64, int(counter)
        if self._block is not None:
            from . import ops
            ops.short_side_state_write(self._block, seed=self._seed, counter=self._counter)

    def set_rank(self, rank: int) -> None:
        "One stream per data-parallel rank: seed = ``base_seed`` (the constructor's) + rank, the counter kept."
        self.reseed((self.base_seed + int(rank)) & _M64, self.counter)

    @property
    def counter(self) -> int:
        "Batches drawn so far (with the device block: one read-back, i.e. a synchronisation)."
        if self._block is not None:
            from . import ops
            return int(ops.short_side_state_read(self._block)[1])
        return self._counter

    def state_dict(self) -> Dict[str, object]:
        return {"seed": self._seed, "counter": self.counter, "sizes": list(self._sizes)}

    def load_state_dict(self, state: Dict[str, object]) -> None:
        self.sizes = state["sizes"]
        self.reseed(int(state["seed"]), int(state["counter"]))


def from_transforms(entries, seed: int = 0, log=None) -> Optional[RandomHorizontalFlip]:
    """The flip an hparams ``transforms`` list asks for (reference ``hparams.yaml:55-58``), or None.  ``albumentations.HorizontalFlip``
    (``p``, default 0.5; ``always_apply: true`` means p = 1) and ``RandomHorizontalFlip`` (``prob``, default 0.5; any module path) map
    onto ``RandomHorizontalFlip``.  albumentations itself is not used: every other entry is skipped with one warning naming it."""
    import logging
    log = log or logging.getLogger(__name__)
    found = None
    for e in entries or []:
        name = str(e.get("class_name", "")) if isinstance(e, dict) else str(e)
        params = dict(e.get("params") or {}) if isinstance(e, dict) else {}
        short = name.rsplit(".", 1)[-1]
        if name in ("albumentations.HorizontalFlip", "HorizontalFlip"):
            p = 1.0 if params.get("always_apply") else float(params.get("p", 0.5))
        elif short == "RandomHorizontalFlip":
            p = float(params.get("prob", params.get("p", 0.5)))
        else:
            log.warning("transforms: %s is not supported (albumentations is not available; only the horizontal flip is implemented, "
                        "on the GPU): skipped", name)
            continue
        if found is not None:
            log.warning("transforms: a second horizontal flip (%s) is skipped", name)
            continue
        found = RandomHorizontalFlip(p=p, seed=seed)
    return found
