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
"""
from typing import Dict, List, Optional

import numpy as np
import torch
from torch import Tensor

__all__ = ["RandomHorizontalFlip", "hflip_u"]

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
