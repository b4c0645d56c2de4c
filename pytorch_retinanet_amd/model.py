"""``RetinaNetModel`` -- the Lightning-style wrapper of the reference (``model.py:18-147``):
same constructor (``RetinaNetModel(conf)``), same hook names, same step-output dict keys
(``loss`` / ``log`` / ``progress_bar``, ``val_loss``, ``AP``).

``pytorch_lightning`` is used as the base class when it is importable; otherwise a minimal
local base provides the two things the hooks rely on (``save_hyperparameters`` and
``nn.Module``), and ``SimpleTrainer`` below drives the hooks (one process per GPU, gradients
exchanged by ``parallel.BucketedGradAllReduce`` over RCCL).

Data: ``dataset.kind: synthetic`` or ``csv`` (the reference's csv format, ``datasets.py``); the COCO-json /
Pascal-xml readers and albumentations pipelines of the reference's ``utils/`` are outside this framework's
scope (``prepare_data`` says so); the one augmentation the reference trains with, the horizontal flip of the ``transforms``
block, runs on the GPU inside the model's transform (``augment.RandomHorizontalFlip``, installed by ``prepare_data`` for csv).  ``test_step`` / ``test_epoch_end`` feed the pycocotools-free
``coco_eval.CocoEvaluator`` (reference ``utils/coco/coco_eval.py``).
"""
import argparse
import logging
from typing import Any, Dict, List, Optional, Union

import torch
from torch import nn
from torch.utils.data import DataLoader, Dataset

from .graph import gt_capacity_classes, image_capacity_classes
from .models import Retinanet
from .optim import check_accumulate_grad_batches
from .utils import AttrDict, collate_fn, load_obj

try:                                                   # pragma: no cover - not installed in this image
    import pytorch_lightning as pl
    _Base = pl.LightningModule
except Exception:                                      # noqa: BLE001
    pl = None

    class _Base(nn.Module):
        "The slice of LightningModule the hooks below need."

        def save_hyperparameters(self, conf) -> None:
            self.hparams = conf


class SyntheticDetectionDataset(Dataset):
    """Random images + boxes in the reference's sample format ``(image, target, image_idx)``
    (``utils/pascal/pascal_utils.py:98-142``): image ``F32[3,H,W]`` in 0..1, target
    ``{"boxes": F32[T,4] xyxy, "labels": I64[T] in 1..K, "image_id": I64[1]}``."""

    def __init__(self, length: int = 16, height: int = 800, width: int = 1333, num_classes: int = 90,
                 boxes_per_image: int = 8, seed: int = 0):
        self.length, self.h, self.w, self.k, self.t, self.seed = length, height, width, num_classes, boxes_per_image, seed

    def __len__(self) -> int:
        return self.length

    def __getitem__(self, idx: int):
        g = torch.Generator().manual_seed(self.seed * 1000003 + idx)
        img = torch.rand(3, self.h, self.w, generator=g)
        cx = torch.rand(self.t, generator=g) * self.w
        cy = torch.rand(self.t, generator=g) * self.h
        bw = 16 + torch.rand(self.t, generator=g) * 300
        bh = 16 + torch.rand(self.t, generator=g) * 300
        boxes = torch.stack([(cx - bw / 2).clamp(0, self.w - 2), (cy - bh / 2).clamp(0, self.h - 2),
                             (cx + bw / 2).clamp(0, self.w), (cy + bh / 2).clamp(0, self.h)], 1)
        boxes[:, 2:] = torch.maximum(boxes[:, 2:], boxes[:, :2] + 1.0)
        labels = torch.randint(1, self.k + 1, (self.t,), generator=g)
        return img, {"boxes": boxes, "labels": labels, "image_id": torch.tensor([idx])}, idx


class RetinaNetModel(_Base):
    def __init__(self, conf: Union[AttrDict, Dict[str, Any], argparse.Namespace]):
        super().__init__()
        self.conf = conf
        self.net = Retinanet(**conf.model, logger=logging.getLogger("lightning"))
        self.save_hyperparameters(conf)
        self.trn_ds = self.val_ds = self.test_ds = None
        self.test_evaluator = None
        self.predictor = None         # a callable images -> detections used by test_step instead of net.predict (graph.CapturedPredict)
        self.device_eval = False      # test_dataloader: score on the GPU (coco_eval.DeviceBBoxEval) when the net is on CUDA; SimpleTrainer sets it
        self.device_brightness_contrast = False      # prepare_data: map a RandomBrightnessContrast entry of the transforms; SimpleTrainer sets it

    def device_brightness_contrast_enabled(self) -> bool:
        "This model's ``device_brightness_contrast`` (``SimpleTrainer`` sets it) or ``trainer.device_brightness_contrast`` of its hparams."
        return bool(self.device_brightness_contrast or _hparam(self.conf, "device_brightness_contrast"))

    def forward(self, xb, *args, **kwargs):
        # reference model.py:33-35 calls self.net(xb) with no targets (a TypeError there, Q19);
        # here that means inference.
        return self.net(xb)

    # -- data ----------------------------------------------------------------------------------
    def prepare_data(self):
        d = self.conf.dataset
        if d.kind == "synthetic":
            kw = dict(num_classes=self.net.num_classes)
            kw.update({k: v for k, v in d.items() if k in ("length", "height", "width", "boxes_per_image", "seed")})
            self.trn_ds = SyntheticDetectionDataset(**kw)
            self.val_ds = SyntheticDetectionDataset(**{**kw, "seed": kw.get("seed", 0) + 1})
            self.test_ds = SyntheticDetectionDataset(**{**kw, "seed": kw.get("seed", 0) + 2})
        elif d.kind == "csv":             # README.md:103-125: trn_paths / val_paths (optional) / test_paths are csv files
            from functools import partial
            from .augment import SLOT_MAPPERS, from_transforms
            from .datasets import CSVDetectionDataset
            # the training set's transforms (reference model.py:51-52, hparams.yaml:55-58) run on the GPU, inside the model's transform:
            # each mapper turns the entries it owns into the object of its slot (the flip, albumentations' or torchvision's ColorJitter,
            # BBoxSafeRandomCrop, ShiftScaleRotate: augment.py); validation / test never augment (eval mode, no targets)
            # (RandomBrightnessContrast is opt-in: with the switch its entry is mapped too, without it the flip's mapping warns about it)
            bc_on = self.device_brightness_contrast_enabled()
            mappers = (("hflip", partial(from_transforms, brightness_contrast=bc_on)),) + tuple((slot, mapper) for slot, _, mapper in SLOT_MAPPERS)
            for slot, mapper in mappers:
                if slot != "brightness_contrast" or bc_on:
                    setattr(self.net.transform, slot, mapper(self.conf.get("transforms")))
            # dataset.image_dtype (optional; "float32" or "uint8"): "uint8" hands the decoder's bytes to the model, which converts them
            # on the device (ops.image_stage_u8 on the staged path, ops.images_u8_to_f32 in the transform)
            dt = d.get("image_dtype") or "float32"
            self.trn_ds = CSVDetectionDataset(d.trn_paths, image_dtype=dt)
            self.val_ds = CSVDetectionDataset(d.val_paths, image_dtype=dt) if d.get("val_paths") else None
            self.test_ds = CSVDetectionDataset(d.test_paths, image_dtype=dt) if d.get("test_paths") else None
        elif d.kind in ("coco", "pascal"):
            raise NotImplementedError(
                f"dataset.kind={d.kind!r}: the reference's COCO-json / Pascal-xml readers (utils/coco, utils/pascal; "
                "pycocotools, albumentations, cv2) are outside this framework's scope. Convert to the csv format "
                "(kind: csv), assign `trn_ds` / `val_ds` / `test_ds` with your own Dataset yielding "
                "(image, target, image_idx), or use kind: synthetic.")
        else:
            raise ValueError("DATASET_KIND not supported")

    def _loader(self, ds, bs, shuffle=False, shard=False):
        """``shard``: under ``torch.distributed`` the rank reads its own shard (``DistributedSampler``, what Lightning injects
        for the reference's train / val loaders); ``SimpleTrainer`` calls ``sampler.set_epoch`` so the shards reshuffle per
        epoch.  The TEST loader is never sharded: ``test_epoch_end`` scores the detections a rank has seen, a shard would
        report AP on 1/W of the images and the sampler's padding would duplicate image ids; every rank evaluates the full set."""
        import torch.distributed as dist
        sampler = None
        if shard and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            from torch.utils.data.distributed import DistributedSampler
            sampler = DistributedSampler(ds, shuffle=shuffle)
            shuffle = False
        return DataLoader(ds, bs, shuffle=shuffle, sampler=sampler, collate_fn=collate_fn, **dict(self.conf.dataloader.args))

    def train_dataloader(self, *args, **kwargs):
        return self._loader(self.trn_ds, self.conf.dataloader.train_bs, shuffle=True, shard=True)

    def val_dataloader(self, *args, **kwargs):
        # sharded: SimpleTrainer averages the validation loss over ranks (a padded duplicate shifts a mean loss by O(1/len))
        return None if self.val_ds is None else self._loader(self.val_ds, self.conf.dataloader.valid_bs, shard=True)

    def test_dataloader(self, *args, **kwargs):
        from .coco_eval import CocoEvaluator, gt_from_dataset
        loader = self._loader(self.test_ds, self.conf.dataloader.test_bs)
        # device_eval: the metric's matching and precision / recall rows as HIP kernels, the detections kept on the device
        device = next(self.net.parameters()).device if self.device_eval else None
        device = device if device is not None and device.type == "cuda" else None
        self.test_evaluator = CocoEvaluator(gt_from_dataset(loader.dataset), ["bbox"], device=device)       # reference model.py:105-110
        return loader

    # -- optimisation ----------------------------------------------------------------------------
    def configure_optimizers(self, *args, **kwargs):
        opt_cls = load_obj(self.conf.optimizer.class_name)
        if getattr(opt_cls, "_rn_master_weights", False) and next(self.net.parameters()).is_cuda:
            # optimizer.class_name: pytorch_retinanet_amd.optim.MasterSGD / MasterAdam / MasterAdamW -- the update on fp32 masters,
            # conv weights held in 16 bits
            from .optim import use_16bit_conv_weights
            use_16bit_conv_weights(self.net, getattr(self, "working_dtype", None) or torch.bfloat16)     # (SimpleTrainer sets it from its precision)
        self.optimizer = opt_cls(self.net.parameters(), **dict(self.conf.optimizer.params))
        sched = self.conf.scheduler
        if sched.class_name is None:
            return [self.optimizer]
        params = dict(sched.params)
        if "verbose" in params:
            import inspect
            if "verbose" not in inspect.signature(load_obj(sched.class_name).__init__).parameters:
                params.pop("verbose")               # removed from torch schedulers after the reference was written
        scheduler = load_obj(sched.class_name)(self.optimizer, **params)
        self.scheduler = {"scheduler": scheduler, "interval": sched.interval, "frequency": sched.frequency}
        if sched.monitor:
            self.scheduler["monitor"] = sched.monitor
        return [self.optimizer], [self.scheduler]

    # -- steps (same dict contracts as reference model.py:112-146) ---------------------------------
    def training_step(self, batch, batch_idx, *args, **kwargs):
        images, targets, _ = batch
        targets = [{k: v for k, v in t.items()} for t in targets]
        loss_dict = self.net(images, targets)
        losses = sum(loss for loss in loss_dict.values())
        return {"loss": losses, "log": loss_dict, "progress_bar": loss_dict}

    def validation_step(self, batch, batch_idx, *args, **kwargs):
        images, targets, _ = batch
        targets = [{k: v for k, v in t.items()} for t in targets]
        loss_dict = self.net(images, targets)
        loss = torch.as_tensor(sum(loss for loss in loss_dict.values()))
        logs = {"val_loss": loss}
        return {"val_loss": loss, "log": logs, "progress_bar": logs}

    def test_step(self, batch, batch_idx, *args, **kwargs):
        images, targets, _ = batch
        targets = [{k: v for k, v in t.items()} for t in targets]
        outputs = self.net.predict(images) if self.predictor is None else self.predictor(images)
        res = {t["image_id"].item(): o for t, o in zip(targets, outputs)}
        if self.test_evaluator is not None:
            self.test_evaluator.update(res)
        return {"detections": res}

    def test_epoch_end(self, outputs, *args, **kwargs):
        if self.test_evaluator is None:
            return {}
        self.test_evaluator.accumulate()
        self.test_evaluator.summarize()
        metric = torch.as_tensor(self.test_evaluator.coco_eval["bbox"].stats[0])
        logs = {"AP": metric}
        return {"AP": metric, "log": logs, "progress_bar": logs}


def _with_last(loader):
    "``(index, batch, is_last)`` over ``loader``, one batch ahead (works for loaders without a length)."
    it = iter(loader)
    try:
        nxt = next(it)
    except StopIteration:
        return
    i = 0
    while True:
        cur = nxt
        try:
            nxt = next(it)
        except StopIteration:
            yield i, cur, True
            return
        yield i, cur, False
        i += 1


def _to_device(batch, device):
    images, targets, ids = batch
    images = [im.to(device, non_blocking=True) for im in images]
    targets = [{k: v.to(device, non_blocking=True) for k, v in t.items()} for t in targets]
    return images, targets, ids


def _hparam(conf, name: str):
    "``trainer.<name>`` of the hparams, or None: no hparams, no ``trainer`` section, no such key."
    section = conf.get("trainer") if hasattr(conf, "get") else None
    return (section or {}).get(name)


def _number(allowed, rule: str):
    "A parser of ``TRAINER_OPTIONS`` for a float option: ``allowed(v)`` or a ValueError ``<label> must be <rule>, got ...``."
    def parse(value, label: str) -> float:
        v = float(value or 0.0)
        if not allowed(v):
            raise ValueError(f"{label} must be {rule}, got {value}")
        return v
    return parse


def _switch(value, label: str) -> bool:
    return bool(value)


def _canvases(value, label: str):
    """None, "auto" or a list of padded canvases (Hp, Wp), checked by ``graph.image_capacity_classes`` (bad values fail here, not at
    the first step; divisibility by the net's ``size_divisible`` is checked once the net is known).  YAML's [Hp, Wp] lists, whose
    numbers may come as whole floats, become tuples of ints first."""
    if isinstance(value, (list, tuple)):
        value = [tuple(int(v) if isinstance(v, float) and v == int(v) else v for v in c) if isinstance(c, list) else c for c in value]
    image_capacity_classes(value)
    return value


# The options of ``SimpleTrainer`` that the hparams' optional ``trainer`` section may also set: name -> (the off value, the parser).
# ``parse(value, label)`` returns the value as the trainer keeps it or raises ValueError; ``label`` is the name for a constructor
# argument and ``trainer.<name>`` for an hparams entry.  The constructor's value wins unless it is the off value (``_resolve``).
TRAINER_OPTIONS = {
    "gradient_clip_val": (0.0, _number(lambda v: v >= 0.0, ">= 0 (0 = off)")),
    "accumulate_grad_batches": (1, check_accumulate_grad_batches),
    "weight_ema_decay": (0.0, _number(lambda v: 0.0 <= v < 1.0, "in [0, 1) (0 = off)")),
    "weight_ema_warmup": (0.0, _number(lambda v: 0.0 <= v < float("inf"), "a finite number >= 0 (0 = no warm-up)")),
    "device_scale_jitter": (False, _switch),
    "image_capacity": (None, _canvases),
    "predict_image_capacity": (None, _canvases),
    "device_eval": (False, _switch),
    "device_brightness_contrast": (False, _switch),
}


class SimpleTrainer:
    """Minimal stand-in for ``pl.Trainer`` driving the hooks above on ONE device per process:
    ``fit`` (train + optional validation, scheduler stepping per the hparams contract) and ``test``.
    Under ``torch.distributed`` every rank runs this loop on its own shard of the dataset (``DistributedSampler``),
    gradients are averaged by ``BucketedGradAllReduce`` and the validation loss is averaged over ranks before it
    reaches a monitoring scheduler.  Validation runs in ``eval()`` mode like Lightning's (BN buffers untouched).
    After ``fit``: ``captured_steps`` = the steps served by a graph replay, ``captured_graphs`` = the graphs captured for them (one per
    input signature that reached a replay; with the capacity modes: one per class met)."""

    def __init__(self, max_epochs: int = 1, device: Optional[str] = None, precision: str = "bf16",
                 channels_last: bool = True, max_steps: Optional[int] = None, log_every: int = 10, capture: bool = True,
                 gt_capacity=None, gradient_clip_val: float = 0.0, accumulate_grad_batches: int = 1,
                 weight_ema_decay: float = 0.0, weight_ema_warmup: float = 0.0, device_scale_jitter: bool = False,
                 scale_jitter_seed: int = 0, image_capacity=None, predict_image_capacity=None, device_eval: bool = False,
                 device_brightness_contrast: bool = False):
        """``capture``: replay each step as one hipGraph (``graph.CapturedTrainStep`` -- what ``bench.py``'s headline number is
        measured through: ~0.4 ms of host time per step instead of ~20 ms of Python enqueueing ~640 kernels) whenever the step
        is the plain one: one GPU, ``training_step`` not overridden, and no scheduler that changes the learning rate every step
        unless the optimizer reads its hyperparameters on the device (``optim.MasterAdam`` / ``MasterAdamW``, and ``MasterSGD`` with
        ``optimizer.params.capturable: true``: the step reads lr from a device block refreshed before each replay).  ``MasterSGD``
        without that flag and torch's optimizers take lr by value, which is part of a graph's signature: each new value would
        re-capture, so a per-step schedule runs them eagerly.  Batches of a new shape run
        eagerly twice, then replay; the results are the eager step's (``tests/test_graph_gpu.py``).  ``gt_capacity``: passed to the
        ``CapturedTrainStep`` -- "auto" keys batches by GT capacity class instead of by their exact box counts, so data with a
        different number of boxes per image still replays (None: exact keying).

        ``gradient_clip_val`` (Lightning's name and default; 0 = off; left at 0, an optional ``trainer.gradient_clip_val`` in the hparams
        is honoured): clip the gradients by global L2 norm before every optimizer step.  With ``optim.MasterSGD`` / ``MasterAdam`` /
        ``MasterAdamW`` the trainer installs an ``optim.GradClip`` on the optimizer (``self.grad_clip``) and nothing else changes: the
        norm and the scaling run on the device inside the step, capture stays on, and under ``torch.distributed`` the clip sees the
        exchanged gradients, so every rank computes the same coefficient.  Any other optimizer: one process only, eagerly (capture is
        turned off for the run, with a log line), ``torch.nn.utils.clip_grad_norm_`` after ``scaler.unscale_``.

        ``accumulate_grad_batches`` (Lightning's name and default; an int >= 1, dict schedules are refused; left at 1, an optional
        ``trainer.accumulate_grad_batches`` in the hparams is honoured): N micro-batches per optimizer step, Lightning's semantics --
        each contributes ``loss / N``, the optimizer steps after every N-th batch of an epoch and after its last batch (with whatever
        the window holds, still weighted 1 / N), ``interval: step`` schedulers, ``max_steps``, ``log_every`` and the return value of
        ``fit`` count OPTIMIZER steps, and the loss that is logged is the undivided micro-batch loss.  With a master optimizer on CUDA
        the trainer installs an ``optim.GradAccumulator`` (``self.grad_accumulator``): the micro-batch gradients are summed in fp32 on
        the device inside the step and capture stays on (a micro graph and a final graph per batch signature).  Any other optimizer
        or device: eagerly, ``(loss / N).backward()`` into ``.grad``, then step and zero every N; this composes with the torch clip
        and the stock ``GradScaler`` (unscaled once, at the step).  Single process only: N > 1 under ``torch.distributed`` raises.

        ``weight_ema_decay`` / ``weight_ema_warmup`` (0 = off; left at 0, optional ``trainer.weight_ema_decay`` / ``trainer.weight_ema_warmup``
        in the hparams are honoured): keep an exponential moving average of the weights (torchvision's ``--model-ema``, timm's
        ``ModelEma``) and validate / test on it.  With a master optimizer on CUDA the trainer installs an ``optim.WeightEMA`` on the
        optimizer (``self.weight_ema``): the update runs on the device inside ``optimizer.step`` (once per optimizer step, skipped with a
        step the loss scaler skips, identical on every rank) and capture stays on.  Validation inside ``fit`` and ``test()`` after it
        run inside ``weight_ema.swapped(...)``; training always resumes on the training weights.  BatchNorm running statistics are not
        averaged.  Any other optimizer or device raises: there is no CPU fallback.

        ``device_scale_jitter`` / ``scale_jitter_seed`` (off by default; left False, an optional ``trainer.device_scale_jitter`` in the
        hparams is honoured): multi-scale training inside the captured step.  When the model's ``min_size`` has more than one entry,
        ``fit`` installs ``augment.RandomShortSide(min_size, scale_jitter_seed)`` as ``net.transform.scale_jitter`` before the first step
        (``self.scale_jitter``; under ``torch.distributed`` rank r draws from seed + r): the short side of every image is drawn on the
        device over a canvas sized for the largest entry, so one graph replays while the scales vary.  Without it a ``min_size`` tuple
        is drawn on the host, which changes the canvas -- and with it the graph signature -- at nearly every step.  A single-entry
        ``min_size`` installs nothing and logs one line.  The cost: the whole canvas is processed whatever was drawn.

        ``image_capacity`` (None = off; left None, an optional ``trainer.image_capacity`` in the hparams is honoured): passed to the
        ``CapturedTrainStep`` -- "auto" or a list of padded canvases (Hp, Wp) keys batches by canvas class and pixel class instead of
        by their images' exact shapes, so data whose images differ in size still replays.  Needs ``gt_capacity``.  The cost: the conv
        stack processes the class canvas whatever the batch's own canvas was.

        ``predict_image_capacity`` (None = off; left None, an optional ``trainer.predict_image_capacity`` in the hparams is honoured):
        "auto" or a list of padded canvases (Hp, Wp) -- ``test()`` installs a ``graph.CapturedPredict`` over them as the model's
        ``predictor`` (``self.predictor``; removed again when ``test()`` returns), so every test batch is one graph replay keyed by its
        canvas class whatever its images' sizes are.  It runs inside the weight average's swap, and its graphs are dropped whenever the
        weights change.  CUDA only; the cost is the class canvas again.

        ``device_eval`` (off by default; left False, an optional ``trainer.device_eval`` in the hparams is honoured): ``test()`` scores the
        detections on the GPU -- the model's ``test_evaluator`` becomes a ``CocoEvaluator(device=...)`` whose ``coco_eval["bbox"]`` is a
        ``coco_eval.DeviceBBoxEval``: the detections stay on the device as tensors, the greedy matching and the precision / recall rows run
        as two HIP kernels (``rn_eval_match`` / ``rn_eval_accumulate``), and the 12 statistics are the host evaluator's bit for bit.  CUDA
        only: on another device the host evaluator is used as before.

        ``device_brightness_contrast`` (off by default; left False, an optional ``trainer.device_brightness_contrast`` in the hparams is
        honoured): the third transform of the reference's published recipe.  An ``albumentations.RandomBrightnessContrast`` entry of the
        hparams' ``transforms`` is mapped onto ``augment.RandomBrightnessContrast`` (albumentations' defaults) and installed as
        ``net.transform.brightness_contrast`` (``self.brightness_contrast``; under ``torch.distributed`` rank r draws from seed + r): drawn
        and applied on the device inside the captured step.  Without the switch the entry is skipped with one warning, as it always was."""
        given = locals()                                  # (the arguments by name: every option of the table is one)
        for name, (_, parse) in TRAINER_OPTIONS.items():
            setattr(self, name, parse(given[name], name))
        self.grad_accumulator = None                      # the optim.GradAccumulator of the last fit() (master optimizers on CUDA)
        self.grad_clip = None                             # the optim.GradClip of the last fit() (master optimizers)
        self.weight_ema = None                            # the optim.WeightEMA of the last fit() (master optimizers on CUDA)
        self.scale_jitter_seed = int(scale_jitter_seed)
        self.scale_jitter = None                          # the augment.RandomShortSide of the last fit()
        gt_capacity_classes(gt_capacity)                  # (bad values fail here, not at the first step)
        self.gt_capacity = gt_capacity
        if image_capacity is not None and gt_capacity is None:
            raise ValueError("image_capacity needs gt_capacity as well (\"auto\" or a class list)")
        self.predictor = None                             # the graph.CapturedPredict of the last test()
        self.brightness_contrast = None                   # the augment.RandomBrightnessContrast of the last fit()
        self.max_epochs, self.max_steps, self.log_every, self.capture = max_epochs, max_steps, log_every, capture
        self.captured_steps = 0
        self.captured_graphs = 0                          # captures of the last fit() (one per input signature that reached a replay)
        self.device = torch.device(device or ("cuda" if torch.cuda.is_available() else "cpu"))
        self.amp_dtype = {"bf16": torch.bfloat16, "16": torch.float16, "32": None}[str(precision)]
        self.channels_last = channels_last
        self.log = logging.getLogger("lightning")

    def _resolve(self, name: str, conf):
        """The constructor's value of the option ``name`` or, when that is the off value, ``trainer.<name>`` of the hparams, parsed
        and checked like the constructor's (``TRAINER_OPTIONS``); absent: the off value."""
        off, parse = TRAINER_OPTIONS[name]
        mine = getattr(self, name)
        if mine != off:
            return mine
        value = _hparam(conf, name)
        return off if value is None else parse(value, f"trainer.{name}")

    # (the public face of ``_resolve``: one method per option, each "the constructor's value or ``trainer.<option>`` of the hparams")
    def resolve_gradient_clip_val(self, conf) -> float:
        return self._resolve("gradient_clip_val", conf)

    def resolve_accumulate_grad_batches(self, conf) -> int:
        return self._resolve("accumulate_grad_batches", conf)

    def resolve_weight_ema_decay(self, conf) -> float:
        return self._resolve("weight_ema_decay", conf)

    def resolve_weight_ema_warmup(self, conf) -> float:
        return self._resolve("weight_ema_warmup", conf)

    def resolve_device_scale_jitter(self, conf) -> bool:
        return self._resolve("device_scale_jitter", conf)

    def resolve_image_capacity(self, conf):
        return self._resolve("image_capacity", conf)

    def resolve_predict_image_capacity(self, conf):
        return self._resolve("predict_image_capacity", conf)

    def resolve_device_eval(self, conf) -> bool:
        return self._resolve("device_eval", conf)

    def resolve_device_brightness_contrast(self, conf) -> bool:
        return self._resolve("device_brightness_contrast", conf)

    def _install_brightness_contrast(self, model) -> None:
        """``fit``'s part of ``device_brightness_contrast``: the object ``prepare_data`` mapped from the hparams' ``transforms`` -- or,
        for a csv model that was prepared before the switch was known, the mapping made here."""
        transform = model.net.transform
        if (self.resolve_device_brightness_contrast(model.conf) and getattr(transform, "brightness_contrast", None) is None
                and getattr(getattr(model.conf, "dataset", None), "kind", None) == "csv"):
            from .augment import brightness_contrast_from_transforms
            transform.brightness_contrast = brightness_contrast_from_transforms(model.conf.get("transforms"))
        self.brightness_contrast = getattr(transform, "brightness_contrast", None)

    def _install_scale_jitter(self, model) -> None:
        "``fit``'s part of ``device_scale_jitter``: a ``RandomShortSide`` over the transform's ``min_size`` tuple, or one log line."
        transform = model.net.transform
        self.scale_jitter = getattr(transform, "scale_jitter", None)
        if self.resolve_device_scale_jitter(model.conf):
            sizes = tuple(getattr(transform, "min_size", ()))
            if len(sizes) > 1:
                from .augment import RandomShortSide
                self.scale_jitter = transform.scale_jitter = RandomShortSide(sizes, seed=self.scale_jitter_seed)
            else:
                self.log.info("device_scale_jitter: min_size %s has a single entry, there is nothing to draw: no RandomShortSide installed", sizes)

    def _ema_weights(self, model):
        """The context validation and testing run in: ``model``'s weights exchanged with the average that the last fit() kept, else
        nothing.  A model whose parameters are not the averaged ones is refused (``WeightEMA.swap``): it would be evaluated on its raw
        weights while another model's were swapped."""
        import contextlib
        ema = self.weight_ema
        return ema.swapped(model.net.parameters()) if ema is not None and ema.ready else contextlib.nullcontext()

    def _autocast(self):
        return torch.autocast("cuda", dtype=self.amp_dtype, enabled=self.amp_dtype is not None and self.device.type == "cuda")

    def fit(self, model: RetinaNetModel):
        import torch.distributed as dist
        from .parallel import BucketedGradAllReduce
        if self.resolve_device_brightness_contrast(model.conf):
            model.device_brightness_contrast = True       # (prepare_data maps the RandomBrightnessContrast entry and does not warn about it)
        model.prepare_data() if model.trn_ds is None else None
        model.to(self.device)
        if self.channels_last:
            model.to(memory_format=torch.channels_last)
        model.working_dtype = self.amp_dtype
        opt = model.configure_optimizers()
        optimizers, schedulers = (opt if isinstance(opt, tuple) else (opt, []))
        optimizer = optimizers[0]
        n_acc = self.resolve_accumulate_grad_batches(model.conf)
        if n_acc > 1 and dist.is_available() and dist.is_initialized():
            raise ValueError(f"accumulate_grad_batches={n_acc} under torch.distributed is not supported: gradient accumulation is "
                             "single-process only (skipping the exchange on micro steps is not implemented)")
        ddp = BucketedGradAllReduce(model.net) if dist.is_available() and dist.is_initialized() else None
        self._install_scale_jitter(model)
        self._install_brightness_contrast(model)
        if ddp is not None:
            # every installed augmentation draws from seed = its base seed + rank: each rank makes its own flips, scales, factors, windows ...
            model.net.transform.set_rank(dist.get_rank())
        # precision "16" = fp16 autocast WITH dynamic loss scaling, like the reference's native-AMP run (Lightning precision=16):
        # fp16 gradients of a focal loss normalised by num_fg underflow without it
        # (under a gradient exchange: parallel.ExchangeGradScaler -- found_inf from the exchanged buckets, one decision for all ranks)
        from .parallel import ExchangeGradScaler
        # gradient accumulation: fp32 accumulators on the device for the master optimizers, .grad for everything else
        device_acc = (n_acc > 1 and self.device.type == "cuda" and getattr(optimizer, "_rn_master_weights", False)
                      and type(model).training_step is RetinaNetModel.training_step)
        self.grad_accumulator = None
        if device_acc:
            from .optim import GradAccumulator
            self.grad_accumulator = GradAccumulator(n_acc)
        # (the accumulator hands found_inf of the whole window to the scaler: ExchangeGradScaler.step_exchanged takes it)
        scaler = (ExchangeGradScaler("cuda") if ddp is not None or device_acc else torch.amp.GradScaler("cuda")) \
            if (self.amp_dtype == torch.float16 and self.device.type == "cuda") else None
        # gradient clipping: on the device inside the step for the master optimizers, torch's clip_grad_norm_ for the others
        clip_val = self.resolve_gradient_clip_val(model.conf)
        torch_clip = False
        self.grad_clip = getattr(optimizer, "grad_clip", None) if getattr(optimizer, "_rn_grad_clip", False) else None
        if clip_val > 0:
            if getattr(optimizer, "_rn_grad_clip", False):
                from .optim import GradClip
                if self.grad_clip is None:
                    self.grad_clip = optimizer.grad_clip = GradClip(clip_val)
                else:
                    self.grad_clip.max_norm = clip_val        # (the trainer's value wins over the optimizer's max_grad_norm)
            elif ddp is not None:
                raise RuntimeError(f"gradient_clip_val={clip_val} with {type(optimizer).__name__} under torch.distributed is not supported: "
                                   "the clip has to see the exchanged gradients, which only the master optimizers read "
                                   "(optimizer.class_name: pytorch_retinanet_amd.optim.MasterSGD / MasterAdam / MasterAdamW)")
            else:
                torch_clip = True
                if self.capture:
                    self.log.info("gradient_clip_val=%g with %s: torch.nn.utils.clip_grad_norm_ runs eagerly, the step is not captured "
                                  "(the master optimizers clip inside the captured step)", clip_val, type(optimizer).__name__)
        # the weight average: on the device inside optimizer.step for the master optimizers, nothing else
        ema_decay, ema_warmup = self.resolve_weight_ema_decay(model.conf), self.resolve_weight_ema_warmup(model.conf)
        self.weight_ema = getattr(optimizer, "weight_ema", None) if getattr(optimizer, "_rn_weight_ema", False) else None
        if ema_decay > 0:
            if not (getattr(optimizer, "_rn_weight_ema", False) and self.device.type == "cuda"):
                raise ValueError(f"weight_ema_decay={ema_decay} with {type(optimizer).__name__} on {self.device.type} is not supported: the "
                                 "average is kept on the GPU inside the step of the master optimizers, and there is no CPU fallback "
                                 "(optimizer.class_name: pytorch_retinanet_amd.optim.MasterSGD / MasterAdam / MasterAdamW, on CUDA)")
            from .optim import WeightEMA
            if self.weight_ema is None:
                self.weight_ema = optimizer.weight_ema = WeightEMA(ema_decay, ema_warmup)
            else:
                self.weight_ema.decay, self.weight_ema.warmup = ema_decay, ema_warmup      # (the trainer's values win)
        grad_norm = None
        stepper = None
        capturable = (self.capture and not torch_clip and (n_acc == 1 or device_acc) and self.device.type == "cuda" and ddp is None
                      and type(model).training_step is RetinaNetModel.training_step
                      and (getattr(optimizer, "_rn_device_hparams", False)
                           or not any(s["interval"] == "step" and "monitor" not in s for s in schedulers)))
        if capturable or device_acc:
            from .graph import CapturedTrainStep
            # (device accumulation without capture: the same step object runs eagerly, so the gradients are still summed in fp32)
            stepper = CapturedTrainStep(model.net, optimizer, None, amp_dtype=self.amp_dtype, scaler=scaler, gt_capacity=self.gt_capacity,
                                        accumulate=self.grad_accumulator, enabled=bool(capturable),
                                        image_capacity=self.resolve_image_capacity(model.conf))
        step = 0
        for epoch in range(self.max_epochs):
            model.train()
            loader = model.train_dataloader()
            if hasattr(getattr(loader, "sampler", None), "set_epoch"):
                loader.sampler.set_epoch(epoch)
            for i, batch, last in (_with_last(loader) if n_acc > 1 else ((j, b, False) for j, b in enumerate(loader))):
                batch = _to_device(batch, self.device)
                # accumulation windows restart with every epoch and the last batch of an epoch always steps (Lightning)
                final = n_acc == 1 or (i + 1) % n_acc == 0 or last
                if stepper is not None:
                    # the same step (zero_grad -> autocast forward -> loss = sum of the dict -> backward -> optimizer.step) as ONE graph replay
                    images, targets, _ = batch
                    tgs = [{k: v for k, v in t.items() if isinstance(v, torch.Tensor) and k in ("boxes", "labels")} for t in targets]
                    out = stepper(list(images), tgs, final=final) if device_acc else stepper(list(images), tgs)
                    self.captured_steps, self.captured_graphs = stepper.replays, stepper.captures
                else:
                    # the plain thing: every micro-batch adds (loss / N)'s gradients into .grad; zero at the start of a window, step at
                    # its end (N = 1: every batch is a window)
                    from .graph import apply_gradients
                    from .losses import grad_prescale, scaler_prescale
                    with self._autocast(), grad_prescale(scaler_prescale(scaler, self.device)):
                        out = model.training_step(batch, i)
                    if i % n_acc == 0:
                        ddp.zero_grad() if ddp is not None else optimizer.zero_grad(set_to_none=False)
                    part = out["loss"] / n_acc if n_acc > 1 else out["loss"]      # (N = 1: a division by 1 would be one more launch)
                    (scaler.scale(part) if scaler is not None else part).backward()
                    if final:
                        if ddp is not None:
                            ddp.finish()
                        if torch_clip:
                            if scaler is not None:
                                scaler.unscale_(optimizer)
                            grad_norm = torch.nn.utils.clip_grad_norm_(model.net.parameters(), clip_val)
                        apply_gradients(optimizer, scaler, ddp)       # (a master optimizer: on the fp32 bucket views of the 16-bit working copies)
                if not final:
                    continue                                  # (schedulers, max_steps and the log count optimizer steps)
                step += 1
                if step % self.log_every == 0:
                    if self.grad_clip is not None or grad_norm is not None:
                        norm = float(self.grad_clip.total_norm if self.grad_clip is not None else grad_norm)
                        self.log.info("epoch %d step %d grad_norm %.4f loss %.4f", epoch, step, norm, float(out["loss"]))
                    else:
                        self.log.info("epoch %d step %d loss %.4f", epoch, step, float(out["loss"]))
                for s in schedulers:
                    if s["interval"] == "step" and "monitor" not in s:
                        s["scheduler"].step()
                if self.max_steps and step >= self.max_steps:
                    return step
            val = self._validate(model)
            for s in schedulers:
                if s["interval"] == "epoch":
                    s["scheduler"].step(val) if "monitor" in s and val is not None else (None if "monitor" in s else s["scheduler"].step())
        return step

    def _validate(self, model):
        loader = model.val_dataloader()
        if loader is None:
            return None
        import torch.distributed as dist
        tot, n = 0.0, 0
        was_training = model.training
        model.eval()                      # Lightning validates in eval mode: BN uses (and does not update) running statistics
        try:
            with torch.no_grad(), self._ema_weights(model):            # (the swap is undone when validation raises, too)
                for i, batch in enumerate(loader):
                    with self._autocast():
                        out = model.validation_step(_to_device(batch, self.device), i)
                    tot, n = tot + float(out["val_loss"]), n + 1
        finally:
            model.train(was_training)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            t = torch.tensor([tot, float(n)], dtype=torch.float64, device=self.device)
            dist.all_reduce(t)            # every rank steps its ReduceLROnPlateau with the same number
            tot, n = float(t[0]), int(t[1])
        return tot / max(n, 1)

    def test(self, model: RetinaNetModel):
        model.to(self.device).eval()
        outs = []
        capacity = self.resolve_predict_image_capacity(getattr(model, "conf", None))
        installed = False
        if self.resolve_device_eval(getattr(model, "conf", None)):
            model.device_eval = True                      # (test_dataloader below builds the evaluator on the model's device)
        if capacity is not None and self.device.type == "cuda" and getattr(model, "predictor", None) is None:
            from .graph import CapturedPredict
            # (inside the swap below: the predictor stamps the weights it captured under, so the swap and its undoing drop its graphs)
            self.predictor = model.predictor = CapturedPredict(model.net, capacity, amp_dtype=self.amp_dtype)
            installed = True
        try:
            with torch.no_grad(), self._ema_weights(model):
                for i, batch in enumerate(model.test_dataloader()):
                    with self._autocast():
                        outs.append(model.test_step(_to_device(batch, self.device), i))
        finally:
            if installed:
                model.predictor = None
        return model.test_epoch_end(outs), outs
