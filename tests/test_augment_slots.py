"""CPU suite: the tables behind the train-time augmentations -- ``transform.AUGMENT_SLOTS`` (the slots of ``GeneralizedRCNNTransform``:
who acts, in which order, one stream per rank), the key ``graph.CapturedTrainStep._signature`` builds from them, element for element,
``model.TRAINER_OPTIONS`` (the trainer options the hparams may also set) and ``augment.SLOT_MAPPERS`` (who maps which entry of the
hparams' ``transforms``).  Tiny nets, no GPU."""
import pytest
import torch

from pytorch_retinanet_amd.augment import (SLOT_MAPPERS, BBoxSafeRandomCrop, ColorJitter, RandomBrightnessContrast, RandomHorizontalFlip,
                                           RandomShortSide, ShiftScaleRotate, from_transforms)
from pytorch_retinanet_amd.model import TRAINER_OPTIONS
from pytorch_retinanet_amd.transform import AUGMENT_SLOTS, GeneralizedRCNNTransform, augments_of

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
SIZES, MAX_SIZE = (24, 32), 48

# slot -> an object for it from a seed; equal arguments give equal-valued but distinct objects
MAKE = {
    "hflip": lambda seed=0: RandomHorizontalFlip(p=0.5, seed=seed),
    "scale_jitter": lambda seed=0: RandomShortSide(SIZES, seed=seed),
    "color_jitter": lambda seed=0: ColorJitter(0.4, 0.4, 0.4, 0.1, p=0.5, seed=seed),
    "crop": lambda seed=0: BBoxSafeRandomCrop(p=0.5, seed=seed),
    "shift_scale_rotate": lambda seed=0: ShiftScaleRotate(p=0.5, seed=seed),
    "brightness_contrast": lambda seed=0: RandomBrightnessContrast(p=0.5, seed=seed),
}
# the order in which one training call of the PyTorch path draws (transform.py's module docstring): crop and shift / scale / rotate
# first, then the flip, the colour jitter, brightness / contrast and the short side
DRAW_ORDER = ("crop", "shift_scale_rotate", "hflip", "color_jitter", "brightness_contrast", "scale_jitter")


def test_the_tables_name_the_same_slots():
    assert set(MAKE) == set(AUGMENT_SLOTS) == set(DRAW_ORDER) and len(set(AUGMENT_SLOTS)) == len(AUGMENT_SLOTS)
    # every slot an hparams entry can fill has one mapper: the flip's is from_transforms, the short side comes from min_size
    assert {slot for slot, _, _ in SLOT_MAPPERS} | {"hflip", "scale_jitter"} == set(AUGMENT_SLOTS)
    tr = GeneralizedRCNNTransform(SIZES, MAX_SIZE, MEAN, STD)
    assert all(getattr(tr, name) is None for name in AUGMENT_SLOTS) and tr.augments() == [] and augments_of(None) == []
    objs = {name: MAKE[name]() for name in AUGMENT_SLOTS}
    for name in reversed(AUGMENT_SLOTS):                                   # (installed in another order: the table's order comes back)
        setattr(tr, name, objs[name])
    assert tr.augments() == [(name, objs[name]) for name in AUGMENT_SLOTS] == augments_of(tr)


# ---- the graph key --------------------------------------------------------------------------------------------------------
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 4, 1)
        self.transform = GeneralizedRCNNTransform(SIZES, MAX_SIZE, MEAN, STD)


def _batch():
    return [torch.zeros(3, 16, 16)], [{"boxes": torch.zeros(2, 4), "labels": torch.zeros(2, dtype=torch.int64)}]


def _base_key(hflip=None):
    "The eight base elements of the key of ``_Net`` + ``MasterSGD(lr=1e-2, momentum=0.9)`` + ``_batch()`` in fp32, written out."
    cpu = torch.device("cpu")
    return ((((3, 16, 16), torch.float32, cpu),),                                                       # 0: the images
            ((("boxes", (2, 4), torch.float32), ("labels", (2,), torch.int64)),),                        # 1: the targets
            ((1e-2, 0.9, 0.0, 0.0, False),),                                                             # 2: lr, momentum, weight decay, dampening, nesterov
            hash((True, True, True)),                                                                    # 3: net, conv, transform in training mode
            hash((True, True)),                                                                          # 4: weight and bias take gradients
            None,                                                                                        # 5: no autocast
            hflip,                                                                                       # 6: the flip, None without one
            None)                                                                                        # 7: no clip


def _stepper(accumulate=None):
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from pytorch_retinanet_amd.optim import MasterSGD
    net = _Net()
    opt = MasterSGD(net.parameters(), lr=1e-2, momentum=0.9)
    return net, opt, CapturedTrainStep(net, opt, amp_dtype=None, enabled=False, accumulate=accumulate)


def test_the_key_is_element_for_element_what_it_was():
    from pytorch_retinanet_amd.optim import GradAccumulator, WeightEMA
    images, targets = _batch()
    net, opt, step = _stepper()
    assert step._signature(images, targets) == _base_key()
    acc, ema = GradAccumulator(2), WeightEMA(0.9)
    net, opt, step = _stepper(accumulate=acc)
    opt.weight_ema = ema
    objs = {name: MAKE[name]() for name in AUGMENT_SLOTS}
    for name, obj in objs.items():
        setattr(net.transform, name, obj)
    key = step._signature(images, targets)
    want = _base_key(objs["hflip"]) + (acc, ("weight_ema", ema), ("scale_jitter", objs["scale_jitter"]), ("color_jitter", objs["color_jitter"]),
                                      ("crop", objs["crop"]), ("shift_scale_rotate", objs["shift_scale_rotate"]),
                                      ("brightness_contrast", objs["brightness_contrast"]))
    assert key == want and len(key) == 15
    assert key[6] is objs["hflip"] and key[8] is acc and key[9][1] is ema and all(key[10 + i][1] is objs[name] for i, name in enumerate(AUGMENT_SLOTS[1:]))


def _set_setting(name, obj):
    if name == "scale_jitter":
        obj.sizes = (24,)
    else:
        obj.p = 0.25
    if name == "shift_scale_rotate":
        obj.set_limits(rotate_limit=10)
    if name == "brightness_contrast":
        obj.set_limits(brightness_limit=0.1)
    obj.reseed(11)


@pytest.mark.parametrize("name", AUGMENT_SLOTS)
def test_the_key_holds_the_installed_object_of_every_slot(name):
    images, targets = _batch()
    net, opt, step = _stepper()
    plain = step._signature(images, targets)
    assert plain == _base_key()
    a, b = MAKE[name](), MAKE[name]()
    setattr(net.transform, name, a)
    with_a = step._signature(images, targets)
    assert with_a != plain                                                 # installing changes the key
    _set_setting(name, a)
    assert step._signature(images, targets) == with_a                      # a setting of the installed object does not
    setattr(net.transform, name, b)
    assert step._signature(images, targets) != with_a                      # an equal-valued NEW object does
    setattr(net.transform, name, None)
    assert step._signature(images, targets) == plain                       # removing it restores the plain key
    # a transform unpickled from before the slot existed has no such attribute: the plain key, and a forward that works
    delattr(net.transform, name)
    assert not hasattr(net.transform, name)
    assert step._signature(images, targets) == plain
    net.transform.train()
    ims = [torch.rand(3, 20, 30), torch.rand(3, 28, 24)]
    tgs = [{"boxes": torch.tensor([[2., 3., 12., 14.]]), "labels": torch.tensor([1])},
           {"boxes": torch.tensor([[1., 1., 9., 20.], [5., 6., 20., 25.]]), "labels": torch.tensor([2, 3])}]
    out, out_t = net.transform(ims, tgs)
    assert out.tensors.shape[0] == 2 and [tuple(t["boxes"].shape) for t in out_t] == [(1, 4), (2, 4)]
    net.transform.set_rank(1)                                              # (and nothing to seed there)
    out, _ = net.transform.eval()(ims)
    assert out.tensors.shape[0] == 2


# ---- one stream per rank --------------------------------------------------------------------------------------------------
_IN_HW = [(20, 30), (28, 24)]
_BOXES = [torch.tensor([[2., 3., 12., 14.]]), torch.tensor([[1., 1., 9., 20.], [5., 6., 20., 25.]])]
HOST_DRAW = {
    "hflip": lambda o: o.next_flags(2, torch.device("cpu")),
    "scale_jitter": lambda o: o.next_sizes(_IN_HW, MAX_SIZE, torch.device("cpu")),
    "color_jitter": lambda o: o.next_draw(2),
    "crop": lambda o: o.next_rects(_IN_HW, _BOXES),
    "shift_scale_rotate": lambda o: o.next_coefs(_IN_HW, _BOXES),
    "brightness_contrast": lambda o: o.next_draw(2),
}


def test_set_rank_seeds_every_installed_object_and_keeps_its_counter():
    tr = GeneralizedRCNNTransform(SIZES, MAX_SIZE, MEAN, STD)
    objs = {name: MAKE[name](seed=100 + 10 * i) for i, name in enumerate(AUGMENT_SLOTS)}
    for i, (name, obj) in enumerate(objs.items()):
        setattr(tr, name, obj)
        for _ in range(i + 1):
            HOST_DRAW[name](obj)
    assert [o.counter for o in objs.values()] == [1, 2, 3, 4, 5, 6]
    tr.set_rank(3)
    for i, (name, obj) in enumerate(objs.items()):
        assert obj.base_seed == 100 + 10 * i and obj.seed == obj.base_seed + 3 and obj.counter == i + 1, name
    # only two installed: the other slots are skipped
    tr = GeneralizedRCNNTransform(SIZES, MAX_SIZE, MEAN, STD)
    tr.crop, tr.color_jitter = MAKE["crop"](seed=7), MAKE["color_jitter"](seed=9)
    tr.set_rank(2)
    assert (tr.crop.seed, tr.color_jitter.seed) == (9, 11) and tr.augments() == [("color_jitter", tr.color_jitter), ("crop", tr.crop)]


# ---- who draws, and in which order ----------------------------------------------------------------------------------------
def _recording(tr):
    "Every slot filled, each object's host draw wrapped to note the slot's name first."
    order, objs = [], {}
    for name in AUGMENT_SLOTS:
        obj = objs[name] = MAKE[name](seed=3)
        setattr(tr, name, obj)

        def noted(draw, name=name, inner=obj._host_draw):
            order.append(name)
            return inner(draw)
        obj._host_draw = noted
    return order, objs


def _cpu_batch():
    ims = [torch.rand(3, 20, 30), torch.rand(3, 28, 24)]
    tgs = [{"boxes": _BOXES[0].clone(), "labels": torch.tensor([1])}, {"boxes": _BOXES[1].clone(), "labels": torch.tensor([2, 3])}]
    return ims, tgs


def test_the_pytorch_path_draws_once_per_slot_in_the_order_it_always_did():
    tr = GeneralizedRCNNTransform(SIZES, MAX_SIZE, MEAN, STD).train()
    order, objs = _recording(tr)
    ims, tgs = _cpu_batch()
    out, out_t = tr(ims, tgs)
    assert tuple(order) == DRAW_ORDER
    assert {name: o.counter for name, o in objs.items()} == {name: 1 for name in AUGMENT_SLOTS}
    assert out.tensors.shape[0] == 2 and len(out_t) == 2
    tr(ims, tgs)
    assert tuple(order) == DRAW_ORDER * 2 and all(o.counter == 2 for o in objs.values())


@pytest.mark.parametrize("training, with_targets", [(False, True), (False, False), (True, False)])
def test_no_slot_draws_in_eval_mode_or_without_targets(training, with_targets):
    tr = GeneralizedRCNNTransform(SIZES, MAX_SIZE, MEAN, STD).train(training)
    order, objs = _recording(tr)
    ims, tgs = _cpu_batch()
    tr(ims, tgs if with_targets else None)
    assert order == [] and all(o.counter == 0 for o in objs.values())


# ---- the trainer's options ------------------------------------------------------------------------------------------------
# option -> (a constructor value, an hparams value, what the hparams value resolves to, an invalid value or None)
OPTION_CASES = {
    "gradient_clip_val": (0.5, 0.25, 0.25, -1.0),
    "accumulate_grad_batches": (4, 2, 2, 0),
    "weight_ema_decay": (0.9, 0.99, 0.99, 1.0),
    "weight_ema_warmup": (10.0, 5, 5.0, float("inf")),
    "device_scale_jitter": (True, True, True, None),
    "image_capacity": ([(96, 128)], [[96, 128], [128.0, 96]], [(96, 128), (128, 96)], [(96, 128, 3)]),
    "predict_image_capacity": ([(160, 160)], [[800, 1344], [1344, 800]], [(800, 1344), (1344, 800)], [(0, 160)]),
    "device_eval": (True, True, True, None),
    "device_brightness_contrast": (True, True, True, None),
}
# the options whose ValueError starts with the option's label (the canvases' comes from graph.image_capacity_classes: "image_capacity: ...")
LABELLED = ("gradient_clip_val", "accumulate_grad_batches", "weight_ema_decay", "weight_ema_warmup")


def _trainer(**kw):
    import pytorch_retinanet_amd as P
    return P.SimpleTrainer(device="cpu", gt_capacity="auto", **kw)


def test_every_option_of_the_table_has_a_case_and_a_public_resolver():
    assert set(OPTION_CASES) == set(TRAINER_OPTIONS)
    t = _trainer()
    for name, (off, _) in TRAINER_OPTIONS.items():
        assert getattr(t, name) == off and type(getattr(t, name)) is type(off), name
        assert getattr(t, f"resolve_{name}")({"trainer": {}}) == off, name


@pytest.mark.parametrize("name", list(TRAINER_OPTIONS))
def test_trainer_option_constructor_then_hparams_then_off(name):
    off, _ = TRAINER_OPTIONS[name]
    mine, raw, resolved, bad = OPTION_CASES[name]
    resolve = lambda t, conf: getattr(t, f"resolve_{name}")(conf)
    conf = {"trainer": {name: raw}}
    assert resolve(_trainer(**{name: mine}), conf) == mine                 # the constructor's value wins
    got = resolve(_trainer(), conf)                                        # left at the off value: the hparams' value
    assert got == resolved and type(got) is type(resolved)
    for absent in (None, {}, {"trainer": None}, {"trainer": {}}, {"trainer": {"another_key": 1}}):
        assert resolve(_trainer(), absent) == off                          # no section, no key: off
        assert resolve(_trainer(**{name: mine}), absent) == mine
    if name in ("image_capacity", "predict_image_capacity"):
        assert all(type(c) is tuple and all(type(v) is int for v in c) for c in got)      # YAML's lists of lists: tuples of ints
    if bad is None:
        return
    starts = (lambda label: rf"^{label.replace('.', chr(92) + '.')}\b") if name in LABELLED else (lambda label: "image_capacity")
    with pytest.raises(ValueError, match=starts(name)):
        _trainer(**{name: bad})
    with pytest.raises(ValueError, match=starts(f"trainer.{name}")):
        resolve(_trainer(), {"trainer": {name: bad}})


# ---- the mappers' registry ------------------------------------------------------------------------------------------------
class _ListLog:
    def __init__(self):
        self.lines = []

    def warning(self, fmt, *args):
        self.lines.append(fmt % args)


@pytest.mark.parametrize("bc_on", [True, False])
def test_only_an_unknown_entry_is_called_unsupported(bc_on):
    owned = [name for _, names, _ in SLOT_MAPPERS for name in names]
    assert len(owned) == len(set(owned)) >= 9
    entries = [{"class_name": "albumentations.HorizontalFlip", "params": {"p": 0.5}}] + [{"class_name": n} for n in owned] \
        + [{"class_name": "albumentations.GaussNoise", "params": {"p": 0.2}}]
    log = _ListLog()
    flip = from_transforms(entries, log=log, brightness_contrast=bc_on)
    assert isinstance(flip, RandomHorizontalFlip)
    unsupported = [line for line in log.lines if "not supported" in line]
    assert len(unsupported) == 1 and "albumentations.GaussNoise" in unsupported[0]
    # (without the switch the brightness / contrast entries are named as skipped-but-implemented, which is another warning)
    assert len(log.lines) == (1 if bc_on else 3)
    # and every owned name is mapped by its slot's mapper
    for slot, names, mapper in SLOT_MAPPERS:
        for n in names:
            assert type(mapper([{"class_name": n}])) is type(MAKE[slot]()), (slot, n)
