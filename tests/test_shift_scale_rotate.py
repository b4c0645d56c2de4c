"""CPU: shift / scale / rotate (``augment.ShiftScaleRotate``) -- properties of the Python restatement of ``rn_affine_draw`` and
``rn_image_warp_stage`` that follow from the rule alone (the identity, a pure half-image shift, a half turn, boxes inside the image,
labels following their boxes), the constructor, the hparams mapping, ``CapturedTrainStep``'s refusal without capacities and the
host path of the transform.

``SIZES`` / ``gt_boxes()`` / ``images()`` are the batch ``tests/test_shift_scale_rotate_gpu.py`` runs on the device as well."""
import logging
import types

import numpy as np
import pytest
import torch

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
SIZES = [(37, 53), (64, 40), (1, 1), (1, 9), (16, 16)]            # odd, w % 4 == 0, one pixel, one row, no boxes


def gt_boxes():
    "Per image of ``SIZES``: four boxes, the second a small one in a corner (a rotation drops it); three, likewise; one covering the pixel; one; none."
    return [torch.tensor([[3.5, 4.0, 20.0, 30.0], [49.0, 1.0, 52.5, 4.0], [10.0, 2.0, 40.25, 12.0], [30.0, 20.0, 44.0, 31.5]]),
            torch.tensor([[5.0, 6.0, 20.0, 50.0], [36.0, 0.5, 39.5, 3.0], [22.0, 30.0, 38.5, 61.0]]),
            torch.tensor([[0.0, 0.0, 1.0, 1.0]]),
            torch.tensor([[2.0, 0.0, 7.0, 1.0]]),
            torch.zeros((0, 4))]


def gt_labels():
    return [torch.tensor([1, 2, 3, 4]), torch.tensor([4, 1, 5]), torch.tensor([2]), torch.tensor([3]), torch.zeros((0,), dtype=torch.int64)]


def images(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand((3, h, w), generator=g) for h, w in SIZES]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _refl(i, n):
    "reflect-101 by walking, independent of the restatement's closed form"
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * (n - 1) - i
    return i


# ---- 1. the restatement ---------------------------------------------------------------------------------------------------
def test_p_zero_is_the_identity():
    from pytorch_retinanet_amd.augment import ShiftScaleRotate
    ssr = ShiftScaleRotate(p=0.0, seed=3)
    ims, boxes, labels = images(), gt_boxes(), gt_labels()
    for k in range(3):
        c = ssr.draw(k, SIZES, boxes)
        assert c.applied == [False] * 5
        assert np.array_equal(c.m, np.tile(np.float32([1, 0, 0, 0, 1, 0]), (5, 1))) and np.array_equal(c.inv, c.m)
        for b, (bx, lb) in enumerate(ShiftScaleRotate.warp_boxes(c, SIZES, boxes, labels)):
            assert torch.equal(_bits(bx), _bits(boxes[b])) and torch.equal(lb, labels[b])
            assert ShiftScaleRotate.warp_image(ims[b], c.inv[b], c.applied[b]) is ims[b]


def test_a_pure_half_image_shift_moves_pixels_by_reflection_and_drops_exactly_the_boxes_that_leave():
    from pytorch_retinanet_amd.augment import ShiftScaleRotate
    h, w = 12, 20
    g = torch.Generator().manual_seed(1)
    img = torch.rand((3, h, w), generator=g)
    boxes = torch.tensor([[1.0, 1.0, 6.0, 4.0],          # stays: shifted whole
                          [8.0, 2.0, 15.0, 5.5],         # stays: clipped on the right
                          [10.0, 1.0, 14.0, 3.0],        # x1 >= w / 2: dropped
                          [2.0, 6.0, 5.0, 9.0],          # y1 >= h / 2: dropped
                          [9.5, 5.5, 19.0, 11.0],        # stays: clipped on both
                          [12.0, 7.0, 18.0, 10.0]])      # both: dropped
    labels = torch.tensor([5, 6, 7, 8, 9, 10])
    ssr = ShiftScaleRotate(shift_limit=(0.5, 0.5), scale_limit=0.0, rotate_limit=0, p=1.0, seed=2)
    c = ssr.draw(0, [(h, w)], [boxes])
    assert c.applied == [True]
    assert np.array_equal(c.m[0], np.float32([1, 0, w / 2, 0, 1, h / 2])) and np.array_equal(c.inv[0], np.float32([1, 0, -w / 2, 0, 1, -h / 2]))
    got = ShiftScaleRotate.warp_image(img, c.inv[0])
    want = torch.stack([torch.stack([img[:, _refl(y - h // 2, h), _refl(x - w // 2, w)] for x in range(w)], 1) for y in range(h)], 1)
    assert torch.equal(_bits(got), _bits(want))
    (bx, lb), = ShiftScaleRotate.warp_boxes(c, [(h, w)], [boxes], [labels])
    keep = ~((boxes[:, 0] >= w / 2) | (boxes[:, 1] >= h / 2))
    assert keep.tolist() == [True, True, False, False, True, False]
    moved = boxes[keep] + torch.tensor([w / 2, h / 2, w / 2, h / 2])
    moved[:, 0::2].clamp_(0, w), moved[:, 1::2].clamp_(0, h)
    assert torch.equal(bx, moved) and lb.tolist() == [5, 6, 9]


def test_an_image_whose_boxes_would_all_drop_is_left_alone():
    from pytorch_retinanet_amd.augment import ShiftScaleRotate
    h, w = 12, 20
    boxes = [torch.tensor([[10.0, 1.0, 14.0, 3.0], [12.0, 7.0, 18.0, 10.0]]), torch.tensor([[1.0, 1.0, 6.0, 4.0]]), torch.zeros((0, 4))]
    ssr = ShiftScaleRotate(shift_limit=(0.5, 0.5), scale_limit=0.0, rotate_limit=0, p=1.0, seed=2)
    c = ssr.draw(0, [(h, w)] * 3, boxes)
    assert c.applied == [False, True, True]                            # (an image WITHOUT rows is warped)
    assert np.array_equal(c.m[0], np.float32([1, 0, 0, 0, 1, 0])) and np.array_equal(c.inv[0], c.m[0])
    out = ShiftScaleRotate.warp_boxes(c, [(h, w)] * 3, boxes)
    assert torch.equal(_bits(out[0][0]), _bits(boxes[0])) and out[2][0].shape == (0, 4)
    # min_visibility: the box that is clipped to less than half of its area goes, and with it the image's only row
    half = ShiftScaleRotate(shift_limit=(0.5, 0.5), scale_limit=0.0, rotate_limit=0, p=1.0, min_visibility=0.5, seed=2)
    edge = [torch.tensor([[8.0, 2.0, 15.0, 5.5]])]                     # 2 of its 7 columns stay
    assert ssr.draw(0, [(h, w)], edge).applied == [True] and half.draw(0, [(h, w)], edge).applied == [False]


def test_a_half_turn_flips_both_axes():
    from pytorch_retinanet_amd.augment import ShiftScaleRotate
    ssr = ShiftScaleRotate(shift_limit=0.0, scale_limit=0.0, rotate_limit=(180, 180), p=1.0, seed=4)
    ims = images(seed=5)
    c = ssr.draw(0, SIZES, [None] * 5)
    assert c.applied == [True] * 5
    for b, im in enumerate(ims):
        assert torch.equal(_bits(ShiftScaleRotate.warp_image(im, c.inv[b])), _bits(torch.flip(im, [1, 2]))), b


def test_kept_boxes_lie_inside_the_image_with_positive_area_and_labels_follow_their_boxes():
    from pytorch_retinanet_amd.augment import ShiftScaleRotate
    rng = np.random.default_rng(0)
    h, w = 48, 64
    T = 12
    x1, y1 = rng.uniform(-4, w - 2, T), rng.uniform(-4, h - 2, T)
    boxes = torch.from_numpy(np.stack([x1, y1, x1 + rng.uniform(1, 30, T), y1 + rng.uniform(1, 30, T)], 1).astype(np.float32))
    labels = torch.arange(100, 100 + T)
    ssr = ShiftScaleRotate(shift_limit=0.3, scale_limit=0.4, rotate_limit=90, p=1.0, min_visibility=0.3, seed=7)
    dropped = applied = 0
    for k in range(40):
        c = ssr.draw(k, [(h, w)], [boxes])
        (bx, lb), = ShiftScaleRotate.warp_boxes(c, [(h, w)], [boxes], [labels], 0.3)
        if not c.applied[0]:
            assert torch.equal(bx, boxes)
            continue
        applied += 1
        dropped += T - bx.shape[0]
        assert bx.shape[0] >= 1 and bool((bx[:, 0] >= 0).all() and (bx[:, 1] >= 0).all() and (bx[:, 2] <= w).all() and (bx[:, 3] <= h).all())
        assert bool((bx[:, 2] > bx[:, 0]).all() and (bx[:, 3] > bx[:, 1]).all())
        # labels follow their boxes: warp each row alone and find it again, in order
        alone = [ShiftScaleRotate.warp_boxes(c, [(h, w)], [boxes[r:r + 1]], [labels[r:r + 1]], 0.3)[0] for r in range(T)]
        want = [(a[0][0], int(a[1][0])) for a in alone if a[0].shape[0]]
        assert [int(v) for v in lb] == [l for _, l in want] and torch.equal(bx, torch.stack([b for b, _ in want]))
    assert applied >= 30 and dropped >= 20
    # the inverse matrix undoes the forward one (float64 product of the fp32 entries)
    m, inv = c.m[0].astype(np.float64), c.inv[0].astype(np.float64)
    A, Ai = np.vstack([m.reshape(2, 3), [0, 0, 1]]), np.vstack([inv.reshape(2, 3), [0, 0, 1]])
    assert np.allclose(A @ Ai, np.eye(3), atol=1e-4)


def test_the_salts_are_new():
    import os
    import re
    from pytorch_retinanet_amd import augment
    mine = [augment.AFFINE_SALT_APPLY, augment.AFFINE_SALT_ANGLE, augment.AFFINE_SALT_SCALE, augment.AFFINE_SALT_DX, augment.AFFINE_SALT_DY]
    assert all(s % 2 == 1 and 0 < s < 2 ** 64 for s in mine)
    header = open(os.path.join(os.path.dirname(augment.__file__), "..", "include", "retinanet_hip.h")).read()
    every = re.findall(r"0x[0-9A-Fa-f]{16}", header)
    for s in mine:
        assert every.count("0x%016X" % s) == 1
    other = [augment.SHORT_SIDE_SALT, augment.COLOR_SALT_APPLY, augment.COLOR_SALT_ORDER, *augment.COLOR_SALT_FACTOR, augment.CROP_SALT_APPLY,
             augment.CROP_SALT_LEFT, augment.CROP_SALT_TOP, augment.CROP_SALT_RIGHT, augment.CROP_SALT_BOTTOM, 0]
    assert len(set(mine + other)) == len(mine) + len(other)


# ---- 2. the object ------------------------------------------------------------------------------------------------------------
def test_constructor_validation_and_ranges():
    from pytorch_retinanet_amd.augment import ShiftScaleRotate
    d = ShiftScaleRotate()
    f = lambda v: float(np.float32(v))
    assert d.p == 0.5 and d.min_visibility == 0.0 and d.seed == 0
    assert d.ranges == ((-45.0, f(0.9), f(-0.0625), f(-0.0625)), (45.0, f(1.1), f(0.0625), f(0.0625)))
    pair = ShiftScaleRotate(shift_limit=(0.1, 0.2), scale_limit=(-0.5, 0.25), rotate_limit=(10, 30))
    assert pair.ranges == ((10.0, 0.5, f(0.1), f(0.1)), (30.0, 1.25, f(0.2), f(0.2)))
    for bad in (1.0, 1.5, (-1.0, 0.0), (-2.0, 3.0)):
        with pytest.raises(ValueError, match="scale"):
            ShiftScaleRotate(scale_limit=bad)
    for kw in ({"p": 1.5}, {"p": -0.1}, {"min_visibility": 1.5}, {"min_visibility": -0.5}, {"shift_limit": (1, 2, 3)}, {"rotate_limit": float("inf")}):
        with pytest.raises(ValueError):
            ShiftScaleRotate(**kw)
    with pytest.raises(RuntimeError, match="GPU"):
        d.device_block("cpu")


def test_two_objects_with_one_seed_agree_and_the_state_round_trips():
    from pytorch_retinanet_amd.augment import ShiftScaleRotate
    boxes = gt_boxes()
    a, b = ShiftScaleRotate(p=0.75, seed=11), ShiftScaleRotate(p=0.75, seed=11)
    seen = set()
    for k in range(4):
        ca, cb = a.next_coefs(SIZES, boxes), b.next_coefs(SIZES, boxes)
        assert np.array_equal(ca.m, cb.m) and np.array_equal(ca.inv, cb.inv) and ca.applied == cb.applied
        assert np.array_equal(ca.m, a.draw(k, SIZES, boxes).m) and a.counter == k + 1 and a.coefs is ca
        seen.add(ca.m.tobytes())
    assert len(seen) == 4 and not np.array_equal(ShiftScaleRotate(p=0.75, seed=12).draw(0, SIZES, boxes).m, a.draw(0, SIZES, boxes).m)
    state = a.state_dict()
    assert state == {"seed": 11, "counter": 4, "p": 0.75}
    c = ShiftScaleRotate(seed=1)
    c.load_state_dict(state)
    assert c.state_dict() == state and np.array_equal(c.next_coefs(SIZES, boxes).m, a.next_coefs(SIZES, boxes).m)
    c.set_rank(2)
    assert c.seed == 3 and c.counter == 5                              # the constructor's seed + rank, the counter kept
    c.set_limits(rotate_limit=0, scale_limit=0.0)
    assert c.ranges[0][:2] == (0.0, 1.0) and c.ranges[1][:2] == (0.0, 1.0) and c.ranges[1][2] == float(np.float32(0.0625))


# ---- 3. hparams ---------------------------------------------------------------------------------------------------------------
def test_hparams_mapping_and_its_warnings(caplog):
    from pytorch_retinanet_amd.augment import ShiftScaleRotate, from_transforms, shift_scale_rotate_from_transforms
    ssr = shift_scale_rotate_from_transforms([{"class_name": "albumentations.ShiftScaleRotate"}], seed=4)
    assert isinstance(ssr, ShiftScaleRotate) and ssr.p == 0.5 and ssr.seed == 4 and ssr.ranges == ShiftScaleRotate().ranges
    demo = [{"class_name": "albumentations.HorizontalFlip", "params": {"p": 0.5}},
            {"class_name": "albumentations.ShiftScaleRotate", "params": {"p": 0.5}},
            {"class_name": "albumentations.RandomBrightnessContrast", "params": {"p": 0.5}}]
    assert shift_scale_rotate_from_transforms(demo).p == 0.5
    ssr = shift_scale_rotate_from_transforms([{"class_name": "ShiftScaleRotate", "params": {"shift_limit": [0.0, 0.1], "scale_limit": 0.2,
                                                                                           "rotate_limit": 10, "p": 0.25, "always_apply": True}}])
    assert ssr.p == 1.0 and ssr.rotate_limit == (-10.0, 10.0) and ssr.shift_limit == (0.0, float(np.float32(0.1)))
    assert shift_scale_rotate_from_transforms(None) is None and shift_scale_rotate_from_transforms(demo[:1]) is None
    for key, value in (("interpolation", 0), ("border_mode", 0), ("value", [0, 0, 0]), ("shift_limit_x", 0.2), ("shift_limit_y", 0.2)):
        caplog.clear()
        with caplog.at_level(logging.WARNING):
            ssr = shift_scale_rotate_from_transforms([{"class_name": "albumentations.ShiftScaleRotate", "params": {key: value}}])
        assert ssr.ranges == ShiftScaleRotate().ranges and sum(key in r.getMessage() for r in caplog.records) == 1, key
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        # the defaults spelled out do not warn, and the flip mapping no longer warns about this entry
        assert shift_scale_rotate_from_transforms([{"class_name": "albumentations.ShiftScaleRotate", "params": {"interpolation": 1, "border_mode": 4}}])
        assert from_transforms(demo[1:2]) is None
        assert not caplog.records
        two = shift_scale_rotate_from_transforms([demo[1], {"class_name": "ShiftScaleRotate", "params": {"p": 0.9}}])
        assert two.p == 0.5 and sum("second" in r.getMessage() for r in caplog.records) == 1
        caplog.clear()
        assert from_transforms(demo) is not None
    msgs = [r.getMessage() for r in caplog.records]
    assert len(msgs) == 1 and "albumentations.RandomBrightnessContrast" in msgs[0] and "skipped" in msgs[0]


def test_prepare_data_installs_it(tmp_path, caplog):
    from pytorch_retinanet_amd.augment import ShiftScaleRotate
    from test_hflip import _model, _png_csv
    path = _png_csv(tmp_path)
    with caplog.at_level(logging.WARNING):
        model = _model("csv", path, [{"class_name": "albumentations.HorizontalFlip", "params": {"p": 0.5}},
                                     {"class_name": "albumentations.ShiftScaleRotate", "params": {"p": 0.3, "rotate_limit": 15}}])
    assert not any("ShiftScaleRotate" in r.getMessage() for r in caplog.records)
    ssr = model.net.transform.shift_scale_rotate
    assert isinstance(ssr, ShiftScaleRotate) and ssr.p == float(np.float32(0.3)) and ssr.rotate_limit == (-15.0, 15.0)
    assert model.net.transform.hflip is not None
    assert _model("csv", path).net.transform.shift_scale_rotate is None            # the shipped hparams: none
    assert _model("synthetic").net.transform.shift_scale_rotate is None
    assert not any("shift_scale_rotate" in k for k in model.net.state_dict())       # a plain attribute: no state-dict key


# ---- 4. the captured step refuses it without capacities -------------------------------------------------------------------------
def test_captured_step_without_capacities_says_what_it_needs():
    """The refusal comes before anything touches the batch, so a stand-in for a CUDA image is enough here; the GPU file repeats it on
    real tensors."""
    import pytorch_retinanet_amd as P
    from pytorch_retinanet_amd.augment import ShiftScaleRotate
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    net = P.Retinanet(num_classes=3, backbone_kind="resnet18", pretrained=False, min_size=32, max_size=48).train()
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    net.transform.shift_scale_rotate = ShiftScaleRotate(seed=1)
    fake = [types.SimpleNamespace(is_cuda=True)]
    for kw in ({}, {"gt_capacity": "auto"}):
        step = CapturedTrainStep(net, opt, eager_steps=1, **kw)
        with pytest.raises(ValueError, match="gt_capacity= and image_capacity="):
            step(fake, [])
        assert step.captures == 0 and net.transform.shift_scale_rotate.counter == 0


# ---- 5. the host path of the transform ------------------------------------------------------------------------------------------
def _transforms(seed=9):
    from pytorch_retinanet_amd.augment import ColorJitter, RandomHorizontalFlip
    from pytorch_retinanet_amd.transform import GeneralizedRCNNTransform
    out = []
    for _ in range(2):
        t = GeneralizedRCNNTransform(32, 64, MEAN, STD).train()
        t.hflip = RandomHorizontalFlip(0.5, seed=seed)
        t.color_jitter = ColorJitter(0.4, 0.4, 0.4, 0.1, p=0.8, seed=seed)
        out.append(t)
    return out


def test_cpu_transform_equals_warping_first_and_then_the_plain_transform():
    from pytorch_retinanet_amd.augment import ShiftScaleRotate
    ims, boxes, labels = images(), gt_boxes(), gt_labels()
    t, plain = _transforms()
    ssr = t.shift_scale_rotate = ShiftScaleRotate(shift_limit=0.2, p=0.8, min_visibility=0.2, seed=6)
    applied = dropped = 0
    for k in range(4):
        targets = [{"boxes": b.clone(), "labels": l.clone()} for b, l in zip(boxes, labels)]
        got, got_t = t(ims, targets)
        c = ssr.draw(k, SIZES, boxes)
        assert np.array_equal(ssr.coefs.m, c.m) and ssr.coefs.applied == c.applied and ssr.counter == k + 1
        applied += sum(c.applied)
        warped = [ShiftScaleRotate.warp_image(im, c.inv[b], c.applied[b]) for b, im in enumerate(ims)]
        moved = ShiftScaleRotate.warp_boxes(c, SIZES, boxes, labels, ssr.min_visibility)
        dropped += sum(b.shape[0] - m[0].shape[0] for b, m in zip(boxes, moved))
        want, want_t = plain(warped, [{"boxes": bx, "labels": lb} for bx, lb in moved])
        assert torch.equal(_bits(got.tensors), _bits(want.tensors)), k
        assert got.image_sizes == want.image_sizes
        for a, b in zip(got_t, want_t):
            assert torch.equal(_bits(a["boxes"]), _bits(b["boxes"])) and torch.equal(a["labels"], b["labels"])
        assert all(torch.equal(x["boxes"], b) and torch.equal(x["labels"], l) for x, b, l in zip(targets, boxes, labels))   # not written
    assert applied >= 8 and dropped >= 1
    # eval mode and calls without targets never warp
    for train, with_targets in ((False, True), (False, False), (True, False)):
        t.train(train), plain.train(train)
        tg = (lambda: [{"boxes": b.clone(), "labels": l} for b, l in zip(boxes, labels)]) if with_targets else (lambda: None)
        got, _ = t(ims, tg())
        want, _ = plain(ims, tg())
        assert torch.equal(got.tensors, want.tensors) and ssr.counter == 4, (train, with_targets)


def test_it_runs_after_the_crop():
    from pytorch_retinanet_amd.augment import BBoxSafeRandomCrop, ShiftScaleRotate
    ims, boxes, labels = images(), gt_boxes(), gt_labels()
    t, plain = _transforms()
    t.crop, plain.crop = BBoxSafeRandomCrop(p=1.0, seed=2), BBoxSafeRandomCrop(p=1.0, seed=2)
    ssr = t.shift_scale_rotate = ShiftScaleRotate(p=1.0, seed=6)
    got, got_t = t(ims, [{"boxes": b.clone(), "labels": l} for b, l in zip(boxes, labels)])
    rects = t.crop.rects
    sliced = [im[:, y0:y0 + ch, x0:x0 + cw] for im, (y0, x0, ch, cw) in zip(ims, rects)]
    hw = [(r[2], r[3]) for r in rects]
    shifted = [b - torch.tensor([r[1], r[0], r[1], r[0]], dtype=torch.float32) if (r[0], r[1]) != (0, 0) and b.shape[0] else b for b, r in zip(boxes, rects)]
    c = ssr.draw(0, hw, shifted)
    assert any(r != (0, 0, h, w) for r, (h, w) in zip(rects, SIZES)) and any(c.applied)
    plain.crop = None
    warped = [ShiftScaleRotate.warp_image(im, c.inv[b], c.applied[b]) for b, im in enumerate(sliced)]
    want, want_t = plain(warped, [{"boxes": bx, "labels": lb} for bx, lb in ShiftScaleRotate.warp_boxes(c, hw, shifted, labels)])
    assert torch.equal(_bits(got.tensors), _bits(want.tensors))
    assert all(torch.equal(_bits(a["boxes"]), _bits(b["boxes"])) for a, b in zip(got_t, want_t))
