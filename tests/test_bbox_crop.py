"""CPU: the bbox-safe random crop (``augment.BBoxSafeRandomCrop``) -- the invariants of the Python restatement of ``rn_bbox_crop_draw``
(every rectangle inside its image, around every box, in the image's orientation), its identity cases, the object's state, the hparams
mapping, the PyTorch path of the transform and ``staged_bounds``.

``SIZES`` / ``gt_boxes()`` are the batch ``tests/test_bbox_crop_gpu.py`` runs on the device as well."""
import logging

import numpy as np
import pytest
import torch

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
SIZES = [(37, 53), (64, 48), (5, 7), (40, 40), (33, 61)]          # landscape, portrait, tiny, square, landscape


def gt_boxes():
    """Per image of ``SIZES``: several boxes; one box; none; a fractional box whose union starts at the odd pixel 7; boxes touching the
    right and the bottom edge whose union is tall (the widening of step 5 in a landscape image)."""
    return [torch.tensor([[3.5, 4.0, 20.0, 30.0], [10.0, 2.0, 40.25, 12.0], [30.0, 20.0, 44.0, 31.5]]),
            torch.tensor([[5.0, 6.0, 20.0, 50.0]]),
            torch.zeros((0, 4)),
            torch.tensor([[7.3, 2.5, 9.9, 30.1]]),
            torch.tensor([[52.0, 2.0, 61.0, 20.0], [54.5, 10.0, 60.0, 33.0]])]


def images(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand((3, h, w), generator=g) for h, w in SIZES]


def shift_boxes(boxes, rect):
    "The restatement of step 6 in torch: one fp32 subtraction per coordinate; a rectangle at the origin leaves the bits alone."
    y0, x0 = rect[0], rect[1]
    if (y0, x0) == (0, 0):
        return boxes.clone()
    return boxes - torch.tensor([x0, y0, x0, y0], dtype=torch.float32)


def _inside(box, h, w):
    return 0 <= box[0] <= box[2] <= w and 0 <= box[1] <= box[3] <= h


# ---- 1. the restatement's invariants ------------------------------------------------------------------------------------------
def test_every_rectangle_is_inside_its_image_around_every_box_and_keeps_the_orientation():
    from pytorch_retinanet_amd.augment import BBoxSafeRandomCrop
    boxes = gt_boxes()
    widened = moved = 0
    for seed in range(20):
        for counter in range(15):
            rects = BBoxSafeRandomCrop.draw_rects(seed, counter, SIZES, boxes, 0.9)
            for (h, w), bx, (y0, x0, ch, cw) in zip(SIZES, boxes, rects):
                assert 0 <= y0 and 0 <= x0 and ch >= 1 and cw >= 1 and y0 + ch <= h and x0 + cw <= w
                assert (ch <= cw) if h <= w else (ch >= cw)
                for b in bx.tolist():
                    if _inside(b, h, w):
                        assert x0 <= b[0] and b[2] <= x0 + cw and y0 <= b[1] and b[3] <= y0 + ch, (seed, counter, b)
                widened += ch == cw and h != w
                moved += (y0, x0, ch, cw) != (0, 0, h, w)
    assert widened > 10 and moved > 600                                # the hard branches are exercised (1500 draws)


def test_boxes_outside_the_image_never_move_the_rectangle_outside():
    from pytorch_retinanet_amd.augment import BBoxSafeRandomCrop
    wild = [torch.tensor([[-30.0, -2.0, 1e30, 9.0]]), torch.tensor([[70.0, 90.0, 80.0, 99.0]]), torch.tensor([[-9.0, -9.0, -3.0, -1.0]]),
            torch.tensor([[-1e30, 3.0, 4.0, 1e38]]), torch.tensor([[61.0, 33.0, 61.0, 33.0]])]
    for counter in range(40):
        for (h, w), (y0, x0, ch, cw) in zip(SIZES, BBoxSafeRandomCrop.draw_rects(5, counter, SIZES, wild, 1.0)):
            assert 0 <= y0 and 0 <= x0 and ch >= 1 and cw >= 1 and y0 + ch <= h and x0 + cw <= w
            assert (ch <= cw) if h <= w else (ch >= cw)


def test_identity_cases():
    from pytorch_retinanet_amd.augment import BBoxSafeRandomCrop
    boxes = gt_boxes()
    full = [(0, 0, h, w) for h, w in SIZES]
    for counter in range(5):
        assert BBoxSafeRandomCrop.draw_rects(3, counter, SIZES, boxes, 0.0) == full                       # p = 0
        rects = BBoxSafeRandomCrop.draw_rects(3, counter, SIZES, boxes, 1.0)
        assert rects[2] == full[2]                                                                         # no boxes
        for bad in (float("nan"), float("inf"), float("-inf")):
            for col in range(4):
                broken = [b.clone() for b in boxes]
                broken[0][1, col] = bad
                got = BBoxSafeRandomCrop.draw_rects(3, counter, SIZES, broken, 1.0)
                lost = bad != bad or (bad > 0) == (col >= 2)           # a NaN always; an infinity only where it is the extreme
                assert (got[0] == full[0]) if lost else (got[0][2] >= 1), (bad, col)
                assert got[1:] == rects[1:]                                                                # the others are not touched
        # a box touching all four borders leaves nothing to cut
        whole = [torch.tensor([[0.0, 0.0, float(w), float(h)]]) for h, w in SIZES]
        assert BBoxSafeRandomCrop.draw_rects(3, counter, SIZES, whole, 1.0) == full
    # an empty image: the zero rectangle, whatever its boxes
    assert BBoxSafeRandomCrop.draw_rects(3, 0, [(0, 9), (4, 0), (-1, 5)], [boxes[1]] * 3, 1.0) == [(0, 0, 0, 0)] * 3
    assert BBoxSafeRandomCrop.draw_rects(3, 0, SIZES, [None] * 5, 1.0) == full


def test_the_salts_are_new():
    import re
    import os
    from pytorch_retinanet_amd import augment
    mine = [augment.CROP_SALT_APPLY, augment.CROP_SALT_LEFT, augment.CROP_SALT_TOP, augment.CROP_SALT_RIGHT, augment.CROP_SALT_BOTTOM]
    other = [augment.SHORT_SIDE_SALT, augment.COLOR_SALT_APPLY, augment.COLOR_SALT_ORDER, *augment.COLOR_SALT_FACTOR, 0]
    assert len(set(mine + other)) == len(mine) + len(other)
    header = open(os.path.join(os.path.dirname(augment.__file__), "..", "include", "retinanet_hip.h")).read()
    for s in mine:
        assert len(re.findall("0x%016X" % s, header)) == 1


# ---- 2. the object ------------------------------------------------------------------------------------------------------------
def test_two_objects_with_one_seed_agree_and_the_state_round_trips():
    from pytorch_retinanet_amd.augment import BBoxSafeRandomCrop
    boxes = gt_boxes()
    a, b = BBoxSafeRandomCrop(p=0.75, seed=11), BBoxSafeRandomCrop(p=0.75, seed=11)
    seen = set()
    for k in range(4):
        ra = a.next_rects(SIZES, boxes)
        assert ra == b.next_rects(SIZES, boxes) == a.draw(k, SIZES, boxes) == BBoxSafeRandomCrop.draw_rects(11, k, SIZES, boxes, 0.75)
        assert a.counter == k + 1 and a.rects == ra
        seen.add(tuple(ra))
    assert len(seen) == 4 and BBoxSafeRandomCrop(p=0.75, seed=12).draw(0, SIZES, boxes) != a.draw(0, SIZES, boxes)
    state = a.state_dict()
    assert state == {"seed": 11, "counter": 4, "p": 0.75}
    c = BBoxSafeRandomCrop(seed=1)
    assert c.p == 1.0
    c.load_state_dict(state)
    assert c.state_dict() == state and c.next_rects(SIZES, boxes) == a.next_rects(SIZES, boxes)
    c.set_rank(2)
    assert c.seed == 3 and c.counter == 5                              # the constructor's seed + rank, the counter kept
    c.p = 0.0
    assert c.next_rects(SIZES, boxes) == [(0, 0, h, w) for h, w in SIZES]
    with pytest.raises(ValueError):
        c.p = 1.5
    with pytest.raises(RuntimeError, match="GPU"):
        c.device_block("cpu")


def test_bound_follows_the_orientation():
    from pytorch_retinanet_amd.augment import BBoxSafeRandomCrop
    assert BBoxSafeRandomCrop.bound(37, 53, 800, 1333) == (800, 1333)
    assert BBoxSafeRandomCrop.bound(40, 40, 800, 1333) == (800, 1333)
    assert BBoxSafeRandomCrop.bound(64, 48, 800, 1333) == (1333, 800)


# ---- 3. hparams ---------------------------------------------------------------------------------------------------------------
def test_hparams_mapping_and_its_warnings(caplog):
    from pytorch_retinanet_amd.augment import BBoxSafeRandomCrop, bbox_crop_from_transforms, from_transforms
    crop = bbox_crop_from_transforms([{"class_name": "albumentations.BBoxSafeRandomCrop"}], seed=4)
    assert isinstance(crop, BBoxSafeRandomCrop) and crop.p == 1.0 and crop.seed == 4
    crop = bbox_crop_from_transforms([{"class_name": "albumentations.HorizontalFlip"},
                                      {"class_name": "albumentations.BBoxSafeRandomCrop", "params": {"p": 0.25}}])
    assert crop.p == 0.25
    assert bbox_crop_from_transforms([{"class_name": "albumentations.BBoxSafeRandomCrop", "params": {"p": 0.25, "always_apply": True}}]).p == 1.0
    assert bbox_crop_from_transforms(None) is None and bbox_crop_from_transforms([{"class_name": "albumentations.HorizontalFlip"}]) is None
    with caplog.at_level(logging.WARNING):
        crop = bbox_crop_from_transforms([{"class_name": "albumentations.BBoxSafeRandomCrop", "params": {"erosion_rate": 0.2, "p": 0.5}}])
    assert crop.p == 0.5 and sum("erosion_rate" in r.getMessage() for r in caplog.records) == 1
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        assert bbox_crop_from_transforms([{"class_name": "albumentations.BBoxSafeRandomCrop", "params": {"erosion_rate": 0.0}}]) is not None
        # the flip mapping does not warn about the crop's entry, and still does about every other crop
        assert from_transforms([{"class_name": "albumentations.BBoxSafeRandomCrop"}]) is None
        assert not caplog.records
        for other in ("albumentations.RandomSizedBBoxSafeCrop", "albumentations.RandomCrop"):
            assert bbox_crop_from_transforms([{"class_name": other, "params": {"height": 8, "width": 8}}]) is None
            assert from_transforms([{"class_name": other}]) is None
    msgs = [r.getMessage() for r in caplog.records]
    assert sum("RandomSizedBBoxSafeCrop" in m and "skipped" in m for m in msgs) == 1 and sum("albumentations.RandomCrop" in m for m in msgs) == 1


def test_prepare_data_installs_the_crop(tmp_path, caplog):
    from pytorch_retinanet_amd.augment import BBoxSafeRandomCrop
    from test_hflip import _model, _png_csv
    path = _png_csv(tmp_path)
    with caplog.at_level(logging.WARNING):
        model = _model("csv", path, [{"class_name": "albumentations.HorizontalFlip", "params": {"p": 0.5}},
                                     {"class_name": "albumentations.BBoxSafeRandomCrop", "params": {"p": 0.3}}])
    assert not any("BBoxSafeRandomCrop" in r.getMessage() for r in caplog.records)
    crop = model.net.transform.crop
    assert isinstance(crop, BBoxSafeRandomCrop) and crop.p == float(np.float32(0.3)) and model.net.transform.hflip is not None
    assert _model("csv", path).net.transform.crop is None                         # the shipped hparams: no crop
    assert _model("synthetic").net.transform.crop is None
    assert not any("crop" in k for k in model.net.state_dict())                   # a plain attribute: no state-dict key


# ---- 4. the PyTorch path of the transform -------------------------------------------------------------------------------------
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


def test_cpu_transform_with_a_crop_equals_slicing_and_then_the_uncropped_transform():
    from pytorch_retinanet_amd.augment import BBoxSafeRandomCrop
    ims, boxes = images(), gt_boxes()
    labels = [torch.ones((b.shape[0],), dtype=torch.int64) for b in boxes]
    t, plain = _transforms()
    t.crop = BBoxSafeRandomCrop(p=0.8, seed=6)
    moved = 0
    for k in range(4):
        targets = [{"boxes": b.clone(), "labels": l} for b, l in zip(boxes, labels)]
        got, got_t = t(ims, targets)
        rects = BBoxSafeRandomCrop.draw_rects(6, k, SIZES, boxes, 0.8)
        assert t.crop.rects == rects and t.crop.counter == k + 1
        moved += sum(r != (0, 0, h, w) for r, (h, w) in zip(rects, SIZES))
        sliced = [im[:, y0:y0 + ch, x0:x0 + cw].contiguous() for im, (y0, x0, ch, cw) in zip(ims, rects)]
        want, want_t = plain(sliced, [{"boxes": shift_boxes(b, r), "labels": l} for b, r, l in zip(boxes, rects, labels)])
        assert torch.equal(got.tensors.view(torch.int32), want.tensors.view(torch.int32)), k
        assert got.image_sizes == want.image_sizes
        for a, b in zip(got_t, want_t):
            assert torch.equal(a["boxes"].view(torch.int32), b["boxes"].view(torch.int32)) and torch.equal(a["labels"], b["labels"])
        assert all(torch.equal(x["boxes"], b) for x, b in zip(targets, boxes))     # the caller's targets are not written
    assert moved >= 8
    # eval mode and calls without targets never crop
    for train, with_targets in ((False, True), (False, False), (True, False)):
        t.train(train), plain.train(train)
        tg = (lambda: [{"boxes": b.clone(), "labels": l} for b, l in zip(boxes, labels)]) if with_targets else (lambda: None)
        got, _ = t(ims, tg())
        want, _ = plain(ims, tg())
        assert torch.equal(got.tensors, want.tensors) and t.crop.counter == 4, (train, with_targets)


def test_staged_bounds_with_a_crop_are_the_orientation_bounds():
    from pytorch_retinanet_amd.augment import BBoxSafeRandomCrop, RandomShortSide
    from pytorch_retinanet_amd.transform import GeneralizedRCNNTransform
    t = GeneralizedRCNNTransform(96, 120, MEAN, STD).train()
    plain = t.staged_bounds(SIZES)
    t.crop = BBoxSafeRandomCrop()
    assert t.staged_bounds(SIZES) == [(96, 120), (120, 96), (96, 120), (96, 120), (96, 120)]
    assert all(p[0] <= c[0] and p[1] <= c[1] for p, c in zip(plain, t.staged_bounds(SIZES)))
    assert t.staged_eval_bounds(SIZES) == plain                                   # eval mode never crops
    t.scale_jitter = RandomShortSide((64, 80), seed=1)
    assert t.staged_bounds(SIZES)[:2] == [(80, 120), (120, 80)]
    t.scale_jitter = None
    t.min_size = (64, 96)
    with pytest.raises(ValueError, match="min_size"):
        t.staged_bounds(SIZES)
