"""GPU: the bbox-safe random crop on the device -- the draw (``rn_bbox_crop_draw``) against its Python restatement, the copy
(``rn_image_crop_stage``) against the sliced tensors, the transform module on staged images with every augmentation installed against
the same call on pre-sliced images, and ``CapturedTrainStep`` replaying one graph with a new crop each time.

Every comparison is exact: the draw is integer arithmetic on a 24-bit hash apart from two fp32 multiplies per axis that numpy
restates, the boxes take one fp32 subtraction each, and the copy moves bits."""
import numpy as np
import pytest
import torch

from test_bbox_crop import MEAN, SIZES, STD, gt_boxes, images, shift_boxes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, P = 15, 0.7
PIX = 4096                                      # pixels per arena slot (>= 64 x 48): a slot of 12288 floats, every slot 16-byte aligned
CAP = 4                                         # GT rows per image
SENTINEL = -7.25
FULL = [(0, 0, h, w) for h, w in SIZES]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _stage(ims, boxes, slot=3 * PIX):
    "The images into a fresh arena of ``slot`` floats per image and the boxes into packed GT whose unused rows hold the sentinel."
    from pytorch_retinanet_amd import ops
    dev = torch.device(DEV)
    B = len(ims)
    staged = ops.StagedImages(torch.full((B, slot), SENTINEL, dtype=torch.float32, device=dev), torch.empty((B, 2), dtype=torch.int32, device=dev))
    ops.image_stage([x.to(dev) for x in ims], staged)
    gt = ops.PackedGT.empty(B, CAP, dev)
    gt.gt_boxes.fill_(SENTINEL)
    ops.gt_stage([b.to(dev) for b in boxes], [torch.ones((b.shape[0],), dtype=torch.int64, device=dev) for b in boxes], gt)
    return staged, gt


def _check_boxes(out, boxes, rects):
    "The packed rows equal the restatement's bit for bit; the rows past gt_off[B] keep what the buffer held."
    want = torch.cat([shift_boxes(b, r) for b, r in zip(boxes, rects)])
    n = want.shape[0]
    assert torch.equal(_bits(out[:n].cpu()), _bits(want))
    return n


@pytest.fixture(scope="module")
def batch():
    "The shared inputs, and -- from the restatement alone -- the proof that counters 0, 1, 2 exercise the hard cases."
    from pytorch_retinanet_amd import augment
    from pytorch_retinanet_amd.augment import BBoxSafeRandomCrop
    ims, boxes = images(seed=3), gt_boxes()
    rects = [BBoxSafeRandomCrop.draw_rects(SEED, k, SIZES, boxes, P) for k in range(3)]
    moved = [(b, k, r) for k, rs in enumerate(rects) for b, r in enumerate(rs) if r != FULL[b]]
    assert any(r[1] % 2 == 1 for _, _, r in moved)                                        # an odd x0: 4-byte aligned source rows
    assert any(r[3] % 4 != 0 for _, _, r in moved)                                        # cw % 4 != 0: 16-byte stores across rows
    # the widening of step 5: in the landscape image 4 the rectangle of step 4 is taller than wide
    widened = 0
    for b, k, (y0, x0, ch, cw) in moved:
        if b == 4:
            u = lambda salt: augment.hflip_u(SEED ^ salt, k, b)
            s, e = augment._crop_axis(u(augment.CROP_SALT_LEFT), u(augment.CROP_SALT_RIGHT), 52, 61, 61)
            widened += e - s < ch and cw == ch
    assert widened >= 1
    # the identity cases: no rows (image 2, always) and u_apply >= p; the non-finite box and the empty image are test_identity's
    assert all(rs[2] == FULL[2] for rs in rects)
    assert any(not augment.hflip_u(SEED ^ augment.CROP_SALT_APPLY, k, b) < float(np.float32(P)) for k in range(3) for b in (0, 1, 3, 4))
    return ims, boxes, rects


# ---- 1. the draw ------------------------------------------------------------------------------------------------------
def test_draw_equals_the_restatement_and_advances_the_counter(batch):
    from pytorch_retinanet_amd import draw_state, ops
    ims, boxes, rects = batch
    staged, gt = _stage(ims, boxes)
    block = draw_state.new(draw_state.BBOX_CROP, torch.device(DEV), seed=SEED, counter=0, p=P)
    for k in range(3):
        rect, crop_hw, out = ops.bbox_crop_draw(block, staged.in_hw, gt)
        # (a fresh buffer per call: prefilled here through the allocator is not possible, so the untouched rows are checked in the next test)
        assert [tuple(r) for r in rect.tolist()] == rects[k], k
        assert crop_hw.tolist() == [[r[2], r[3]] for r in rects[k]]
        _check_boxes(out, boxes, rects[k])
        assert draw_state.read(draw_state.BBOX_CROP, block)[1] == k + 1                                 # the counter = the number of calls
    assert torch.equal(gt.gt_boxes[: sum(b.shape[0] for b in boxes)].cpu(), torch.cat(boxes))  # out of place: the input is not written


def test_rows_past_the_last_image_are_not_written(batch):
    "The library call itself, on an output buffer prefilled with a sentinel."
    import ctypes as C
    from pytorch_retinanet_amd import draw_state, ops
    from pytorch_retinanet_amd._lib import check, lib
    ims, boxes, rects = batch
    staged, gt = _stage(ims, boxes)
    dev = torch.device(DEV)
    block = draw_state.new(draw_state.BBOX_CROP, dev, seed=SEED, counter=1, p=P)
    rect = torch.full((5, 4), -1, dtype=torch.int32, device=dev)
    crop_hw = torch.full((5, 2), -1, dtype=torch.int32, device=dev)
    out = torch.full_like(gt.gt_boxes, SENTINEL)
    check(lib.rn_bbox_crop_draw(block.data_ptr(), gt.gt_boxes.data_ptr(), gt.gt_off.data_ptr(), staged.in_hw.data_ptr(), 5, rect.data_ptr(),
                                crop_hw.data_ptr(), out.data_ptr(), gt.rows, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "draw")
    assert [tuple(r) for r in rect.tolist()] == rects[1]
    n = _check_boxes(out, boxes, rects[1])
    assert n < gt.rows and bool((out[n:] == SENTINEL).all())


def test_identity_for_a_non_finite_box_an_empty_image_and_p_zero(batch):
    from pytorch_retinanet_amd import draw_state, ops
    from pytorch_retinanet_amd.augment import BBoxSafeRandomCrop
    ims, boxes, _ = batch
    broken = [b.clone() for b in boxes]
    broken[1][0, 2] = float("nan")
    broken[4][1, 3] = float("inf")
    staged, gt = _stage(ims, broken)
    staged.in_hw[3] = 0                                                                    # an empty image: (0, 0)
    sizes = [s if b != 3 else (0, 0) for b, s in enumerate(SIZES)]
    block = draw_state.new(draw_state.BBOX_CROP, torch.device(DEV), seed=SEED, counter=0, p=1.0)
    want = BBoxSafeRandomCrop.draw_rects(SEED, 0, sizes, broken, 1.0)
    assert want[1] == FULL[1] and want[4] == FULL[4] and want[3] == (0, 0, 0, 0) and want[0] != FULL[0]
    rect, crop_hw, out = ops.bbox_crop_draw(block, staged.in_hw, gt)
    assert [tuple(r) for r in rect.tolist()] == want and crop_hw.tolist() == [[r[2], r[3]] for r in want]
    n = sum(b.shape[0] for b in broken)
    assert torch.equal(_bits(out[:n].cpu()), _bits(torch.cat([shift_boxes(b, r) for b, r in zip(broken, want)])))    # NaN and inf copied bit for bit
    # the empty image's slot is not touched by the copy; the others are the slices
    dst = ops.StagedImages(torch.full_like(staged.arena, SENTINEL), torch.empty_like(staged.in_hw))
    res = ops.image_crop_stage(staged, rect, crop_hw, out=dst)
    assert bool((res.arena[3] == SENTINEL).all()) and res.in_hw.tolist()[3] == [0, 0]
    draw_state.write(draw_state.BBOX_CROP, block, p=0.0)
    rect, _, out = ops.bbox_crop_draw(block, staged.in_hw, gt)
    assert [tuple(r) for r in rect.tolist()] == [f if b != 3 else (0, 0, 0, 0) for b, f in enumerate(FULL)]
    assert torch.equal(_bits(out[:n]), _bits(gt.gt_boxes[:n]))


def test_draw_does_not_depend_on_64_images():
    "B = 130: more images than a wave has lanes, every third one without boxes."
    from pytorch_retinanet_amd import draw_state, ops
    from pytorch_retinanet_amd.augment import BBoxSafeRandomCrop
    dev = torch.device(DEV)
    rng = np.random.default_rng(2)
    B = 130
    sizes = [(int(rng.integers(8, 40)), int(rng.integers(8, 40))) for _ in range(B)]
    boxes = []
    for b, (h, w) in enumerate(sizes):
        n = 0 if b % 3 == 2 else int(rng.integers(1, 4))
        x1, y1 = rng.uniform(0, w - 2, n), rng.uniform(0, h - 2, n)
        boxes.append(torch.from_numpy(np.stack([x1, y1, x1 + rng.uniform(1, 2, n), y1 + rng.uniform(1, 2, n)], 1).astype(np.float32)).reshape(-1, 4))
    gt = ops.PackedGT.empty(B, CAP, dev)
    ops.gt_stage([b.to(dev) for b in boxes], [torch.ones((b.shape[0],), dtype=torch.int64, device=dev) for b in boxes], gt)
    in_hw = torch.tensor(sizes, dtype=torch.int32).to(dev)
    block = draw_state.new(draw_state.BBOX_CROP, dev, seed=5, counter=7, p=0.9)
    rect, crop_hw, out = ops.bbox_crop_draw(block, in_hw, gt)
    want = BBoxSafeRandomCrop.draw_rects(5, 7, sizes, boxes, 0.9)
    assert [tuple(r) for r in rect.tolist()] == want and draw_state.read(draw_state.BBOX_CROP, block)[1] == 8
    _check_boxes(out, boxes, want)


# ---- 2. the copy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slot", [3 * PIX, 3 * 64 * 48 + 1], ids=["aligned-slots", "odd-slot"])
def test_copy_equals_the_sliced_tensor_and_leaves_the_rest_of_the_slot(batch, slot):
    "``odd-slot``: a slot that is no multiple of 4 floats -- destination slots 1..4 are not 16-byte aligned and take the 4-byte stores."
    from pytorch_retinanet_amd import ops
    ims, boxes, rects = batch
    staged, _ = _stage(ims, boxes, slot)
    dev = torch.device(DEV)
    for k in range(3):
        rect = torch.tensor(rects[k], dtype=torch.int32).to(dev)
        crop_hw = rect[:, 2:].contiguous()
        dst = ops.StagedImages(torch.full((5, slot), SENTINEL, dtype=torch.float32, device=dev), torch.empty((5, 2), dtype=torch.int32, device=dev))
        res = ops.image_crop_stage(staged, rect, crop_hw, out=dst)
        assert res.arena.data_ptr() == dst.arena.data_ptr() and res.in_hw is crop_hw and res.slot == slot
        got = res.arena.cpu()
        for b, (im, (y0, x0, ch, cw)) in enumerate(zip(ims, rects[k])):
            want = im[:, y0:y0 + ch, x0:x0 + cw].contiguous().reshape(-1)
            assert torch.equal(_bits(got[b, : want.numel()]), _bits(want)), (k, b)
            assert bool((got[b, want.numel():] == SENTINEL).all()), (k, b)
    assert bool((staged.arena[:, 3 * 64 * 48:] == SENTINEL).all())                         # the source arena is only read


def test_copy_clamps_a_rectangle_that_leaves_the_image_and_skips_what_fits_no_slot(batch):
    from pytorch_retinanet_amd import ops
    ims, boxes, _ = batch
    staged, _ = _stage(ims, boxes)
    dev = torch.device(DEV)
    wild = [(30, 50, 100, 100), (-5, -5, 10, 10), (0, 0, 0, 3), (39, 39, 2 ** 30, 2 ** 30), (0, 0, 33, 61)]
    clamped = [(30, 50, 7, 3), (0, 0, 10, 10), None, (39, 39, 1, 1), (0, 0, 33, 61)]
    rect = torch.tensor(wild, dtype=torch.int32).to(dev)
    small = 3 * 33 * 61 - 1                                                                # image 4's window is one float too large
    dst = ops.StagedImages(torch.full((5, small), SENTINEL, dtype=torch.float32, device=dev), torch.empty((5, 2), dtype=torch.int32, device=dev))
    got = ops.image_crop_stage(staged, rect, rect[:, 2:].contiguous(), out=dst).arena.cpu()
    for b, (im, r) in enumerate(zip(ims, clamped)):
        n = 0
        if r is not None and b != 4:
            y0, x0, ch, cw = r
            want = im[:, y0:y0 + ch, x0:x0 + cw].contiguous().reshape(-1)
            n = want.numel()
            assert torch.equal(_bits(got[b, :n]), _bits(want)), b
        assert bool((got[b, n:] == SENTINEL).all()), b


# ---- 3. the transform module ------------------------------------------------------------------------------------------
def _module():
    from pytorch_retinanet_amd.augment import ColorJitter, RandomHorizontalFlip, RandomShortSide
    from pytorch_retinanet_amd.transform import GeneralizedRCNNTransform
    t = GeneralizedRCNNTransform((24, 32), 48, MEAN, STD, size_divisible=32).train()
    t.hflip = RandomHorizontalFlip(0.5, seed=3)
    t.scale_jitter = RandomShortSide((24, 32), seed=4)
    t.color_jitter = ColorJitter(brightness=0.4, contrast=0.4, saturation=0.5, hue=0.1, p=0.8, seed=17)
    return t


def test_staged_transform_with_a_crop_equals_the_same_transform_on_pre_sliced_images(batch):
    from pytorch_retinanet_amd.augment import BBoxSafeRandomCrop
    ims, boxes, rects = batch
    t, plain = _module(), _module()
    crop = t.crop = BBoxSafeRandomCrop(p=P, seed=SEED)
    n = sum(b.shape[0] for b in boxes)
    for k in range(3):
        staged, gt = _stage(ims, boxes)
        got, got_t = t(staged, gt, canvas=(64, 64))
        assert [tuple(r) for r in crop.rect.tolist()] == rects[k] and crop.counter == k + 1
        sliced = [im[:, y0:y0 + ch, x0:x0 + cw].contiguous() for im, (y0, x0, ch, cw) in zip(ims, rects[k])]
        staged, gt = _stage(sliced, [shift_boxes(b, r) for b, r in zip(boxes, rects[k])])
        want, want_t = plain(staged, gt, canvas=(64, 64))
        assert torch.equal(_bits(got.tensors), _bits(want.tensors)), k
        assert torch.equal(_bits(got_t.gt_boxes[:n]), _bits(want_t.gt_boxes[:n])), k
        assert torch.equal(t.hflip.flags, plain.hflip.flags) and torch.equal(t.scale_jitter.sizes_drawn, plain.scale_jitter.sizes_drawn)
        assert torch.equal(_bits(t.color_jitter.coef), _bits(plain.color_jitter.coef))     # the contrast's mean: taken over the window
    # eval mode never crops: the staged eval path is the plain one, and the counter stays
    t.eval(), plain.eval()
    staged, _ = _stage(ims, boxes)
    got, _ = t(staged, None, canvas=(64, 64))
    want, _ = plain(staged, None, canvas=(64, 64))
    assert torch.equal(_bits(got.tensors), _bits(want.tensors)) and crop.counter == 3


def test_cuda_lists_take_the_host_draw(batch):
    "Not staged: the same stream from the restatement (one synchronisation), the fused path on the slices."
    from pytorch_retinanet_amd.augment import BBoxSafeRandomCrop
    ims, boxes, rects = batch
    t, plain = _module(), _module()
    t.crop = BBoxSafeRandomCrop(p=P, seed=SEED)
    dev_ims = [x.to(DEV) for x in ims]
    targets = lambda bs: [{"boxes": b.to(DEV), "labels": torch.ones((b.shape[0],), dtype=torch.int64, device=DEV)} for b in bs]
    got, got_t = t(dev_ims, targets(boxes))
    assert t.crop.rects == rects[0] and t.crop.counter == 1
    sliced = [im[:, y0:y0 + ch, x0:x0 + cw].contiguous() for im, (y0, x0, ch, cw) in zip(dev_ims, rects[0])]
    want, want_t = plain(sliced, targets([shift_boxes(b, r) for b, r in zip(boxes, rects[0])]))
    assert torch.equal(_bits(got.tensors), _bits(want.tensors))
    assert all(torch.equal(_bits(a["boxes"]), _bits(b["boxes"])) for a, b in zip(got_t, want_t))


# ---- 4. the captured step ---------------------------------------------------------------------------------------------
def test_captured_step_draws_a_new_crop_at_every_replay():
    from pytorch_retinanet_amd.augment import BBoxSafeRandomCrop
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from test_image_capacity_gpu import COUNTS32, FIRST, SECOND, _setup96, _size_batches
    sets = [[FIRST[i % 4], SECOND[i % 4]] for i in range(4)]
    data = _size_batches(sets, COUNTS32[:4], seed=6)
    net, opt = _setup96()
    crop = net.transform.crop = BBoxSafeRandomCrop(p=0.9, seed=SEED)
    step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=1, gt_capacity="auto", image_capacity="auto")
    moved = 0
    for k, (ims, tgs) in enumerate(data):
        if k == 3:
            crop.p = 0.0                                                                   # rewritten between replays: no new capture
        loss = float(step(ims, tgs)["loss"])
        want = BBoxSafeRandomCrop.draw_rects(SEED, k, sets[k], [t["boxes"].cpu() for t in tgs], 0.9 if k < 3 else 0.0)
        assert [tuple(r) for r in crop.rect.tolist()] == want, k
        assert np.isfinite(loss)
        moved += sum(r != (0, 0, h, w) for r, (h, w) in zip(want, sets[k]))
    torch.cuda.synchronize()
    assert step.captures == 1 and step.replays == 3 and crop.counter == 4
    assert moved >= 3 and want == [(0, 0, h, w) for h, w in sets[3]]
    (key,) = list(step._entries)
    assert ("crop", crop) in key and key[0][2] == (96, 128)
    net.transform.crop = None
    assert not any(isinstance(k, tuple) and k and k[0] == "crop" for k in step._signature(*data[0]))


def test_a_crop_without_image_capacity_is_refused():
    from pytorch_retinanet_amd.augment import BBoxSafeRandomCrop
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from test_image_capacity_gpu import FIRST, SECOND, _setup96, _size_batches
    net, opt = _setup96()
    net.transform.crop = BBoxSafeRandomCrop(seed=SEED)
    step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=1, gt_capacity="auto")
    (ims, tgs), = _size_batches([[FIRST[0], SECOND[0]]], [[3, 5]], seed=6)
    with pytest.raises(ValueError, match="image_capacity"):
        step(ims, tgs)
    assert net.transform.crop.counter == 0 and step.captures == 0
