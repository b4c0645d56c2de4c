"""GPU: shift / scale / rotate on the device -- the draw (``rn_affine_draw``) against the float64 restatement, its packed rows, labels and
offsets against ``warp_boxes`` fed the device's coefficients, the warp (``rn_image_warp_stage``) against ``warp_image`` on the same
coefficients, hostile device data (a child process with every operand at the end of its mapping), the transform module on staged
images against the same call on pre-warped inputs, and ``CapturedTrainStep`` replaying one graph with a new draw each time.

Rows, labels, offsets and pixels are compared bit for bit: given the fp32 coefficients they are fp32 arithmetic without FMA that the
restatement repeats operation by operation.  The coefficients themselves are compared within one fp32 ulp of the value or
1e-9 max(h, w) absolute, whichever is larger: double-precision sin / cos may differ between host and device in the last double bit,
which can move the fp32 rounding by one step, and the absolute term covers the cancellation in the translation."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_shift_scale_rotate import MEAN, SIZES, STD, gt_boxes, gt_labels, images

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 2
PIX = 4096                                      # pixels per arena slot (>= 64 x 40): every slot 16-byte aligned
CAP = 4                                         # GT rows per image
SENTINEL = -7.25


def _bits(t):
    return t.contiguous().view(torch.int32)


def _stage(ims, boxes, labels=None, slot=3 * PIX):
    "The images into a fresh arena of ``slot`` floats per image and the GT into packed buffers whose unused rows hold the sentinel."
    from pytorch_retinanet_amd import ops
    dev = torch.device(DEV)
    B = len(ims)
    staged = ops.StagedImages(torch.full((B, slot), SENTINEL, dtype=torch.float32, device=dev), torch.empty((B, 2), dtype=torch.int32, device=dev))
    ops.image_stage([x.to(dev) for x in ims], staged)
    gt = ops.PackedGT.empty(B, CAP, dev)
    gt.gt_boxes.fill_(SENTINEL)
    labels = labels if labels is not None else [torch.ones((b.shape[0],), dtype=torch.int64) for b in boxes]
    ops.gt_stage([b.to(dev) for b in boxes], [l.to(dev) for l in labels], gt)
    return staged, gt


def _block(ssr):
    return ssr.device_block(torch.device(DEV))


def _check_rows(out, coefs, sizes, boxes, labels, mv=0.0):
    "The packed rows, labels and offsets equal ``warp_boxes`` on the device's coefficients bit for bit; -> the per-image counts."
    from pytorch_retinanet_amd.augment import ShiftScaleRotate
    want = ShiftScaleRotate.warp_boxes(coefs, sizes, boxes, labels, mv)
    counts = [int(w[0].shape[0]) for w in want]
    n = sum(counts)
    assert out.gt_off.tolist() == [sum(counts[:i]) for i in range(len(sizes) + 1)]
    assert torch.equal(_bits(out.gt_boxes[:n].cpu()), _bits(torch.cat([w[0] for w in want])))
    assert torch.equal(out.gt_labels[:n].cpu(), torch.cat([w[1] for w in want]))
    return counts


def _close(got, want, hw):
    "one fp32 ulp of the value, or 1e-9 max(h, w) absolute, whichever is larger (module docstring)"
    got, want = got.astype(np.float64), want.astype(np.float64)
    tol = np.maximum(np.spacing(np.abs(want).astype(np.float32)).astype(np.float64), 1e-9 * max(hw))
    return bool((np.abs(got - want) <= tol).all())


@pytest.fixture(scope="module")
def batch():
    "The shared inputs, and -- from the restatement alone -- the proof that counters 0, 1, 2 of SEED exercise the hard cases."
    from pytorch_retinanet_amd.augment import ShiftScaleRotate
    ims, boxes, labels = images(seed=3), gt_boxes(), gt_labels()
    ssr = ShiftScaleRotate(p=0.8, seed=SEED)
    drawn = [ssr.draw(k, SIZES, boxes) for k in range(3)]
    kept = [[int(w[0].shape[0]) for w in ShiftScaleRotate.warp_boxes(c, SIZES, boxes)] for c in drawn]
    # a row dropped in the middle of image 0 (its second box) moves every later image's offset; so does one of image 1
    assert any(c.applied[0] and k[0] == 3 for c, k in zip(drawn, kept)) and any(c.applied[1] and k[1] == 2 for c, k in zip(drawn, kept))
    assert any(not a for c in drawn for a in c.applied) and all(sum(c.applied) >= 3 for c in drawn)
    return ims, boxes, labels, drawn


# ---- 1. the draw ------------------------------------------------------------------------------------------------------
def test_draw_equals_the_restatement_and_advances_the_counter(batch):
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.augment import AffineCoefs, ShiftScaleRotate
    ims, boxes, labels, drawn = batch
    staged, gt = _stage(ims, boxes, labels)
    ssr = ShiftScaleRotate(p=0.8, seed=SEED)
    seen = set()
    for k in range(3):
        coef, out = ops.affine_draw(_block(ssr), staged.in_hw, gt)
        c = AffineCoefs.from_device(coef)
        assert c.applied == drawn[k].applied, k
        for b, hw in enumerate(SIZES):
            assert _close(c.m[b], drawn[k].m[b], hw) and _close(c.inv[b], drawn[k].inv[b], hw), (k, b, c.m[b], drawn[k].m[b])
        counts = _check_rows(out, c, SIZES, boxes, labels)
        assert ops.affine_coef_views(coef)[3].tolist() == counts
        assert ssr.counter == k + 1                                                        # the counter = the number of calls
        assert out.num_fg is gt.num_fg and out.cap_per_image == CAP
        seen.add(c.m.tobytes())
    assert len(seen) == 3                                                                  # every call draws differently
    n = sum(b.shape[0] for b in boxes)
    assert torch.equal(gt.gt_boxes[:n].cpu(), torch.cat(boxes)) and gt.gt_off.tolist() == [0, 4, 7, 8, 9, 9]     # the input is not written


def test_rows_past_the_last_image_are_not_written_and_two_calls_give_the_same_bits(batch):
    "The library call itself, on output buffers prefilled with a sentinel."
    import ctypes as C
    from pytorch_retinanet_amd import draw_state, ops
    from pytorch_retinanet_amd._lib import check, lib
    from pytorch_retinanet_amd.augment import AffineCoefs
    ims, boxes, labels, _ = batch
    staged, gt = _stage(ims, boxes, labels)
    dev = torch.device(DEV)
    res = []
    for _ in range(2):
        block = draw_state.new(draw_state.AFFINE, dev, seed=SEED, counter=0, p=1.0, min_visibility=0.0, lo=(-45.0, 0.9, -0.0625, -0.0625), hi=(45.0, 1.1, 0.0625, 0.0625))
        coef = torch.full((5, ops.AFFINE_COEF_WORDS), -1, dtype=torch.int32, device=dev)
        ob, ol, oo = torch.full_like(gt.gt_boxes, SENTINEL), torch.full_like(gt.gt_labels, -9), torch.full_like(gt.gt_off, -1)
        check(lib.rn_affine_draw(block.data_ptr(), gt.gt_boxes.data_ptr(), gt.gt_labels.data_ptr(), gt.gt_off.data_ptr(), staged.in_hw.data_ptr(),
                                 5, coef.data_ptr(), ob.data_ptr(), ol.data_ptr(), oo.data_ptr(), gt.rows,
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)), "draw")
        res.append((coef, ob, ol, oo))
    for a, b in zip(*res):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    coef, ob, ol, oo = res[0]
    n = oo.tolist()[-1]
    _check_rows(gt.with_rows(ob, ol, oo), AffineCoefs.from_device(coef), SIZES, boxes, labels)
    assert 0 < n < gt.rows and bool((ob[n:] == SENTINEL).all()) and bool((ol[n:] == -9).all())


def test_the_all_dropped_image_the_box_free_image_a_nan_box_and_min_visibility():
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.augment import AffineCoefs, ShiftScaleRotate
    sizes = [(12, 20)] * 5
    g = torch.Generator().manual_seed(4)
    ims = [torch.rand((3, 12, 20), generator=g) for _ in sizes]
    boxes = [torch.tensor([[10.0, 1.0, 14.0, 3.0], [12.0, 7.0, 18.0, 10.0]]),                          # both leave: the image is left alone
             torch.zeros((0, 4)),                                                                      # no rows: warped all the same
             torch.tensor([[1.0, 1.0, 6.0, 4.0], [float("nan"), 1.0, 6.0, 4.0], [2.0, 2.0, 7.0, 5.0]]),   # the NaN row goes, the others stay
             torch.tensor([[8.0, 2.0, 15.0, 5.5], [1.0, 1.0, 4.0, 4.0]]),                              # the first keeps 2 of 7 columns
             torch.tensor([[1.0, 1.0, 6.0, float("inf")]])]                                            # its only row is not finite: left alone
    labels = [torch.arange(10 * b, 10 * b + bx.shape[0]) for b, bx in enumerate(boxes)]
    staged, gt = _stage(ims, boxes, labels, slot=3 * 12 * 20)
    for mv, kept in ((0.0, [2, 0, 2, 2, 1]), (0.5, [2, 0, 2, 1, 1])):
        ssr = ShiftScaleRotate(shift_limit=(0.5, 0.5), scale_limit=0.0, rotate_limit=0, p=1.0, min_visibility=mv, seed=SEED)
        want = ssr.draw(0, sizes, boxes)
        assert want.applied == [False, True, True, True, False]
        coef, out = ops.affine_draw(_block(ssr), staged.in_hw, gt)
        c = AffineCoefs.from_device(coef)
        assert c.applied == want.applied and np.array_equal(c.m, want.m) and np.array_equal(c.inv, want.inv)    # (cos 0, sin 0: exact)
        assert _check_rows(out, c, sizes, boxes, labels, mv) == kept
        n = sum(kept)
        rows = out.gt_boxes[:n].cpu()
        assert torch.equal(_bits(rows[:2]), _bits(boxes[0])) and torch.equal(_bits(rows[-1:]), _bits(boxes[4]))    # left alone: bit for bit
        assert out.gt_labels[:n].tolist() == ([0, 1, 20, 22, 30, 31, 40] if mv == 0.0 else [0, 1, 20, 22, 31, 40])
        res = ops.image_warp_stage(staged, coef)
        for b in (0, 4):
            assert torch.equal(_bits(res.arena[b]), _bits(staged.arena[b]))
        assert not torch.equal(res.arena[1], staged.arena[1])


def test_draw_does_not_depend_on_64_images_or_64_rows():
    "B = 130: more images than a wave has lanes; one image of 150 rows: more rows than a wave has lanes, every third one dropped."
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.augment import AffineCoefs, ShiftScaleRotate
    dev = torch.device(DEV)
    rng = np.random.default_rng(2)
    B, cap = 130, 150
    sizes = [(int(rng.integers(8, 40)), int(rng.integers(8, 40))) for _ in range(B)]
    boxes = []
    for b, (h, w) in enumerate(sizes):
        n = cap if b == 77 else (0 if b % 3 == 2 else int(rng.integers(1, 4)))
        x1, y1 = rng.uniform(0, w - 2, n), rng.uniform(0, h - 2, n)
        bx = np.stack([x1, y1, x1 + rng.uniform(1, 2, n), y1 + rng.uniform(1, 2, n)], 1).astype(np.float32).reshape(-1, 4)
        if b == 77:
            bx[::3] += 1000.0                                                              # far outside: dropped
        boxes.append(torch.from_numpy(bx))
    labels = [torch.from_numpy(rng.integers(1, 90, b.shape[0])) for b in boxes]
    gt = ops.PackedGT.empty(B, cap, dev)
    ops.gt_stage([b.to(dev) for b in boxes], [l.to(dev) for l in labels], gt)
    in_hw = torch.tensor(sizes, dtype=torch.int32).to(dev)
    ssr = ShiftScaleRotate(p=0.9, seed=5)
    ssr.reseed(5, 7)
    coef, out = ops.affine_draw(_block(ssr), in_hw, gt)
    c = AffineCoefs.from_device(coef)
    assert c.applied == ssr.draw(7, sizes, boxes).applied and c.applied[77] and ssr.counter == 8
    counts = _check_rows(out, c, sizes, boxes, labels)
    assert counts[77] <= 100 and sum(a and n < b.shape[0] for a, n, b in zip(c.applied, counts, boxes)) >= 5


# ---- 2. the warp ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slot", [3 * PIX, 3 * 64 * 40 + 1], ids=["aligned-slots", "odd-slot"])
def test_warp_equals_the_restatement_and_leaves_the_rest_of_the_slot(batch, slot):
    """p = 1 and the default ranges on every listed size.  ``odd-slot``: a slot that is no multiple of 4 floats -- destination slots
    1..4 are not 16-byte aligned, so the 64 x 40 image takes the 4-byte stores there and the 16-byte ones with aligned slots."""
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.augment import AffineCoefs, ShiftScaleRotate
    ims, boxes, labels, _ = batch
    staged, gt = _stage(ims, boxes, labels, slot)
    dev = torch.device(DEV)
    ssr = ShiftScaleRotate(p=1.0, seed=SEED)
    for k in range(2):
        coef, _ = ops.affine_draw(_block(ssr), staged.in_hw, gt)
        c = AffineCoefs.from_device(coef)
        assert c.applied == [True] * 5
        dst = ops.StagedImages(torch.full((5, slot), SENTINEL, dtype=torch.float32, device=dev), torch.empty((5, 2), dtype=torch.int32, device=dev))
        res = ops.image_warp_stage(staged, coef, out=dst)
        assert res.arena.data_ptr() == dst.arena.data_ptr() and res.in_hw is staged.in_hw and res.slot == slot
        got = res.arena.cpu()
        for b, im in enumerate(ims):
            for where in ("cpu", DEV):                                                     # the restatement runs on both
                want = ShiftScaleRotate.warp_image(im.to(where), c.inv[b]).cpu().reshape(-1)
                assert torch.equal(_bits(got[b, : want.numel()]), _bits(want)), (k, b, where)
            assert bool((got[b, want.numel():] == SENTINEL).all()), (k, b)
    assert bool((staged.arena[:, 3 * 64 * 40:] == SENTINEL).all())                         # the source arena is only read


def test_p_zero_copies_bit_for_bit_including_nan_and_inf(batch):
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.augment import ShiftScaleRotate
    ims, boxes, labels, _ = batch
    weird = [im.clone() for im in ims]
    weird[0][1, 5, 7], weird[0][2, 36, 52], weird[1][0, 0, 0], weird[4][2, 15, 15] = float("nan"), float("inf"), float("-inf"), float("nan")
    weird[3].view(torch.int32)[0, 0, 3] = 0x7FC12345                                       # a NaN with a payload
    for slot in (3 * PIX, 3 * 64 * 40 + 1):
        staged, gt = _stage(weird, boxes, labels, slot)
        ssr = ShiftScaleRotate(p=0.0, seed=SEED)
        coef, out = ops.affine_draw(_block(ssr), staged.in_hw, gt)
        dev = torch.device(DEV)
        dst = ops.StagedImages(torch.full((5, slot), SENTINEL, dtype=torch.float32, device=dev), torch.empty((5, 2), dtype=torch.int32, device=dev))
        res = ops.image_warp_stage(staged, coef, out=dst)
        assert torch.equal(_bits(res.arena), _bits(staged.arena))                          # (the sentinel past 3 h w on both sides)
        assert ops.affine_coef_views(coef)[2].tolist() == [0] * 5
        n = sum(b.shape[0] for b in boxes)
        assert torch.equal(_bits(out.gt_boxes[:n]), _bits(gt.gt_boxes[:n])) and torch.equal(out.gt_off, gt.gt_off)


# ---- 3. hostile device data -------------------------------------------------------------------------------------------
def test_hostile_sizes_and_offsets_stay_inside_the_operands():
    """``tools/guard_probe.py affine``, a child process: every operand ends at the end of its own mapping; an image that claims h = 0
    and one that claims a size no slot holds are skipped (their slots stay as they were) and the others come out right; offsets below
    0 and past rows are clamped."""
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "guard_probe.py"), "affine"], capture_output=True, text=True, env=env,
                       timeout=300, cwd=ROOT)
    tail = (r.stdout + r.stderr)[-1500:]
    assert r.returncode == 0, f"probe affine failed:\n{tail}"
    assert "ok affine" in r.stdout, tail


# ---- 4. the transform module ------------------------------------------------------------------------------------------
def _module(crop=False):
    from pytorch_retinanet_amd.augment import BBoxSafeRandomCrop, ColorJitter, RandomHorizontalFlip, RandomShortSide
    from pytorch_retinanet_amd.transform import GeneralizedRCNNTransform
    t = GeneralizedRCNNTransform((24, 32), 48, MEAN, STD, size_divisible=32).train()
    t.hflip = RandomHorizontalFlip(0.5, seed=3)
    t.scale_jitter = RandomShortSide((24, 32), seed=4)
    t.color_jitter = ColorJitter(brightness=0.4, contrast=0.4, saturation=0.5, hue=0.1, p=0.8, seed=17)
    if crop:
        t.crop = BBoxSafeRandomCrop(p=0.7, seed=15)
    return t


SIZES5 = [(37, 53), (64, 40), (5, 7), (40, 40), (16, 16)]          # sizes the resize accepts (the 1-pixel images are the warp's business)


def _boxes5():
    b = gt_boxes()
    return [b[0], b[1], torch.tensor([[1.0, 1.0, 4.0, 3.5]]), torch.tensor([[7.3, 2.5, 9.9, 30.1], [30.0, 1.0, 39.0, 6.0]]), b[4]]


@pytest.mark.parametrize("crop", [False, True], ids=["alone", "after-the-crop"])
def test_staged_transform_equals_the_same_transform_on_pre_warped_inputs(crop):
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.augment import AffineCoefs, ShiftScaleRotate
    g = torch.Generator().manual_seed(3)
    ims, boxes = [torch.rand((3, h, w), generator=g) for h, w in SIZES5], _boxes5()
    labels = [torch.arange(10 * b + 1, 10 * b + 1 + bx.shape[0]) for b, bx in enumerate(boxes)]
    t, plain = _module(crop), _module(crop)
    ssr = t.shift_scale_rotate = ShiftScaleRotate(shift_limit=0.2, p=0.8, seed=SEED)
    dropped = 0
    for k in range(3):
        staged, gt = _stage(ims, boxes, labels)
        got, got_t = t(staged, gt, canvas=(64, 64))
        assert ssr.counter == k + 1
        c = AffineCoefs.from_device(ssr.coef)
        if crop:
            rects = [tuple(r) for r in t.crop.rect.tolist()]
            base_ims = [im[:, y0:y0 + ch, x0:x0 + cw].contiguous() for im, (y0, x0, ch, cw) in zip(ims, rects)]
            base_boxes = [b - torch.tensor([r[1], r[0], r[1], r[0]], dtype=torch.float32) if (r[0], r[1]) != (0, 0) and b.shape[0] else b
                          for b, r in zip(boxes, rects)]
            hw = [(r[2], r[3]) for r in rects]
            plain.crop = None                                                              # the reference call gets the windows themselves
        else:
            base_ims, base_boxes, hw = ims, boxes, SIZES5
        warped = [ShiftScaleRotate.warp_image(im.to(DEV), c.inv[b], c.applied[b]).cpu() for b, im in enumerate(base_ims)]
        moved = ShiftScaleRotate.warp_boxes(c, hw, base_boxes, labels)
        dropped += sum(b.shape[0] - m[0].shape[0] for b, m in zip(boxes, moved))
        staged, gt = _stage(warped, [m[0] for m in moved], [m[1] for m in moved])
        want, want_t = plain(staged, gt, canvas=(64, 64))
        n = sum(m[0].shape[0] for m in moved)
        assert torch.equal(_bits(got.tensors), _bits(want.tensors)), k
        assert got_t.gt_off.tolist() == want_t.gt_off.tolist() and got_t.gt_off.tolist()[-1] == n
        assert torch.equal(_bits(got_t.gt_boxes[:n]), _bits(want_t.gt_boxes[:n])) and torch.equal(got_t.gt_labels[:n], want_t.gt_labels[:n]), k
        assert torch.equal(t.hflip.flags, plain.hflip.flags) and torch.equal(t.scale_jitter.sizes_drawn, plain.scale_jitter.sizes_drawn)
        assert torch.equal(_bits(t.color_jitter.coef), _bits(plain.color_jitter.coef))     # the contrast's mean: taken over the warped image
    assert dropped >= 1
    # eval mode never warps: the staged eval path is the plain one, and the counter stays
    t.eval(), plain.eval()
    staged, _ = _stage(ims, boxes)
    got, _ = t(staged, None, canvas=(64, 64))
    want, _ = plain(staged, None, canvas=(64, 64))
    assert torch.equal(_bits(got.tensors), _bits(want.tensors)) and ssr.counter == 3


def test_cuda_lists_take_the_host_draw():
    "Not staged: the stream of draws from the restatement (one synchronisation), the images warped by torch ops on the device."
    from pytorch_retinanet_amd.augment import ShiftScaleRotate
    g = torch.Generator().manual_seed(3)
    ims, boxes = [torch.rand((3, h, w), generator=g).to(DEV) for h, w in SIZES5], _boxes5()
    t, plain = _module(), _module()
    ssr = t.shift_scale_rotate = ShiftScaleRotate(p=0.8, seed=SEED)
    targets = lambda bs: [{"boxes": b.to(DEV), "labels": torch.ones((b.shape[0],), dtype=torch.int64, device=DEV)} for b in bs]
    got, got_t = t(ims, targets(boxes))
    c = ssr.draw(0, SIZES5, boxes)
    assert np.array_equal(ssr.coefs.m, c.m) and ssr.counter == 1 and any(c.applied)
    warped = [ShiftScaleRotate.warp_image(im, c.inv[b], c.applied[b]) for b, im in enumerate(ims)]
    want, want_t = plain(warped, targets([m[0] for m in ShiftScaleRotate.warp_boxes(c, SIZES5, boxes)]))
    assert torch.equal(_bits(got.tensors), _bits(want.tensors))
    assert all(torch.equal(_bits(a["boxes"]), _bits(b["boxes"])) and a["boxes"].is_cuda for a, b in zip(got_t, want_t))


# ---- 5. the captured step ---------------------------------------------------------------------------------------------
def _run_steps(data, captured, with_all):
    from pytorch_retinanet_amd.augment import BBoxSafeRandomCrop, RandomHorizontalFlip, ShiftScaleRotate
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from test_gt_capacity_gpu import _params
    from test_image_capacity_gpu import _setup96
    net, opt = _setup96()
    ssr = net.transform.shift_scale_rotate = ShiftScaleRotate(p=0.9, seed=SEED)
    if with_all:
        net.transform.crop, net.transform.hflip = BBoxSafeRandomCrop(p=0.7, seed=5), RandomHorizontalFlip(0.5, seed=6)
    step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=1 if captured else 10 ** 6, gt_capacity="auto", image_capacity="auto")
    losses, coefs = [], []
    for ims, tgs in data:
        losses.append(float(step(ims, tgs)["loss"]))
        coefs.append(ssr.coef.cpu().clone())
    torch.cuda.synchronize()
    return np.array(losses), coefs, _params(net), step, ssr


@pytest.mark.parametrize("with_all", [False, True], ids=["alone", "with-crop-and-flip"])
def test_captured_step_draws_anew_at_every_replay_and_equals_the_eager_staged_step(with_all):
    """One capture, three replays, each with other coefficients; the replayed run equals the same staged steps run eagerly (same
    counters, so the same draws) within the bars of ``test_gt_capacity_gpu._compare_to_eager``."""
    from test_image_capacity_gpu import COUNTS32, FIRST, SECOND, _size_batches
    sets = [[FIRST[i % 4], SECOND[i % 4]] for i in range(4)]
    data = _size_batches(sets, COUNTS32[:4], seed=6)
    loss_g, coef_g, par_g, step, ssr = _run_steps(data, True, with_all)
    assert step.captures == 1 and step.replays == 3 and ssr.counter == 4
    assert len({c.numpy().tobytes() for c in coef_g}) == 4 and sum(int(c[:, 12].sum()) for c in coef_g) >= 4
    (key,) = list(step._entries)
    assert ("shift_scale_rotate", ssr) in key
    loss_e, coef_e, par_e, eager, _ = _run_steps(data, False, with_all)
    assert eager.captures == 0
    if not with_all:                        # (with a crop the sizes feed the draw's matrices: equal too, but only the losses are compared there)
        assert all(torch.equal(a, b) for a, b in zip(coef_g, coef_e))
    assert np.all(np.isfinite(loss_g))
    np.testing.assert_allclose(loss_g, loss_e, rtol=2e-2)
    for k, a in par_e.items():
        torch.testing.assert_close(par_g[k], a, rtol=0, atol=2e-3, msg=k)
    step.net.transform.shift_scale_rotate = None
    assert not any(isinstance(k, tuple) and k and k[0] == "shift_scale_rotate" for k in step._signature(*data[0]))


def test_without_capacities_it_is_refused():
    from pytorch_retinanet_amd.augment import ShiftScaleRotate
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from test_image_capacity_gpu import FIRST, SECOND, _setup96, _size_batches
    net, opt = _setup96()
    net.transform.shift_scale_rotate = ShiftScaleRotate(seed=SEED)
    (ims, tgs), = _size_batches([[FIRST[0], SECOND[0]]], [[3, 5]], seed=6)
    for kw in ({}, {"gt_capacity": "auto"}):
        step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=1, **kw)
        with pytest.raises(ValueError, match="image_capacity"):
            step(ims, tgs)
        assert net.transform.shift_scale_rotate.counter == 0 and step.captures == 0
