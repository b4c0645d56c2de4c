"""GPU: the image capacity mode -- images of varying sizes staged into a fixed arena (``rn_image_stage``), the resize plan, the
transform and the box rescale reading every input size from device memory (``rn_resize_plan_dev``, ``rn_transform_batch_var``,
``rn_gt_flip_scale_packed_var``), and ``graph.CapturedTrainStep(image_capacity=...)`` replaying one graph for batches whose image
sizes differ.

Bars: the kernels run the existing kernels' arithmetic on the same values -- bit for bit (``torch.equal``) against
``ops.transform_batch`` / ``_flip``, ``RandomShortSide.draw`` / ``rn_short_side_draw`` and ``ops.gt_flip_scale_packed_dev``; whole
train steps against an eager twin with the mode off at the tolerances of ``tests/test_gt_capacity_gpu.py`` (bf16 conv stack,
MIOpen's atomically accumulated weight gradients)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RN_EINVAL = -1
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
SIZES = [(37, 53), (64, 40), (1, 7), (50, 50)]
PIX = 2 ** 16
SENTINEL = -7.25
GUARD = 1024                                    # floats before and after a guarded buffer (a multiple of 4: 16-byte alignment is kept)


def _images(sizes, seed=0, misalign_first=False):
    g = torch.Generator().manual_seed(seed)
    ims = [torch.rand((3, h, w), generator=g).to(DEV) for h, w in sizes]
    if misalign_first:                          # image 0 four bytes past a 16-byte boundary: the 4-byte copy path
        h, w = sizes[0]
        buf = torch.zeros(3 * h * w + 1, device=DEV)
        buf[1:].copy_(ims[0].reshape(-1))
        ims[0] = buf[1:].view(3, h, w)
        assert ims[0].data_ptr() % 16 == 4
    return ims


def _guarded_arena(B, pix=PIX):
    "(the whole buffer, an ``ops.StagedImages`` over its middle): sentinels everywhere, ``in_hw`` inside a guarded buffer too."
    from pytorch_retinanet_amd import ops
    slot = 3 * pix
    buf = torch.full((GUARD + B * slot + GUARD,), SENTINEL, device=DEV)
    hwbuf = torch.full((16 + 2 * B + 16,), -99, dtype=torch.int32, device=DEV)
    staged = ops.StagedImages(buf[GUARD:GUARD + B * slot].view(B, slot), hwbuf[16:16 + 2 * B].view(B, 2))
    return buf, hwbuf, staged


def _check_staged(buf, hwbuf, staged, ims):
    torch.cuda.synchronize()
    B = len(ims)
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())
    assert bool((hwbuf[:16] == -99).all()) and bool((hwbuf[-16:] == -99).all())
    for b, im in enumerate(ims):
        n = im.numel()
        assert torch.equal(staged.arena[b, :n], im.reshape(-1)), b
        assert bool((staged.arena[b, n:] == SENTINEL).all()), b
    assert staged.in_hw.tolist() == [list(im.shape[1:]) for im in ims] == [list(s) for s in staged.hw]
    assert staged.B == B


# ---- 1. rn_image_stage -----------------------------------------------------------------------------------------------------
def test_stage_copies_each_image_into_its_slot_and_nothing_else():
    from pytorch_retinanet_amd import ops
    ims = _images(SIZES, misalign_first=True)
    buf, hwbuf, staged = _guarded_arena(len(ims))
    assert ops.image_stage(ims, staged) is staged
    _check_staged(buf, hwbuf, staged, ims)
    # a strided image is made dense by the wrapper; staging again overwrites the prefixes only
    ims2 = _images([(50, 50), (1, 7), (64, 40), (37, 53)], seed=1)
    ims2[2] = ims2[2].transpose(1, 2).contiguous().transpose(1, 2)
    assert not ims2[2].is_contiguous()
    ops.image_stage(ims2, staged)
    torch.cuda.synchronize()
    for b, im in enumerate(ims2):
        assert torch.equal(staged.arena[b, :im.numel()], im.contiguous().reshape(-1))
    assert staged.in_hw.tolist() == [[50, 50], [1, 7], [64, 40], [37, 53]]
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def test_stage_crosses_the_64_image_launch_boundary():
    from pytorch_retinanet_amd import ops
    ims = _images([(8, 12)] * 65, seed=2)
    buf, hwbuf, staged = _guarded_arena(65, pix=128)                # (3 x 8 x 12 = 288 of 384 floats per slot)
    ops.image_stage(ims, staged)
    _check_staged(buf, hwbuf, staged, ims)


def test_stage_rejects_what_does_not_fit_before_anything_runs():
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd._lib import lib
    ims = _images(SIZES)
    buf, hwbuf, staged = _guarded_arena(len(ims))
    before = buf.clone()
    with pytest.raises(ValueError, match="does not fit"):
        ops.image_stage(ims[:3] + [torch.rand(3, 300, 300, device=DEV)], staged)              # 90000 pixels > 2**16
    with pytest.raises(ValueError, match="does not fit"):
        ops.image_stage(ims[:3] + [torch.empty(3, 0, 5, device=DEV)], staged)
    with pytest.raises(ValueError, match="f32"):
        ops.image_stage(ims[:3] + [torch.zeros(3, 8, 8, dtype=torch.uint8, device=DEV)], staged)
    with pytest.raises(ValueError, match="f32"):
        ops.image_stage(ims[:3] + [torch.rand(8, 8, 3, device=DEV)], staged)                   # HWC
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.image_stage(ims[:3] + [torch.rand(3, 8, 8)], staged)
    with pytest.raises(ValueError, match="slots"):
        ops.image_stage(ims[:3], staged)
    # the library's own checks: every argument before any launch
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptrs = (C.c_void_p * 4)(*[im.data_ptr() for im in ims])

    def call(hw, slot=staged.slot):
        return lib.rn_image_stage(ptrs, (C.c_int32 * 8)(*hw), 4, staged.arena.data_ptr(), slot, staged.in_hw.data_ptr(), st)
    good = [v for s in SIZES for v in s]
    assert call(good, slot=3 * 64 * 40 - 1) == RN_EINVAL                 # image 1 is one float too large for the slot
    assert call(good[:6] + [0, 50]) == RN_EINVAL and call(good[:6] + [50, -1]) == RN_EINVAL
    assert call(good[:6] + [300, 300]) == RN_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and bool((hwbuf == -99).all())        # nothing ran


# ---- 2. rn_resize_plan_dev -------------------------------------------------------------------------------------------------
def _in_hw(sizes):
    return torch.tensor(sizes, dtype=torch.int32).to(DEV)


def test_plan_with_a_fixed_short_side_equals_the_host_arithmetic():
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.transform import GeneralizedRCNNTransform, _ratios
    tr = GeneralizedRCNNTransform(48, 64, MEAN, STD)
    sizes = SIZES + [(48, 64), (64, 48), (7, 1), (1000, 999)]
    out_hw, ratios = ops.resize_plan_dev(None, _in_hw(sizes), 48, 64)
    want_hw, want_r = [], []
    for h, w in sizes:
        scale = tr._scale_for(h, w, 48.0)
        new = (int(math.floor(h * scale)), int(math.floor(w * scale)))
        want_hw.append(list(new))
        want_r += list(_ratios((h, w), new))
    assert out_hw.tolist() == want_hw
    assert torch.equal(ratios.cpu(), torch.tensor(want_r, dtype=torch.float32))
    assert want_hw[4] == [48, 64]                                        # the identity case
    # one launch serves any B (no 64-image table); a size < 1 gives an empty plan entry
    many = [(8 + i % 5, 12 + i % 7) for i in range(131)] + [(0, 9), (5, -2)]
    out_hw, ratios = ops.resize_plan_dev(None, _in_hw(many), 48, 64)
    want = [list(tr.staged_bounds([s])[0]) for s in many[:131]] + [[0, 0], [0, 0]]
    assert out_hw.tolist() == want and ratios[-4:].tolist() == [0.0] * 4
    with pytest.raises(ValueError, match="short side"):
        ops.resize_plan_dev(None, _in_hw(sizes), None, 64)


def test_plan_with_a_state_block_draws_the_short_side_stream():
    from pytorch_retinanet_amd.augment import RandomShortSide
    a, b = RandomShortSide((32, 48, 64), seed=5), RandomShortSide((32, 48, 64), seed=5)
    in_hw = _in_hw(SIZES)
    for n in range(5):
        hw_a, r_a = a.next_sizes_dev(in_hw, 64)
        hw_b, r_b = b.next_sizes(SIZES, 64, torch.device(DEV))           # rn_short_side_draw, host sizes in the kernel arguments
        want = a.draw(n, SIZES, 64)
        assert hw_a.tolist() == [list(s) for s in want], n
        assert torch.equal(r_a.cpu(), torch.tensor(RandomShortSide.ratios(SIZES, want), dtype=torch.float32).reshape(-1)), n
        assert torch.equal(hw_a, hw_b) and torch.equal(r_a, r_b), n
        assert a.sizes_drawn is hw_a and a.ratios_drawn is r_a
    assert a.counter == 5 and b.counter == 5
    assert len({tuple(map(tuple, a.draw(n, SIZES, 64))) for n in range(5)}) > 1        # the stream really varies


def test_plan_equals_the_table_draw_across_its_64_image_launches():
    "B = 70: ``rn_short_side_draw`` takes two launches that share one counter value, the device-sizes plan one; the same rows, twice."
    from pytorch_retinanet_amd.augment import RandomShortSide
    sizes = [(30 + (i * 7) % 41, 25 + (i * 11) % 53) for i in range(70)]
    a, b = RandomShortSide((32, 40, 48, 56, 64), seed=9), RandomShortSide((32, 40, 48, 56, 64), seed=9)
    in_hw = _in_hw(sizes)
    for n in range(2):
        hw_a, r_a = a.next_sizes_dev(in_hw, 64)
        hw_b, r_b = b.next_sizes(sizes, 64, torch.device(DEV))
        assert torch.equal(hw_a, hw_b) and torch.equal(r_a, r_b), n
        assert hw_a.tolist() == [list(s) for s in a.draw(n, sizes, 64)], n
    assert a.counter == 2 and b.counter == 2


def test_stage_keeps_the_callers_bounds_for_the_transform():
    from pytorch_retinanet_amd import ops
    ims = _images(SIZES[:2])
    staged = ops.new_image_arena(2, PIX, torch.device(DEV))
    assert ops.image_stage(ims, staged, bounds=[(44, 64), (64, 40)]).bounds == [(44, 64), (64, 40)]
    assert ops.image_stage(ims, staged).bounds is None and staged.hw == SIZES[:2]
    with pytest.raises(ValueError, match="bounds"):
        ops.image_stage(ims, staged, bounds=[(44, 64)])


# ---- 3. rn_transform_batch_var ---------------------------------------------------------------------------------------------
T_SIZES = SIZES + [(48, 64)]                    # + the identity case (short 48)
_SHARED = {}


def _transform_inputs():
    "Staged once and shared (read-only) by the transform tests: the images, the arena, the plan and the host sizes."
    if not _SHARED:
        from pytorch_retinanet_amd import ops
        ims = _images(T_SIZES, seed=3)
        staged = ops.image_stage(ims, ops.new_image_arena(len(ims), PIX, torch.device(DEV)))
        out_hw, _ = ops.resize_plan_dev(None, staged.in_hw, 48, 64)
        flags = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8).to(DEV)
        torch.cuda.synchronize()
        _SHARED.update(ims=ims, staged=staged, out_hw=out_hw, host=[tuple(s) for s in out_hw.tolist()], flags=flags)
    return _SHARED


@pytest.mark.parametrize("flip", [False, True], ids=["noflags", "flags"])
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("canvas", [(64, 64), (64, 96)], ids=["64x64", "64x96"])
def test_var_transform_equals_the_host_size_transform(canvas, dtype, channels_last, flip):
    from pytorch_retinanet_amd import ops
    s = _transform_inputs()
    flags = s["flags"] if flip else None
    hp, wp = canvas
    got = ops.transform_batch_var(s["staged"], s["out_hw"], MEAN, STD, hp, wp, dtype, channels_last, flags=flags)
    want = ops.transform_batch(s["ims"], s["host"], MEAN, STD, hp, wp, dtype, channels_last, flags=flags)
    torch.cuda.synchronize()
    assert got.dtype == dtype and got.shape == want.shape == (5, 3, hp, wp) and got.stride() == want.stride()
    assert torch.equal(got, want)
    assert bool(got[4, :, :48, :64].any()) and (wp == 64 or not bool(got[:, :, :, 64:].any()))
    assert s["host"][4] == (48, 64)


@pytest.mark.parametrize("bad", [(0, 5), (4096, 4096)], ids=["zero-height", "above-the-slot"])
def test_sizes_no_slot_can_hold_leave_the_image_all_padding(bad):
    """``in_hw`` overwritten on the device for one image: the kernel's own checks reject both values -- that image's canvas is all
    zeros, the others are as before and the margins around the output keep their sentinel."""
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd._lib import lib
    s = _transform_inputs()
    staged = s["staged"]
    want = ops.transform_batch(s["ims"], s["host"], MEAN, STD, 64, 64, torch.float32, False)
    in_hw = staged.in_hw.clone()
    in_hw[1] = torch.tensor(bad, dtype=torch.int32)
    n = 5 * 3 * 64 * 64
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, device=DEV)
    out = buf[GUARD:GUARD + n].view(5, 3, 64, 64)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for flags in (None, s["flags"]):
        rc = lib.rn_transform_batch_var(staged.arena.data_ptr(), staged.slot, in_hw.data_ptr(), s["out_hw"].data_ptr(), 5, (C.c_float * 3)(*MEAN),
                                        (C.c_float * 3)(*STD), 64, 64, out.data_ptr(), 0, 0, flags.data_ptr() if flags is not None else None, st)
        assert rc == 0
        torch.cuda.synchronize()
        assert not bool(out[1].any())
        ref = want if flags is None else ops.transform_batch(s["ims"], s["host"], MEAN, STD, 64, 64, torch.float32, False, flags=flags)
        for b in (0, 2, 3, 4):
            assert torch.equal(out[b], ref[b]), b
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


# ---- 4. rn_gt_flip_scale_packed_var ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [False, True], ids=["noflags", "flags"])
def test_var_box_rescale_equals_the_host_width_form(flip):
    from pytorch_retinanet_amd import ops
    from test_gt_capacity_gpu import _gt, _poisoned
    counts = [3, 0, 9, 1]
    boxes, labels = _gt(np.random.default_rng(4), counts, H=37, W=40)
    p = ops.gt_stage(boxes, labels, _poisoned(4, 9))
    in_hw = _in_hw(SIZES)
    _, ratios = ops.resize_plan_dev(None, in_hw, 48, 64)
    flags = torch.tensor([1, 0, 1, 1], dtype=torch.uint8).to(DEV) if flip else None
    got = ops.gt_flip_scale_packed_var(p, in_hw, ratios, flags)
    want = ops.gt_flip_scale_packed_dev(p, [float(w) for _, w in SIZES], ratios, flags)
    torch.cuda.synchronize()
    n = sum(counts)
    assert got.gt_boxes.data_ptr() != p.gt_boxes.data_ptr() and got.gt_off is p.gt_off
    assert torch.equal(got.gt_boxes[:n], want.gt_boxes[:n]) and not torch.equal(got.gt_boxes[:n], p.gt_boxes[:n])
    assert torch.equal(p.gt_boxes[:n], torch.cat(boxes))                  # the staged buffer is left as it was


# ---- 5. whole train steps --------------------------------------------------------------------------------------------------
def _setup96(seed=11, dtype=torch.bfloat16):
    "``test_graph_gpu._setup`` at min_size 96 / max_size 120 (the construction ``test_gt_capacity_gpu`` uses for resized images)."
    import pytorch_retinanet_amd as P
    from pytorch_retinanet_amd.optim import MasterSGD, use_16bit_conv_weights
    torch.manual_seed(seed)
    net = P.Retinanet(num_classes=5, backbone_kind="resnet18", pretrained=False, min_size=96, max_size=120).to(DEV)
    net = net.to(memory_format=torch.channels_last).train()
    use_16bit_conv_weights(net, dtype)
    return net, MasterSGD(net.parameters(), lr=1e-2, momentum=0.9, weight_decay=1e-3)


def _size_batches(size_sets, count_sets, seed=5):
    "One batch per entry: images of the given raw sizes with the given box counts (boxes inside their image)."
    from test_gt_capacity_gpu import _gt
    rng = np.random.default_rng(seed)
    out = []
    for sizes, counts in zip(size_sets, count_sets):
        images = [torch.from_numpy(rng.random((3, h, w), dtype=np.float32)).to(DEV) for h, w in sizes]
        targets = []
        for (h, w), c in zip(sizes, counts):
            b, l = _gt(rng, [c], H=h, W=w)
            targets.append({"boxes": b[0], "labels": l[0]})
        out.append((images, targets))
    return out


FIRST = [(128, 160), (64, 80), (112, 140), (96, 120)]                     # all resize to 96 x 120
SECOND = [(100, 150), (60, 60), (90, 160), (120, 121)]                    # 80 x 120, 96 x 96, 67 x 120, 96 x 96
COUNTS32 = [[3, 9], [32, 1], [0, 17], [12, 12], [31, 2], [5, 20], [9, 0], [25, 30]]      # all in class 32


def test_one_graph_serves_a_canvas_class():
    """Every batch's natural canvas is the class's 96 x 128, so the run with the mode off (eager) is a valid yardstick: same losses
    and parameters at the bars of ``test_gt_capacity_gpu._compare_to_eager``."""
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from test_gt_capacity_gpu import _params
    data = _size_batches([[FIRST[i % 4], SECOND[i % 4]] for i in range(8)], COUNTS32)
    res = {}
    for on in (False, True):
        net, opt = _setup96()
        step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=2, enabled=on, gt_capacity="auto" if on else None,
                                 image_capacity="auto" if on else None)
        losses = [float(step(im, tg)["loss"]) for im, tg in data]
        torch.cuda.synchronize()
        res[on] = (np.array(losses), _params(net), step)
    assert np.all(np.isfinite(res[True][0]))
    np.testing.assert_allclose(res[True][0], res[False][0], rtol=2e-2)
    for k, a in res[False][1].items():
        torch.testing.assert_close(res[True][1][k], a, rtol=0, atol=2e-3, msg=k)
    step = res[True][2]
    assert step.captures == 1 and step.replays == 6 and res[False][2].replays == 0
    (key,) = list(step._entries)
    assert key[0] == ("img_cap", 2, (96, 128), 2 ** 16, torch.float32, torch.device(DEV)) and key[1] == ("gt_cap", 32)


def test_class_changes_recapture_and_oversized_batches_keep_exact_keys():
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    net, opt = _setup96()
    step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=1, gt_capacity="auto", image_capacity="auto")
    landscape = [[(128, 160), (64, 80)], [(96, 120), (60, 60)], [(112, 140), (100, 150)]]
    portrait = [[(160, 128), (150, 100)], [(80, 64), (60, 60)], [(140, 112), (121, 120)]]
    mixed = [[(160, 128), (128, 160)], [(150, 100), (64, 80)], [(80, 64), (90, 160)]]
    sets = landscape + portrait + mixed
    losses = [float(step(im, tg)["loss"]) for im, tg in _size_batches(sets, [[3, 5]] * 9, seed=8)]
    assert np.all(np.isfinite(losses))
    assert step.captures == 3 and step.replays == 6                       # per class: one eager call, then the capture and two replays
    assert [k[0][2] for k in step._entries] == [(96, 128), (128, 96), (128, 128)]
    # a one-entry class list and a batch above it: the exact-shape key and path, as oversized GT keeps them
    step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=1, gt_capacity="auto", image_capacity=[(96, 128)])
    data = _size_batches([portrait[0], landscape[0]], [[3, 5]] * 2, seed=9)
    losses = [float(step(im, tg)["loss"]) for im, tg in data]
    keys = list(step._entries)
    assert np.all(np.isfinite(losses)) and step.captures == 0
    assert keys[0][0] == tuple(((3, h, w), torch.float32, torch.device(DEV)) for h, w in portrait[0])
    assert keys[1][0][0] == "img_cap" and step._entries[keys[0]].staged is None and step._entries[keys[1]].staged is not None


def test_flip_jitter_and_both_capacity_modes_in_one_graph():
    from pytorch_retinanet_amd.augment import RandomHorizontalFlip, RandomShortSide
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    net, opt = _setup96()
    flip = net.transform.hflip = RandomHorizontalFlip(p=0.5, seed=3)
    jitter = net.transform.scale_jitter = RandomShortSide((64, 80, 96), seed=4)
    step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=2, gt_capacity="auto", image_capacity="auto")
    sets = [[FIRST[i % 4], SECOND[(i + 1) % 4]] for i in range(6)]
    data = _size_batches(sets, COUNTS32[:6], seed=6)
    losses = [float(step(im, tg)["loss"]) for im, tg in data]
    torch.cuda.synchronize()
    assert step.captures == 1 and step.replays == 4 and np.all(np.isfinite(losses))
    assert flip.counter == 6 and jitter.counter == 6
    assert jitter.sizes_drawn.tolist() == [list(s) for s in jitter.draw(5, sets[-1], 120)]
    assert flip.flags.tolist() == [int(f) for f in flip.draw(5, 2)]


def test_fp16_scaler_and_segmented_steps_replay_with_changing_sizes():
    from pytorch_retinanet_amd.graph import CapturedTrainStep, retinanet_stage_of
    from pytorch_retinanet_amd.parallel import BucketedGradAllReduce
    sets = [[FIRST[i % 4], SECOND[(i + 2) % 4]] for i in range(5)]
    data = _size_batches(sets, [[3, 9], [1, 16], [12, 0], [10, 11], [2, 29]], seed=3)          # all in class 32
    net, opt = _setup96(dtype=torch.float16)
    step = CapturedTrainStep(net, opt, amp_dtype=torch.float16, eager_steps=2, scaler=torch.amp.GradScaler("cuda"), gt_capacity="auto",
                             image_capacity="auto")
    l16 = [float(step(im, tg)["loss"]) for im, tg in data]
    assert step.captures == 1 and step.replays == 3 and np.all(np.isfinite(l16))
    net, opt = _setup96()
    ddp = BucketedGradAllReduce(net, stage_of=retinanet_stage_of)        # world 1, no process group
    step = CapturedTrainStep(net, opt, ddp=ddp, amp_dtype=torch.bfloat16, eager_steps=2, gt_capacity="auto", image_capacity="auto")
    assert step.segmented
    ls = [float(step(im, tg)["loss"]) for im, tg in data]
    assert step.captures == 1 and step.replays == 3 and np.all(np.isfinite(ls))


def test_simple_trainer_replays_batches_with_varying_image_sizes():
    import pytorch_retinanet_amd as P

    class Cropped(torch.utils.data.Dataset):
        "Every image cropped to its own landscape size (boxes clipped to it), 1..8 boxes each: one canvas class, one GT class."
        def __init__(self, ds):
            self.ds = ds

        def __len__(self):
            return len(self.ds)

        def __getitem__(self, i):
            img, t, idx = self.ds[i]
            h, w = 128 - 8 * (i % 5), 160 - 6 * (i % 7)
            n = (i * 5) % 8 + 1
            lim = torch.tensor([w - 1.0, h - 1.0, w, h])
            boxes = torch.minimum(t["boxes"][:n], lim)
            boxes[:, 2:] = torch.maximum(boxes[:, 2:], boxes[:, :2] + 1.0)
            return img[:, :h, :w].contiguous(), {**t, "boxes": boxes, "labels": t["labels"][:n]}, idx
    torch.manual_seed(7)
    conf = P.load_hparams()
    conf.model.update(backbone_kind="resnet18", pretrained=False, num_classes=5, min_size=96, max_size=120)
    conf.dataset.kind = "synthetic"
    conf.dataset.update(length=12, height=128, width=160, boxes_per_image=8)
    conf.dataloader.train_bs = 2
    conf.dataloader.valid_bs = 2
    conf.dataloader.args.pin_memory = False
    model = P.RetinaNetModel(conf)
    model.prepare_data()
    model.trn_ds, model.val_ds = Cropped(model.trn_ds), None
    assert len({tuple(model.trn_ds[i][0].shape) for i in range(12)}) == 12           # twelve different sizes
    trainer = P.SimpleTrainer(max_epochs=1, device=DEV, gt_capacity="auto", image_capacity="auto")
    steps = trainer.fit(model)
    assert steps == 6 and trainer.captured_steps == 4 and trainer.captured_graphs == 1, (steps, trainer.captured_steps, trainer.captured_graphs)
    assert bool(torch.isfinite(model.net.retinanet_head.classification_head.class_subnet_output.bias.float()).all())
