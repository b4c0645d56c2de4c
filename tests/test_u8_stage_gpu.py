"""GPU: uint8 images -- planes or interleaved, as image decoders give them -- staged into the fp32 arena by ``rn_image_stage_u8``
(``ops.image_stage_u8`` / ``ops.images_u8_to_f32``), and everything behind the arena fed that way: the transform, the augmentations,
``graph.CapturedTrainStep(image_capacity=...)`` and ``graph.CapturedPredict``.

Bars.  The converted value is ``float(v) / 255`` with one correctly rounded division; the reference is always numpy on the CPU
(``arr.astype(float32) / float32(255)``), compared bit for bit (``torch.equal`` / ``np.array_equal``; no value is NaN or -0).  What runs
behind the arena is the existing kernels on the same bits: ``torch.equal`` against the same call on an arena filled by
``ops.image_stage`` from the CPU-converted floats.  Whole train steps against an eager twin fed the converted floats: the tolerances of
``tests/test_gt_capacity_gpu.py`` (bf16 conv stack, atomically accumulated weight gradients).  ``CapturedPredict`` on uint8 batches against
``net.predict`` of the converted floats: the fp32 bars of ``tests/test_captured_predict_gpu.py`` (``predict`` does not repeat itself
bit for bit on this device).

The kernel's constants this file relies on (``csrc/transform.hip``): 64 images per launch, at most 256 blocks of 256 threads per image,
16 pixels per thread and step -- so one grid pass covers 256 * 256 * 16 = 1 048 576 pixels of an image."""
import numpy as np
import pytest
import torch

from test_image_capacity_gpu import GUARD, SENTINEL, _guarded_arena

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
PLANES, INTERLEAVED = 0, 1
ONE_GRID_PASS = 256 * 256 * 16                  # pixels (module docstring)
OFFSETS = [0, 1, 2, 3, 5, 15]                   # source bytes past a 16-byte boundary
SIZES = [(37, 53), (64, 40), (1, 7), (50, 50), (3, 6), (1, 1), (2, 9)]       # h w % 4 = 1, 0, 3, 0, 2, 1, 2; three below 16 pixels


def _ref(planes: np.ndarray) -> np.ndarray:
    "uint8 [3, h, w] -> the definition, on the CPU with numpy."
    assert planes.dtype == np.uint8
    return planes.astype(np.float32) / np.float32(255)


def _source(planes: np.ndarray, layout: int, offset: int = 0) -> torch.Tensor:
    """The image as a CUDA uint8 ``[3, h, w]`` tensor in the given layout, a view into a larger buffer whose first byte lies
    ``offset`` bytes past a 16-byte boundary."""
    _, h, w = planes.shape
    n = planes.size
    flat = planes.reshape(-1) if layout == PLANES else np.ascontiguousarray(planes.transpose(1, 2, 0)).reshape(-1)
    buf = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device=DEV)
    start = (-buf.data_ptr()) % 16 + offset
    view = buf[start:start + n]
    view.copy_(torch.from_numpy(flat.copy()))
    assert view.data_ptr() % 16 == offset % 16
    im = view.view(3, h, w) if layout == PLANES else view.view(h, w, 3).permute(2, 0, 1)
    assert tuple(im.shape) == (3, h, w) and (layout == PLANES or h * w == 1 or not im.is_contiguous())
    return im


def _random_planes(rng, h, w) -> np.ndarray:
    return rng.integers(0, 256, (3, h, w), dtype=np.uint8)


# ---- 1. all 256 values, both layouts ---------------------------------------------------------------------------------------------------
def test_every_byte_value_in_both_layouts():
    from pytorch_retinanet_amd import ops
    rng = np.random.default_rng(0)
    planes = np.stack([rng.permutation(256).astype(np.uint8).reshape(16, 16) for _ in range(3)])
    assert all(len(set(planes[c].reshape(-1).tolist())) == 256 for c in range(3)) and not np.array_equal(planes[0], planes[1])
    want = _ref(planes)
    table = np.arange(256, dtype=np.float32) / np.float32(255)
    assert np.array_equal(want[0].reshape(-1), table[planes[0].reshape(-1)])
    ims = [_source(planes, PLANES), _source(planes, INTERLEAVED)]
    staged = ops.image_stage_u8(ims, ops.new_image_arena(2, 256, torch.device(DEV)))
    conv = ops.images_u8_to_f32(ims)
    torch.cuda.synchronize()
    for b in range(2):
        got = staged.arena[b, :768].cpu().numpy().reshape(3, 16, 16)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), b
        assert conv[b].dtype == torch.float32 and conv[b].is_contiguous() and tuple(conv[b].shape) == (3, 16, 16)
        assert np.array_equal(conv[b].cpu().numpy().view(np.uint32), want.view(np.uint32)), b
    assert staged.in_hw.tolist() == [[16, 16], [16, 16]] and staged.hw == [(16, 16), (16, 16)]
    # the CPU branch of the same op gives the same bits
    assert all(np.array_equal(c.numpy().view(np.uint32), want.view(np.uint32)) for c in ops.images_u8_to_f32([im.cpu() for im in ims]))


# ---- 2. shapes and alignment in a guarded arena ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pix", [2601, 2560 + 64], ids=["odd-slot", "aligned-slot"])
def test_shapes_alignments_and_layouts_in_a_guarded_arena(pix):
    """Six batches into ONE arena: the sizes, the source offsets and the layouts rotate, so every size meets several offsets in both
    layouts, and every batch after the first overwrites the prefixes only.  The expected arena is kept on the CPU: sentinels where
    nothing was ever staged, the remains of earlier batches behind shorter images.  (slot = 3 x 2601 floats is odd: the slots, and with
    them the destination planes, start at every alignment; 3 x 2624 keeps every slot at 16 bytes.)"""
    from pytorch_retinanet_amd import ops
    B = len(SIZES)
    buf, hwbuf, staged = _guarded_arena(B, pix=pix)
    expect = np.full((B, staged.slot), SENTINEL, np.float32)
    rng = np.random.default_rng(1)
    for r in range(6):
        sizes = SIZES[r:] + SIZES[:r]
        layouts = [(b + r) % 2 for b in range(B)]
        offsets = [OFFSETS[(b + 2 * r) % 6] for b in range(B)]
        planes = [_random_planes(rng, h, w) for h, w in sizes]
        ims = [_source(p, lay, off) for p, lay, off in zip(planes, layouts, offsets)]
        assert ops.image_stage_u8(ims, staged) is staged
        torch.cuda.synchronize()
        for b, p in enumerate(planes):
            expect[b, :p.size] = _ref(p).reshape(-1)
        assert np.array_equal(staged.arena.cpu().numpy().view(np.uint32), expect.view(np.uint32)), r
        assert staged.in_hw.tolist() == [list(s) for s in sizes] and staged.hw == sizes and staged.bounds is None
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())
        assert bool((hwbuf[:16] == -99).all()) and bool((hwbuf[-16:] == -99).all())
    assert (expect[:, -1] == SENTINEL).all()                                   # (every slot kept a tail no batch reached)


# ---- 3. past the 64-image table ----------------------------------------------------------------------------------------------------------
def test_stage_crosses_the_64_image_launch_boundary():
    from pytorch_retinanet_amd import ops
    rng = np.random.default_rng(2)
    planes = [_random_planes(rng, 8, 12) for _ in range(65)]
    ims = [_source(p, b % 2, OFFSETS[b % 6]) for b, p in enumerate(planes)]
    buf, hwbuf, staged = _guarded_arena(65, pix=128)                           # (3 x 8 x 12 = 288 of 384 floats per slot)
    ops.image_stage_u8(ims, staged)
    conv = ops.images_u8_to_f32(ims)
    torch.cuda.synchronize()
    got = staged.arena.cpu().numpy()
    for b, p in enumerate(planes):
        assert np.array_equal(got[b, :288], _ref(p).reshape(-1)) and (got[b, 288:] == SENTINEL).all(), b
        assert np.array_equal(conv[b].cpu().numpy(), _ref(p)), b
    assert staged.in_hw.tolist() == [[8, 12]] * 65
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())
    assert bool((hwbuf[:16] == -99).all()) and bool((hwbuf[-16:] == -99).all())


# ---- 4. past one grid pass ----------------------------------------------------------------------------------------------------------------
def test_an_image_above_one_grid_pass_in_both_layouts():
    "1030 x 1031 = 1 061 930 pixels > 1 048 576: the grid-stride loop takes a second turn (odd pixel count, sources at odd addresses)."
    from pytorch_retinanet_amd import ops
    h, w = 1030, 1031
    assert h * w > ONE_GRID_PASS and (h * w) % 4 == 2
    planes = _random_planes(np.random.default_rng(3), h, w)
    want = torch.from_numpy(_ref(planes).reshape(-1)).to(DEV)
    buf, hwbuf, staged = _guarded_arena(2, pix=h * w + 5)
    ops.image_stage_u8([_source(planes, PLANES, 1), _source(planes, INTERLEAVED, 5)], staged)
    torch.cuda.synchronize()
    n = 3 * h * w
    for b in range(2):
        assert torch.equal(staged.arena[b, :n].view(torch.int32), want.view(torch.int32)), b
        assert bool((staged.arena[b, n:] == SENTINEL).all()), b
    assert staged.in_hw.tolist() == [[h, w], [h, w]]
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


# ---- 5. the wrappers' refusals ------------------------------------------------------------------------------------------------------------
def test_wrapper_refusals_write_nothing_and_other_strides_are_made_dense():
    from pytorch_retinanet_amd import ops
    rng = np.random.default_rng(4)
    planes = [_random_planes(rng, h, w) for h, w in SIZES[:4]]
    ims = [_source(p, b % 2) for b, p in enumerate(planes)]
    buf, hwbuf, staged = _guarded_arena(4, pix=2600)
    before = buf.clone()
    u8 = dict(dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="uint8"):
        ops.image_stage_u8(ims[:3] + [torch.rand(3, 8, 8, device=DEV)], staged)                        # fp32 input
    with pytest.raises(ValueError, match="uint8"):
        ops.image_stage_u8(ims[:3] + [torch.zeros(8, 8, 3, **u8)], staged)                             # [h, w, 3] shape
    with pytest.raises(ValueError, match="uint8"):
        ops.image_stage_u8(ims[:3] + [torch.zeros(1, 3, 8, 8, **u8)], staged)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.image_stage_u8(ims[:3] + [torch.zeros(3, 8, 8, dtype=torch.uint8)], staged)
    with pytest.raises(ValueError, match="slots"):
        ops.image_stage_u8(ims[:3], staged)
    with pytest.raises(ValueError, match="does not fit"):
        ops.image_stage_u8(ims[:3] + [torch.zeros(3, 51, 51, **u8)], staged)                           # 2601 pixels > 2600
    with pytest.raises(ValueError, match="does not fit"):
        ops.image_stage_u8(ims[:3] + [torch.zeros(3, 0, 5, **u8)], staged)
    with pytest.raises(ValueError, match="bounds"):
        ops.image_stage_u8(ims, staged, bounds=[(4, 4)])
    with pytest.raises(ValueError, match="uint8"):
        ops.images_u8_to_f32(ims[:3] + [torch.rand(3, 8, 8, device=DEV)])
    with pytest.raises(ValueError, match="empty"):
        ops.images_u8_to_f32(ims[:3] + [torch.zeros(3, 0, 5, **u8)])
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and bool((hwbuf == -99).all()) and staged.hw == []                  # nothing ran
    # any other strides: made dense by the wrapper, the right bits
    wide = torch.from_numpy(_random_planes(rng, 50, 100)).to(DEV)
    odd = [wide[:, :, ::2], wide.transpose(1, 2)[:, :50, :50], ims[2], wide[:, 3:40, 7:60]]
    assert not any(x.is_contiguous() for x in (odd[0], odd[1], odd[3]))
    ops.image_stage_u8(odd, staged, bounds=[(1, 1)] * 4)
    conv = ops.images_u8_to_f32(odd)
    torch.cuda.synchronize()
    for b, x in enumerate(odd):
        want = _ref(np.ascontiguousarray(x.cpu().numpy()))
        assert np.array_equal(staged.arena[b, :want.size].cpu().numpy(), want.reshape(-1)), b
        assert np.array_equal(conv[b].cpu().numpy(), want), b
    assert staged.bounds == [(1, 1)] * 4 and staged.hw == [(50, 50), (50, 50), (1, 7), (37, 53)]
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


# ---- 6. downstream is untouched ------------------------------------------------------------------------------------------------------------
T_SHAPES = [(24, 40), (33, 21), (40, 40), (17, 30)]


def _module(augmented: bool):
    from pytorch_retinanet_amd.augment import ColorJitter, RandomBrightnessContrast, RandomHorizontalFlip
    from pytorch_retinanet_amd.transform import GeneralizedRCNNTransform
    t = GeneralizedRCNNTransform(24, 48, MEAN, STD, size_divisible=32).train()
    if augmented:
        t.hflip = RandomHorizontalFlip(0.5, seed=3)
        t.color_jitter = ColorJitter(brightness=0.4, contrast=0.4, saturation=0.5, hue=0.1, p=0.8, seed=17)
        t.brightness_contrast = RandomBrightnessContrast(0.3, 0.4, brightness_by_max=False, p=0.7, seed=9)
    return t


@pytest.mark.parametrize("augmented", [False, True], ids=["plain", "flip-jitter-bc"])
def test_the_transform_behind_the_arena_sees_the_same_bits(augmented):
    from pytorch_retinanet_amd import ops
    rng = np.random.default_rng(6)
    planes = [_random_planes(rng, h, w) for h, w in T_SHAPES]
    u8 = [_source(p, b % 2, OFFSETS[b]) for b, p in enumerate(planes)]
    f32 = [torch.from_numpy(_ref(p)).to(DEV) for p in planes]                   # converted on the CPU
    boxes = [torch.tensor([[2.0, 3.0, 15.0, 16.0], [1.0, 1.0, 12.0, 9.0]]) for _ in T_SHAPES]
    labels = [torch.tensor([1, 2]) for _ in T_SHAPES]
    dev = torch.device(DEV)

    def packed():
        return ops.gt_stage([b.to(DEV) for b in boxes], [l.to(DEV) for l in labels], ops.PackedGT.empty(4, 2, dev))

    def dicts():
        return [{"boxes": b.to(DEV), "labels": l.to(DEV)} for b, l in zip(boxes, labels)]
    a, b = _module(augmented), _module(augmented)
    for k in range(2):
        # staged: image_stage_u8 against image_stage of the converted floats
        got, got_t = a(ops.image_stage_u8(u8, ops.new_image_arena(4, 2048, dev)), packed(), canvas=(64, 64))
        want, want_t = b(ops.image_stage(f32, ops.new_image_arena(4, 2048, dev)), packed(), canvas=(64, 64))
        assert torch.equal(got.tensors.view(torch.int32), want.tensors.view(torch.int32)), k
        assert torch.equal(got_t.gt_boxes, want_t.gt_boxes) and got.image_sizes == want.image_sizes
        # an unstaged CUDA uint8 list: converted by the transform (without the feature it is normalised as 0..255 values)
        got, got_t = a(list(u8), dicts())
        want, want_t = b(list(f32), dicts())
        assert got.tensors.dtype == torch.float32 and torch.equal(got.tensors.view(torch.int32), want.tensors.view(torch.int32)), k
        assert all(torch.equal(x["boxes"], y["boxes"]) for x, y in zip(got_t, want_t)) and got.image_sizes == want.image_sizes
    assert float(want.tensors.abs().max()) < 3.0 and bool(want.tensors.any())
    # a mixed list converts its uint8 members one by one
    a.eval(), b.eval()
    got, _ = a([u8[0], f32[1], u8[2], f32[3]], None)
    want, _ = b(list(f32), None)
    assert torch.equal(got.tensors, want.tensors)


# ---- 7. whole train steps -------------------------------------------------------------------------------------------------------------------
def _u8_batches(size_sets, count_sets, seed):
    "One batch per entry -> (uint8 planes per image (numpy), targets): boxes inside their image."
    from test_gt_capacity_gpu import _gt
    rng = np.random.default_rng(seed)
    out = []
    for sizes, counts in zip(size_sets, count_sets):
        planes = [_random_planes(rng, h, w) for h, w in sizes]
        targets = []
        for (h, w), c in zip(sizes, counts):
            bx, lb = _gt(rng, [c], H=h, W=w)
            targets.append({"boxes": bx[0], "labels": lb[0]})
        out.append((planes, targets))
    return out


def test_uint8_and_fp32_batches_share_one_captured_graph():
    """Three fp32 batches (two eager steps and the capture), then five uint8 batches of other sizes in the same classes, layouts mixed
    within a batch: they replay the fp32 batches' graph.  The eager twin (both modes off) is fed the CPU-converted floats throughout."""
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from test_gt_capacity_gpu import _params
    from test_image_capacity_gpu import COUNTS32, FIRST, SECOND, _setup96
    data = _u8_batches([[FIRST[i % 4], SECOND[i % 4]] for i in range(8)], COUNTS32, seed=5)
    floats = [[torch.from_numpy(_ref(p)).to(DEV) for p in planes] for planes, _ in data]
    res = {}
    for on in (False, True):
        net, opt = _setup96()
        step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=2, enabled=on, gt_capacity="auto" if on else None,
                                 image_capacity="auto" if on else None)
        losses, captures = [], []
        for i, (planes, tg) in enumerate(data):
            as_u8 = on and i >= 3
            ims = [_source(p, (b + i) % 2, OFFSETS[(b + i) % 6]) for b, p in enumerate(planes)] if as_u8 else floats[i]
            losses.append(float(step(ims, tg)["loss"]))
            captures.append(step.captures)
        torch.cuda.synchronize()
        res[on] = (np.array(losses), _params(net), step, captures)
    assert np.all(np.isfinite(res[True][0]))
    np.testing.assert_allclose(res[True][0], res[False][0], rtol=2e-2)
    for k, v in res[False][1].items():
        torch.testing.assert_close(res[True][1][k], v, rtol=0, atol=2e-3, msg=k)
    step, captures = res[True][2], res[True][3]
    assert captures == [0, 0, 1, 1, 1, 1, 1, 1] and step.replays == 6 and res[False][2].replays == 0
    (key,) = list(step._entries)                                               # ONE key: the dtype entry is the arena's
    assert key[0] == ("img_cap", 2, (96, 128), 2 ** 16, torch.float32, torch.device(DEV)) and key[1] == ("gt_cap", 32)


def test_a_uint8_batch_no_class_holds_takes_the_exact_shape_path():
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from test_image_capacity_gpu import _setup96
    net, opt = _setup96()
    step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=1, gt_capacity="auto", image_capacity=[(96, 128)])
    (planes, tg), = _u8_batches([[(160, 128), (150, 100)]], [[3, 5]], seed=9)   # portrait: canvas 128 x 96, outside the class
    loss = float(step([_source(p, b % 2) for b, p in enumerate(planes)], tg)["loss"])
    (key,) = list(step._entries)
    assert np.isfinite(loss) and step.captures == 0 and step._entries[key].staged is None
    assert key[0] == tuple(((3, h, w), torch.uint8, torch.device(DEV)) for h, w in [(160, 128), (150, 100)])


# ---- 8. CapturedPredict -----------------------------------------------------------------------------------------------------------------------
# (every batch holds a portrait image, so its own canvas is 160 x 160: the class below, and net.predict's own canvas)
BATCHES_160 = [[(120, 150), (140, 128)], [(100, 140), (150, 128)], [(128, 160), (100, 90)], [(150, 120), (110, 150)]]


def test_captured_predict_replays_uint8_batches(golden):
    """An fp32 batch (the eager first call), then uint8 batches of other sizes in the same class, both layouts at odd source offsets:
    one key, one capture, every uint8 batch a replay, no fallback.  Detections against ``net.predict`` of the CPU-converted floats on
    the same canvas, at the fp32 bars of ``tests/test_captured_predict_gpu.py``.  (``_class_of`` called without ``u8=True`` classes
    fp32 batches only, as ``tests/test_captured_predict.py`` pins; ``__call__`` passes it.)"""
    from pytorch_retinanet_amd.graph import CapturedPredict
    from test_captured_predict_gpu import _cpu, _meets_fp32_bars, _nonempty
    from test_e2e_gpu import E2E, _model
    net = _model(golden("e2e.npz"), DEV, E2E).eval()
    p = CapturedPredict(net, [(160, 160)])
    rng = np.random.default_rng(8)
    for i, sizes in enumerate(BATCHES_160):
        planes = [_random_planes(rng, h, w) for h, w in sizes]
        f32 = [torch.from_numpy(_ref(q)).to(DEV) for q in planes]
        u8 = [_source(q, (b + i) % 2, OFFSETS[(2 * i + b) % 6 or 1]) for b, q in enumerate(planes)]
        batch = f32 if i == 0 else u8
        assert p._class_of(u8, u8=True) == p._class_of(f32) and p._class_of(f32)[0] == (160, 160) and p._class_of(u8) is None
        want = _cpu(net.predict(f32))
        got = p(batch)
        assert _nonempty(want) and _nonempty(got) and _meets_fp32_bars(got, want), i
        assert p.stats["fallbacks"] == 0 and p.stats["captures"] == min(i, 1) and p.stats["replays"] == i, (i, p.stats)
    assert p.stats == dict(p.stats, captures=1, replays=3, eager=1, fallbacks=0, invalidations=0), p.stats
    assert len(p._entries) == 1
    # a uint8 batch no class holds falls back to net.predict, whose transform converts it
    q = CapturedPredict(net, [(128, 160)])
    assert q._class_of(u8, u8=True) is None
    got = q(u8)
    assert q.stats == dict(q.stats, captures=0, replays=0, eager=0, fallbacks=1) and _nonempty(got) and _meets_fp32_bars(got, want)
