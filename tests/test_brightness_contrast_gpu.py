"""GPU: ``augment.RandomBrightnessContrast`` on the device -- the draw (``rn_brightness_contrast_draw``) against its Python restatement,
the image mean (``rn_brightness_contrast_mean``) against the fp64 mean of the restated image, the application inside the transform
kernel bit for bit against ``rn_transform_batch`` on the restated images, the transform module with every augmentation installed, and
``CapturedTrainStep`` replaying one graph with a new draw each time.

The restatement is ``augment.apply_color_ops`` followed by ``augment.apply_brightness_contrast`` (torch fp32 on the CPU).  Every
operation of the chain is one correctly rounded fp32 operation and contraction is off, so the application tests ask for equal bits."""
import numpy as np
import pytest
import torch

from test_color_jitter import MEAN, STD, order_of, special_image

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 23
PRESENT, PENDING = 1 << 16, 1 << 17
IDENTITY = ((1.0, 1.0, 1.0, 0.0), 0xFFFF, 0.0)
F32 = np.float32


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _coef(rows):
    "rows of (factors, order word, mean, bc_mul, bc_add) -> the f32 [B, 8] ``rn_color_coef`` tensor on the device."
    raw = np.zeros((len(rows), 8), np.float32)
    for b, (fac, order, mean, mul, add) in enumerate(rows):
        raw[b, :4] = np.asarray(fac, np.float32)
        raw[b, 4] = np.float32(mean)
        raw[b, 5:6].view(np.int32)[0] = order
        raw[b, 6], raw[b, 7] = np.float32(mul), np.float32(add)
    return torch.from_numpy(raw).to(DEV)


def _rows(coef):
    "The device rows back on the host: [(factors tuple, order word, mean, bc_mul, bc_add)]."
    raw = coef.cpu().numpy()
    return [(tuple(float(v) for v in r[:4]), int(r[5:6].view(np.int32)[0]), float(r[4]), float(r[6]), float(r[7])) for r in raw]


def _ulp_apart(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def _want_rows(draws, by_max, colour):
    "What the draw leaves in the rows: ``colour`` = per image (factors, order, mean) of the colour part."
    out = []
    for (on, alpha, beta), (fac, order, mean) in zip(draws, colour):
        bits = (PRESENT | (0 if by_max else PENDING)) if on else 0
        out.append((fac, order | bits, mean, alpha if on else 1.0, beta if on else 0.0))
    return out


# ---- 1. the draw ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 64, 65])
@pytest.mark.parametrize("fresh", [1, 0], ids=["fresh", "behind-a-jitter"])
@pytest.mark.parametrize("by_max", [True, False], ids=["by-max", "by-mean"])
def test_draw_equals_the_restatement_bit_for_bit_and_advances_the_counter(B, fresh, by_max):
    from pytorch_retinanet_amd import draw_state, ops
    from pytorch_retinanet_amd.augment import ColorJitter, RandomBrightnessContrast
    lay = draw_state.BRIGHTNESS_CONTRAST
    bc = RandomBrightnessContrast(0.3, (-0.1, 0.5), brightness_by_max=by_max, p=0.6, seed=SEED)
    block = draw_state.new(lay, torch.device(DEV), seed=SEED, counter=0, p=0.6, brightness=bc.brightness_limit, contrast=bc.contrast_limit,
                           by_max=by_max)
    assert draw_state.read(lay, block) == (SEED, 0, float(F32(0.6)), bc.brightness_limit, bc.contrast_limit, by_max)
    cj = ColorJitter(brightness=0.4, contrast=0.4, saturation=0.5, hue=0.1, p=0.8, seed=5)
    cj_block = draw_state.new(draw_state.COLOR_JITTER, torch.device(DEV), seed=5, counter=0, **cj._fields())
    seen = set()
    for k in range(3):
        if fresh:
            coef, colour = ops.brightness_contrast_draw(block, B), [IDENTITY] * B
        else:
            before = ops.color_jitter_draw(cj_block, B)
            before[:, 4] = 0.375                                                  # (a contrast mean: it must survive)
            colour = [(f, o, m) for f, o, m, _, _ in _rows(before)]
            assert [(f, o) for f, o, _ in colour] == cj.draw(k, B)
            coef = ops.brightness_contrast_draw(block, B, before)
            assert coef is before
        assert coef.shape == (B, 8) and coef.dtype == torch.float32
        draws = bc.draw(k, B)
        assert _rows(coef) == _want_rows(draws, by_max, colour), k                # fp32 values as Python floats: equal = equal bits
        seen |= {on for on, _, _ in draws}
        assert draw_state.read(lay, block)[1] == k + 1                            # the counter = the number of calls
    assert B < 3 or seen == {True, False}


def test_rewritten_p_and_limits_change_the_next_draw_without_a_new_object():
    from pytorch_retinanet_amd.augment import RandomBrightnessContrast
    images = [torch.rand(3, 5, 4, device=DEV) for _ in range(6)]
    bc, twin = RandomBrightnessContrast(seed=SEED), RandomBrightnessContrast(seed=SEED)
    colour = [IDENTITY] * 6
    assert _rows(bc.next_coef(images)) == _want_rows(twin.draw(0, 6), True, colour)
    block = bc._block
    bc.set_limits(brightness_limit=(0.25, 0.25), contrast_limit=0.6)
    twin.set_limits(brightness_limit=(0.25, 0.25), contrast_limit=0.6)
    rows = _rows(bc.next_coef(images))
    assert rows == _want_rows(twin.draw(1, 6), True, colour) != _want_rows(RandomBrightnessContrast(seed=SEED).draw(1, 6), True, colour)
    bc.p = 1.0
    assert all(o == 0xFFFF | PRESENT and add == 0.25 for _, o, _, _, add in _rows(bc.next_coef(images)))
    bc.p = 0.0
    assert all((o, mul, add) == (0xFFFF, 1.0, 0.0) for _, o, _, mul, add in _rows(bc.next_coef(images)))
    assert bc._block is block and bc.counter == 4
    with pytest.raises(ValueError, match="brightness_by_max"):
        bc.brightness_by_max = False                                              # which kernels a step launches: fixed with the block
    bc.brightness_by_max = True
    state = bc.state_dict()
    other = RandomBrightnessContrast()
    other.next_coef(images)
    other.load_state_dict(state)
    assert other.counter == 4 and _rows(other.next_coef(images)) == _rows(bc.next_coef(images))
    with pytest.raises(RuntimeError, match="GPU"):
        bc.next_coef([im.cpu() for im in images])


# ---- 2. the image mean ------------------------------------------------------------------------------------------------
MEAN_SHAPES = [(1, 1), (7, 5), (37, 53), (91, 91)]                                # 91 * 91 = 8281 pixels: past one 8192-pixel round
FACTORS = (1.3, 0.7, 1.6, -0.2)
# alone, behind an order without a contrast, and behind two with one (first, and after two other operations)
MEAN_ORDERS = [0xFFFF, order_of([3, 0, 2]), order_of([1, 0]), order_of([2, 0, 1, 3])]
BETA = -0.3125


def _restated(x, factors, order):
    from pytorch_retinanet_amd.augment import apply_color_ops
    return apply_color_ops(x, factors, order)


@pytest.fixture(scope="module")
def mean_case():
    "One batch for the mean tests: every shape under every order, pending and not, and the restated image of each."
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.augment import color_mean_of, order_ops
    images, rows, restated = [], [], []
    for k, (order, (h, w)) in enumerate((o, s) for o in MEAN_ORDERS for s in MEAN_SHAPES):
        x = special_image(h, w, seed=k)
        pre = x
        for op in order_ops(order):                                               # the contrast's own mean, as rn_color_mean would leave it
            if op == 1:
                break
            pre = _restated(pre, FACTORS, order_of([op]))
        mean = color_mean_of(pre) if 1 in order_ops(order) else 0.0
        images.append(x)
        rows.append((FACTORS, order | PRESENT | PENDING, mean, 1.25, BETA))
        restated.append(apply_with_mean(x, order, mean))
    for k, (h, w) in enumerate(MEAN_SHAPES[:2]):                                  # two rows that are not pending: left as they are
        images.append(special_image(h, w, seed=50 + k))
        rows.append((FACTORS, 0xFFFF | (PRESENT if k else 0), 0.0, 0.5, 0.125))
        restated.append(None)
    dev_images = [x.to(DEV) for x in images]
    coef, ref = ops.brightness_contrast_mean(dev_images, _coef(rows), return_ref=True)
    return images, dev_images, rows, restated, coef, ref.cpu().numpy().copy()


def apply_with_mean(x, order, mean):
    from pytorch_retinanet_amd.augment import apply_color_ops
    return apply_color_ops(x, FACTORS, order & 0xFFFF, mean)


def test_ref_is_within_one_ulp_of_the_fp64_mean_and_bc_add_is_beta_times_it(mean_case):
    _, _, rows, restated, coef, ref = mean_case
    worst = 0
    for b, ((fac, order, mean, mul, add), img, got) in enumerate(zip(rows, restated, _rows(coef))):
        if img is None:
            assert got == (tuple(float(F32(v)) for v in fac), order, mean, mul, add)        # not pending: no bit of the row changes
            continue
        want = F32(float(img.to(torch.float64).sum()) / float(img.numel()))
        worst = max(worst, _ulp_apart(ref[b], want))
        assert got[:4] == (tuple(float(F32(v)) for v in fac), order & ~PENDING, float(F32(mean)), mul), b
        assert F32(got[4]).tobytes() == (F32(BETA) * F32(ref[b])).astype(F32).tobytes(), b
    print("worst distance of ref from fp32(fp64 mean), ulp:", worst)
    assert worst <= 1


def test_a_second_call_changes_no_bit_and_the_staged_form_gives_the_same_bits(mean_case):
    from pytorch_retinanet_amd import ops
    _, dev_images, rows, _, coef, ref = mean_case
    again = coef.clone()
    assert ops.brightness_contrast_mean(dev_images, again) is again and torch.equal(_bits(again), _bits(coef))
    staged = ops.image_stage(dev_images, ops.new_image_arena(len(dev_images), 3 * 91 * 91 + 5, torch.device(DEV)))
    by_var, ref_var = ops.brightness_contrast_mean(staged, _coef(rows), return_ref=True)
    assert torch.equal(_bits(by_var), _bits(coef))
    n = len(MEAN_ORDERS) * len(MEAN_SHAPES)
    assert np.array_equal(ref_var.cpu().numpy()[:n].view(np.int32), ref[:n].view(np.int32))
    # a size no slot can hold (device data): nothing is read, ref = 0, bc_add = beta * 0
    staged.in_hw[1] = torch.tensor([2048, 2048], dtype=torch.int32)
    staged.in_hw[6] = torch.tensor([0, 5], dtype=torch.int32)
    got, ref0 = ops.brightness_contrast_mean(staged, _coef(rows), return_ref=True)
    got, ref0 = _rows(got), ref0.cpu().numpy()
    for b in (1, 6):
        assert ref0[b] == 0.0 and got[b][4] == 0.0 and not got[b][1] & PENDING
    assert got[2] == _rows(coef)[2]


def test_mean_past_the_launch_table_and_workspace_checks():
    from pytorch_retinanet_amd import _lib, ops
    images = [special_image(3, 4, seed=k).to(DEV) for k in range(65)]
    rows = [(FACTORS, order_of([0]) | PRESENT | PENDING, 0.0, 1.0, 0.5 + 0.001 * k) for k in range(65)]
    coef, ref = ops.brightness_contrast_mean(images, _coef(rows), return_ref=True)
    got, ref = _rows(coef), ref.cpu().numpy()
    for b in (0, 63, 64):
        img = _restated(images[b].cpu(), FACTORS, order_of([0]))
        assert _ulp_apart(ref[b], F32(float(img.to(torch.float64).sum()) / float(img.numel()))) <= 1, b
        assert F32(got[b][4]).tobytes() == (F32(rows[b][4]) * F32(ref[b])).astype(F32).tobytes() and not got[b][1] & PENDING, b
    need = int(_lib.lib.rn_brightness_contrast_mean_workspace_bytes(65))
    short = torch.empty(need - 1, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.RetinanetHipError, match="rn_brightness_contrast_mean"):
        ops.brightness_contrast_mean(images, _coef(rows), workspace=short)


def test_a_by_max_object_never_launches_the_mean():
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.augment import RandomBrightnessContrast
    images = [torch.rand(3, 6, 6, device=DEV) for _ in range(2)]
    called = []
    real = ops.brightness_contrast_mean
    ops.brightness_contrast_mean = lambda *a, **k: called.append(1) or real(*a, **k)
    try:
        RandomBrightnessContrast(p=1.0).next_coef(images)
        assert not called
        rows = _rows(RandomBrightnessContrast(p=1.0, brightness_by_max=False).next_coef(images))
        assert called and all(o == 0xFFFF | PRESENT for _, o, _, _, _ in rows)      # the pending bit is cleared by then
    finally:
        ops.brightness_contrast_mean = real


# ---- 3. the application -----------------------------------------------------------------------------------------------
APP_SHAPES = [(16, 24), (16, 24), (9, 13), (16, 24), (20, 11)]                  # out: (16, 24) for all: identity and real resizes
APP_OUT = [(16, 24)] * 5
ORDERS5 = [(0, 1, 2, 3), (3, 2, 1, 0), (1, 3, 0, 2), (2, 0, 3, 1), (3, 0, 1, 2)]
# (alpha, beta, ref): ordinary ones, one that clamps much of the image at 0 and one at 1, a by-mean reference
BC5 = [(1.25, 0.1, 1.0), (0.7, -0.15, 1.0), (1.9, -0.6, 1.0), (0.4, 0.8, 1.0), (1.1, 0.3, None)]


def _app(shapes, orders, bcs, factors=FACTORS, seed=0, present=True):
    "-> images, rows and the restated images: apply_color_ops, then apply_brightness_contrast (by-mean: the restatement's own mean)."
    from pytorch_retinanet_amd.augment import apply_brightness_contrast, apply_color_ops, image_mean_of
    images, rows, restated = [], [], []
    for k, ((h, w), order, (alpha, beta, ref)) in enumerate(zip(shapes, orders, bcs)):
        x = special_image(h, w, seed=seed + k)
        pre, mean = x, 0.0
        for op in [(order >> (4 * j)) & 0xF for j in range(4)]:
            if op == 1:
                from pytorch_retinanet_amd.augment import color_mean_of
                mean = color_mean_of(pre)
                break
            if op != 0xF:
                pre = apply_color_ops(pre, factors, order_of([op]))
        y = apply_color_ops(x, factors, order, mean)
        r = image_mean_of(y) if ref is None else ref
        add = float(F32(beta) * F32(r))
        images.append(x)
        rows.append((factors, order | (PRESENT if present else 0), mean, alpha, add))
        restated.append(apply_brightness_contrast(y, alpha, beta, r) if present else y)
    return images, rows, restated


def _check(images, rows, restated, out_sizes, hp, wp, dtype=torch.float32, channels_last=False, flags=None):
    from pytorch_retinanet_amd import ops
    dev = [x.to(DEV) for x in images]
    got = ops.transform_batch(dev, out_sizes, MEAN, STD, hp, wp, dtype, channels_last, flags=flags, coef=_coef(rows))
    want = ops.transform_batch([x.to(DEV) for x in restated], out_sizes, MEAN, STD, hp, wp, dtype, channels_last, flags=flags)
    assert torch.equal(_bits(got), _bits(want))
    return dev, got


@pytest.mark.parametrize("orders", [[()] * 5, ORDERS5], ids=["alone", "behind-all-four"])
@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
def test_application_equals_the_plain_transform_of_the_restated_images(orders, flip):
    flags = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8, device=DEV) if flip else None
    images, rows, restated = _app(APP_SHAPES, [order_of(o) for o in orders], BC5)
    assert all(not torch.equal(a, b) for a, b in zip(images, restated))
    assert bool((restated[2] == 0.0).sum() > 30) and bool((restated[3] == 1.0).sum() > 30)        # the clamps at both ends are exercised
    _check(images, rows, restated, APP_OUT, 32, 32, flags=flags)


@pytest.mark.parametrize("dtype, channels_last", [(torch.float32, False), (torch.bfloat16, True), (torch.float16, False)],
                         ids=["f32-nchw", "bf16-nhwc", "f16-nchw"])
def test_application_in_every_output_form_and_with_device_sizes(dtype, channels_last):
    from pytorch_retinanet_amd import ops
    flags = torch.tensor([0, 1, 1, 0, 1], dtype=torch.uint8, device=DEV)
    images, rows, restated = _app(APP_SHAPES, [order_of(o) for o in ORDERS5], BC5, seed=20)
    dev, got = _check(images, rows, restated, APP_OUT, 32, 32, dtype, channels_last, flags)
    assert got.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    out_hw = torch.tensor(APP_OUT, dtype=torch.int32, device=DEV)
    coef = _coef(rows)
    by_dev = ops.transform_batch_dev(dev, out_hw, MEAN, STD, 32, 32, dtype, channels_last, flags=flags, coef=coef)
    staged = ops.image_stage(dev, ops.new_image_arena(5, 1024, torch.device(DEV)))
    by_var = ops.transform_batch_var(staged, out_hw, MEAN, STD, 32, 32, dtype, channels_last, flags=flags, coef=coef)
    assert torch.equal(_bits(by_dev), _bits(got)) and torch.equal(_bits(by_var), _bits(got))


def test_rows_with_the_bit_clear_give_the_plain_colour_result():
    "bc_mul / bc_add are not read without bit 16, whatever they hold."
    images, rows, restated = _app(APP_SHAPES, [order_of(o) for o in ORDERS5], BC5, present=False)
    assert all(not o & PRESENT for _, o, _, _, _ in rows) and any(mul != 0.0 for _, _, _, mul, _ in rows)
    dev, got = _check(images, rows, restated, APP_OUT, 32, 32)
    zeroed = [(f, o, m, 0.0, 0.0) for f, o, m, _, _ in rows]                     # the rows rn_color_jitter_draw writes
    from pytorch_retinanet_amd import ops
    assert torch.equal(_bits(got), _bits(ops.transform_batch(dev, APP_OUT, MEAN, STD, 32, 32, coef=_coef(zeroed))))


def test_the_second_launch_reads_its_own_coefficients():
    "B = 65: image 64 is the second launch's first; its coefficients are row 64's."
    shapes = [(4, 4)] * 65
    bcs = [(0.5 + 0.02 * k, -0.3 + 0.01 * k, 1.0) for k in range(65)]
    images, rows, restated = _app(shapes, [order_of(ORDERS5[k % 5]) for k in range(65)], bcs)
    _check(images, rows, restated, [(4, 4)] * 65, 4, 4)


# ---- 4. the transform module ------------------------------------------------------------------------------------------
SHAPES = [(24, 40), (33, 21), (40, 40), (17, 30)]
SIZES = (24, 32)


def _module():
    from pytorch_retinanet_amd.augment import RandomHorizontalFlip, RandomShortSide
    from pytorch_retinanet_amd.transform import GeneralizedRCNNTransform
    t = GeneralizedRCNNTransform(SIZES, 48, MEAN, STD, size_divisible=32).train()
    t.hflip = RandomHorizontalFlip(0.5, seed=3)
    t.scale_jitter = RandomShortSide(SIZES, seed=4)
    return t


@pytest.mark.parametrize("staged", [False, True], ids=["list", "staged"])
@pytest.mark.parametrize("by_max", [True, False], ids=["by-max", "by-mean"])
def test_whole_path_equals_the_restatement_with_every_augmentation_installed(staged, by_max):
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.augment import ColorJitter, RandomBrightnessContrast, apply_brightness_contrast, apply_color_ops
    images = [special_image(h, w, seed=30 + k) for k, (h, w) in enumerate(SHAPES)]
    boxes = [torch.tensor([[2.0, 3.0, 15.0, 16.0]]) for _ in SHAPES]
    labels = [torch.tensor([1]) for _ in SHAPES]
    t, plain = _module(), _module()
    cj = t.color_jitter = ColorJitter(brightness=0.4, contrast=0.4, saturation=0.5, hue=0.1, p=0.8, seed=17)
    bc = t.brightness_contrast = RandomBrightnessContrast(0.3, 0.4, brightness_by_max=by_max, p=0.7, seed=SEED)
    seen = set()
    for k in range(3):
        def inputs(ims):
            dev = [x.to(DEV) for x in ims]
            if not staged:
                return dev, [{"boxes": b.to(DEV), "labels": l.to(DEV)} for b, l in zip(boxes, labels)], {}
            gt = ops.gt_stage([b.to(DEV) for b in boxes], [l.to(DEV) for l in labels], ops.PackedGT.empty(4, 2, torch.device(DEV)))
            return ops.image_stage(dev, ops.new_image_arena(4, 2048, torch.device(DEV))), gt, {"canvas": (64, 64)}
        im, tg, kw = inputs(images)
        got, _ = t(im, tg, **kw)
        assert bc.coef is cj.coef                                                 # one set of rows carries both
        rows, draws = _rows(bc.coef), bc.draw(k, 4)
        assert [(f, o & 0xFFFF) for f, o, _, _, _ in rows] == cj.draw(k, 4)       # the jitter's part: the Python draw, bit for bit
        restated = []
        for x, (fac, word, mean, mul, add), (on, alpha, beta) in zip(images, rows, draws):
            assert not word & PENDING and bool(word & PRESENT) == on and mul == (alpha if on else 1.0)
            y = apply_color_ops(x, fac, word & 0xFFFF, mean)                      # the restatement fed the device's coefficients
            if on and by_max:
                assert add == beta
            elif on:
                want_ref = F32(float(y.to(torch.float64).sum()) / float(y.numel()))
                near = [F32(beta) * r for r in (np.nextafter(want_ref, F32(0)), want_ref, np.nextafter(want_ref, F32(2)))]
                assert F32(add) in near                                           # beta times a ref within one ulp of fp32(fp64 mean)
            if on:
                t1 = (y.new_tensor(mul) * y + y.new_tensor(add)).clamp(0.0, 1.0)
                assert not by_max or torch.equal(t1, apply_brightness_contrast(y, alpha, beta, 1.0))
                y = t1
            restated.append(y)
        seen |= {on for on, _, _ in draws}
        im, tg, kw = inputs(restated)
        want, _ = plain(im, tg, **kw)
        assert torch.equal(_bits(got.tensors), _bits(want.tensors)), k
        assert bc.counter == cj.counter == k + 1
    assert seen == {True, False}


def test_eval_mode_and_missing_targets_leave_the_counter_and_the_image_alone():
    from pytorch_retinanet_amd.augment import RandomBrightnessContrast
    images = [special_image(h, w, seed=40 + k).to(DEV) for k, (h, w) in enumerate(SHAPES)]
    t, plain = _module(), _module()
    bc = t.brightness_contrast = RandomBrightnessContrast(p=1.0, seed=SEED)
    for train in (False, True):
        t.train(train), plain.train(train)
        torch.manual_seed(0)                       # (without targets the training transform draws its short side on the host)
        got, _ = t(images, None)
        torch.manual_seed(0)
        want, _ = plain(images, None)
        assert torch.equal(_bits(got.tensors), _bits(want.tensors))
    t.eval(), plain.eval()
    targets = [{"boxes": torch.tensor([[2.0, 3.0, 15.0, 16.0]], device=DEV), "labels": torch.tensor([1], device=DEV)} for _ in SHAPES]
    got, _ = t(images, [dict(x) for x in targets])
    want, _ = plain(images, [dict(x) for x in targets])
    assert torch.equal(_bits(got.tensors), _bits(want.tensors))
    assert bc.counter == 0 and bc.coef is None and bc._block is None


# ---- 5. the captured step ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by_max", [True, False], ids=["by-max", "by-mean"])
def test_captured_step_draws_anew_at_every_replay_and_equals_its_eager_twin(by_max):
    "The bars of tests/test_image_capacity_gpu.py's step tests: losses rtol 2e-2, parameters atol 2e-3."
    from pytorch_retinanet_amd.augment import RandomBrightnessContrast, RandomHorizontalFlip
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from test_graph_gpu import _setup
    from test_hflip_gpu import _const_batches
    data = _const_batches(5)
    res = {}
    for enabled in (False, True):
        net, opt = _setup()
        bc = net.transform.brightness_contrast = RandomBrightnessContrast(0.3, 0.3, brightness_by_max=by_max, p=0.8, seed=SEED)
        net.transform.hflip = RandomHorizontalFlip(p=0.5, seed=21)
        step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=2, enabled=enabled)
        losses, drawn = [], []
        for k, (images, targets) in enumerate(data):
            losses.append(float(step(images, targets)["loss"]))
            rows, draws = _rows(bc.coef), bc.draw(k, len(images))
            drawn.append([(bool(o & PRESENT), mul) for _, o, _, mul, _ in rows])
            assert drawn[-1] == [(on, alpha if on else 1.0) for on, alpha, _ in draws], (enabled, k)
            assert not any(o & PENDING for _, o, _, _, _ in rows)
            if by_max:
                assert [add for _, _, _, _, add in rows] == [beta if on else 0.0 for on, _, beta in draws]
        torch.cuda.synchronize()
        assert bc.counter == 5 and len({str(d) for d in drawn}) == 5
        res[enabled] = (np.array(losses), {n: (p.master if hasattr(p, "master") else p.data).detach().float().cpu()
                                           for n, p in net.named_parameters()}, step)
    step = res[True][2]
    assert step.captures == 1 and step.replays == 3, (step.captures, step.replays)
    assert res[False][2].captures == 0 and np.all(np.isfinite(res[True][0]))
    np.testing.assert_allclose(res[True][0], res[False][0], rtol=2e-2)
    for k, a in res[False][1].items():
        torch.testing.assert_close(res[True][1][k], a, rtol=0, atol=2e-3, msg=k)


def test_rewritten_limits_replay_the_same_graph_and_another_object_is_another_key():
    from pytorch_retinanet_amd.augment import RandomBrightnessContrast
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from test_graph_gpu import _setup
    from test_hflip_gpu import _const_batches
    net, opt = _setup()
    bc = net.transform.brightness_contrast = RandomBrightnessContrast(p=1.0, seed=SEED)
    step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=1)
    data = _const_batches(5, seed=8)
    for images, targets in data[:2]:
        step(images, targets)
    bc.set_limits(brightness_limit=(0.125, 0.125), contrast_limit=(0.5, 0.5))
    for images, targets in data[2:4]:
        out = step(images, targets)
        rows = _rows(bc.coef)
        assert all((mul, add) == (1.5, 0.125) for _, _, _, mul, add in rows) and np.isfinite(float(out["loss"]))
    assert step.captures == 1 and step.replays == 3 and bc.counter == 4
    key = step._signature(*data[4])
    assert ("brightness_contrast", bc) in key
    net.transform.brightness_contrast = RandomBrightnessContrast(p=1.0, seed=SEED)
    assert step._signature(*data[4]) != key
    net.transform.brightness_contrast = None
    assert not any(isinstance(k, tuple) and k and k[0] == "brightness_contrast" for k in step._signature(*data[4]))
