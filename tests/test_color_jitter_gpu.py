"""GPU: the colour jitter on the device -- the draw (``rn_color_jitter_draw``) against its Python restatement, the contrast mean
(``rn_color_mean``) against the fp64 mean of the restated image, the operations inside the transform kernel
(``rn_transform_batch_color``) bit for bit against ``rn_transform_batch`` on the restated jittered images, the transform module with
every augmentation installed, and ``CapturedTrainStep`` replaying one graph with a new draw each time.

The restatement is ``tests/test_color_jitter.py``'s (torch fp32 on the CPU, independent of the package).  Every operation of the chain
is one correctly rounded fp32 add, multiply, divide, compare, floor or select and contraction is off, so the application tests ask
for equal bits."""
import itertools

import numpy as np
import pytest
import torch

from test_color_jitter import MEAN, STD, order_of, restate, restate_mean64, restate_pre, special_image

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 17
RANGES = dict(brightness=0.4, contrast=0.4, saturation=0.5, hue=0.1)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _coef(rows):
    "rows of (factors, order, mean) -> the f32 [B, 8] ``rn_color_coef`` tensor on the device."
    raw = np.zeros((len(rows), 8), np.float32)
    for b, (fac, order, mean) in enumerate(rows):
        raw[b, :4] = np.asarray(fac, np.float32)
        raw[b, 4] = np.float32(mean)
        raw[b, 5:6].view(np.int32)[0] = order
    return torch.from_numpy(raw).to(DEV)


def _rows(coef):
    "The device rows back on the host: [(factors tuple, order, mean)]."
    raw = coef.cpu().numpy()
    return [(tuple(float(v) for v in r[:4]), int(r[5:6].view(np.int32)[0]), float(r[4])) for r in raw]


def _ulp_apart(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


# ---- 1. the draw ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 64, 65])
def test_draw_equals_the_restatement_bit_for_bit_and_advances_the_counter(B):
    from pytorch_retinanet_amd import draw_state, ops
    from pytorch_retinanet_amd.augment import ColorJitter
    cj = ColorJitter(p=0.8, seed=SEED, **RANGES)
    lo, hi = cj._lo_hi()
    block = draw_state.new(draw_state.COLOR_JITTER, torch.device(DEV), seed=SEED, counter=0, p=0.8, lo=lo, hi=hi, enabled_mask=0xF)
    assert draw_state.read(draw_state.COLOR_JITTER, block) == (SEED, 0, float(np.float32(0.8)), tuple(lo), tuple(hi), 0xF)
    for k in range(4):
        coef = ops.color_jitter_draw(block, B)
        assert coef.shape == (B, 8) and coef.dtype == torch.float32
        got, want = _rows(coef), cj.draw(k, B)
        assert [(f, o) for f, o, _ in got] == want, k                             # fp32 values as Python floats: equal = equal bits
        assert all(m == 0.0 for _, _, m in got) and not coef[:, 6:].any()
        assert draw_state.read(draw_state.COLOR_JITTER, block)[1] == k + 1                     # the counter = the number of calls


def test_rewritten_ranges_and_p_change_the_next_draw_without_a_new_object():
    from pytorch_retinanet_amd.augment import ColorJitter
    images = [torch.rand(3, 5, 4, device=DEV) for _ in range(6)]
    cj = ColorJitter(brightness=0.4, hue=0.1, seed=SEED)
    twin = ColorJitter(brightness=0.4, hue=0.1, seed=SEED)
    assert [(f, o) for f, o, _ in _rows(cj.next_coef(images))] == twin.draw(0, 6)
    block = cj._block
    cj.brightness = (0.9, 1.0)
    twin.brightness = (0.9, 1.0)
    assert [(f, o) for f, o, _ in _rows(cj.next_coef(images))] == twin.draw(1, 6) != ColorJitter(brightness=0.4, hue=0.1, seed=SEED).draw(1, 6)
    cj.p = 0.0
    assert all(o == 0xFFFF for _, o, _ in _rows(cj.next_coef(images)))
    cj.p = 1.0
    cj.hue = 0                                                                    # disabling is a block write; hue leaves the orders
    assert all(((o >> (4 * j)) & 0xF) != 3 for _, o, _ in _rows(cj.next_coef(images)) for j in range(4))
    assert cj._block is block and cj.counter == 4
    with pytest.raises(ValueError, match="disabled"):
        cj.contrast = 0.3                                                         # enabling what the block was built without
    state = cj.state_dict()
    other = ColorJitter(brightness=0.4, hue=0.1)
    other.next_coef(images)
    other.load_state_dict(state)
    assert other.counter == 4 and [(f, o) for f, o, _ in _rows(other.next_coef(images))] == [(f, o) for f, o, _ in _rows(cj.next_coef(images))]


# ---- 2. the contrast mean -----------------------------------------------------------------------------------------------
MEAN_SHAPES = [(1, 1), (7, 5), (37, 53)]
FACTORS = (1.3, 0.7, 1.6, -0.2)
# every set of operations that can precede the contrast (in some order each; hue and brightness first included), and two without one
PRE_ORDERS = [order_of(p + (1,) + tuple(sorted(set((0, 2, 3)) - set(p)))) for r in range(4) for p in itertools.permutations((0, 2, 3), r)]
NO_CONTRAST = [0xFFFF, order_of([3, 0, 2])]


@pytest.fixture(scope="module")
def mean_case():
    "One batch for the mean tests: every shape under every order, and the fp64 reference of each image."
    from pytorch_retinanet_amd import ops
    images, rows, want = [], [], []
    for k, (order, (h, w)) in enumerate(itertools.product(PRE_ORDERS + NO_CONTRAST, MEAN_SHAPES)):
        x = special_image(h, w, seed=k)
        images.append(x)
        rows.append((FACTORS, order, 123.0))
        pre = restate_pre(x, FACTORS, order)
        want.append(None if pre is None else restate_mean64(pre))
    assert len(PRE_ORDERS) == 16 and len(images) == 54
    dev_images = [x.to(DEV) for x in images]
    coef = ops.color_mean(dev_images, _coef(rows))
    return images, dev_images, rows, want, coef


def test_mean_is_within_one_ulp_of_the_fp64_mean_and_untouched_without_a_contrast(mean_case):
    images, _, rows, want, coef = mean_case
    worst = 0
    for (fac, order, mean), w, (gf, go, gm) in zip(rows, want, _rows(coef)):
        assert go == order and gf == tuple(float(np.float32(v)) for v in fac)
        if w is None:
            assert gm == 123.0                                                    # no contrast: the field is left as it was
        else:
            worst = max(worst, _ulp_apart(gm, np.float32(w)))
    print("worst distance from fp32(fp64 mean), ulp:", worst)
    assert worst <= 1


def test_mean_is_reproducible_and_the_staged_form_gives_the_same_bits(mean_case):
    from pytorch_retinanet_amd import ops
    _, dev_images, rows, _, coef = mean_case
    again = ops.color_mean(dev_images, _coef(rows))
    assert torch.equal(_bits(again), _bits(coef))
    staged = ops.image_stage(dev_images, ops.new_image_arena(len(dev_images), 2048, torch.device(DEV)))
    assert torch.equal(_bits(ops.color_mean(staged, _coef(rows))), _bits(coef))
    # a size no slot can hold (device data): nothing is read, the mean is 0
    staged.in_hw[1] = torch.tensor([64, 64], dtype=torch.int32)
    staged.in_hw[4] = torch.tensor([0, 5], dtype=torch.int32)
    got = _rows(ops.color_mean(staged, _coef(rows)))
    assert got[1][2] == 0.0 and got[4][2] == 0.0 and got[2] == _rows(coef)[2]


def test_mean_past_the_launch_table_and_workspace_checks():
    from pytorch_retinanet_amd import _lib, ops
    images = [special_image(3, 4, seed=k).to(DEV) for k in range(65)]
    rows = [(FACTORS, order_of([0, 1]), 0.0)] * 65
    got = _rows(ops.color_mean(images, _coef(rows)))
    for b in (0, 63, 64):
        want = np.float32(restate_mean64(restate_pre(images[b].cpu(), FACTORS, order_of([0, 1]))))
        assert _ulp_apart(got[b][2], want) <= 1, b
    need = int(_lib.lib.rn_color_mean_workspace_bytes(65))
    short = torch.empty(need - 1, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.RetinanetHipError, match="rn_color_mean"):
        ops.color_mean(images, _coef(rows), workspace=short)


def test_a_jitter_without_contrast_never_launches_the_mean():
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.augment import ColorJitter
    images = [torch.rand(3, 6, 6, device=DEV) for _ in range(2)]
    called = []
    real = ops.color_mean
    ops.color_mean = lambda *a, **k: called.append(1) or real(*a, **k)
    try:
        ColorJitter(brightness=0.3, saturation=0.3, hue=0.1).next_coef(images)
        assert not called
        ColorJitter(contrast=0.3).next_coef(images)
        assert called
    finally:
        ops.color_mean = real


# ---- 3. the application -----------------------------------------------------------------------------------------------
APP_SHAPES = [(16, 24), (16, 24), (9, 13), (16, 24), (20, 11)]                  # out: (16, 24) for all: identity and real resizes
APP_OUT = [(16, 24)] * 5
ORDERS6 = [(0, 1, 2, 3), (3, 2, 1, 0), (1, 3, 0, 2), (2, 0, 3, 1), (3, 0, 1, 2), (1, 2, 3, 0)]


def _app_rows(shapes, orders, factors=FACTORS, seed=0):
    images, rows, jittered = [], [], []
    for k, ((h, w), order) in enumerate(zip(shapes, orders)):
        x = special_image(h, w, seed=seed + k)
        pre = restate_pre(x, factors, order)
        mean = 0.0 if pre is None else float(np.float32(restate_mean64(pre)))
        images.append(x)
        rows.append((factors, order, mean))
        jittered.append(restate(x, factors, order, mean))
    return images, rows, jittered


def _check(images, rows, jittered, out_sizes, hp, wp, dtype=torch.float32, channels_last=False, flags=None):
    from pytorch_retinanet_amd import ops
    dev = [x.to(DEV) for x in images]
    got = ops.transform_batch(dev, out_sizes, MEAN, STD, hp, wp, dtype, channels_last, flags=flags, coef=_coef(rows))
    want = ops.transform_batch([x.to(DEV) for x in jittered], out_sizes, MEAN, STD, hp, wp, dtype, channels_last, flags=flags)
    assert torch.equal(_bits(got), _bits(want))
    return dev, got


@pytest.mark.parametrize("orders", [[(0,)] * 5, [(1,)] * 5, [(2,)] * 5, [(3,)] * 5, ORDERS6[:5], ORDERS6[1:]],
                         ids=["brightness", "contrast", "saturation", "hue", "all-a", "all-b"])
@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
def test_application_equals_the_plain_transform_of_the_restated_images(orders, flip):
    flags = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8, device=DEV) if flip else None
    images, rows, jittered = _app_rows(APP_SHAPES, [order_of(o) for o in orders])
    assert any(not torch.equal(a, b) for a, b in zip(images, jittered))
    _check(images, rows, jittered, APP_OUT, 32, 32, flags=flags)


@pytest.mark.parametrize("dtype, channels_last", [(torch.float32, False), (torch.bfloat16, True), (torch.float16, False)],
                         ids=["f32-nchw", "bf16-nhwc", "f16-nchw"])
def test_application_in_every_output_form_and_with_device_sizes(dtype, channels_last):
    from pytorch_retinanet_amd import ops
    flags = torch.tensor([0, 1, 1, 0, 1], dtype=torch.uint8, device=DEV)
    images, rows, jittered = _app_rows(APP_SHAPES, [order_of(o) for o in ORDERS6[:5]], seed=20)
    dev, got = _check(images, rows, jittered, APP_OUT, 32, 32, dtype, channels_last, flags)
    assert got.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    out_hw = torch.tensor(APP_OUT, dtype=torch.int32, device=DEV)
    coef = _coef(rows)
    by_dev = ops.transform_batch_dev(dev, out_hw, MEAN, STD, 32, 32, dtype, channels_last, flags=flags, coef=coef)
    staged = ops.image_stage(dev, ops.new_image_arena(5, 1024, torch.device(DEV)))
    by_var = ops.transform_batch_var(staged, out_hw, MEAN, STD, 32, 32, dtype, channels_last, flags=flags, coef=coef)
    assert torch.equal(_bits(by_dev), _bits(got)) and torch.equal(_bits(by_var), _bits(got))


def test_an_order_of_all_skips_equals_the_plain_transform():
    from pytorch_retinanet_amd import ops
    images, rows, jittered = _app_rows(APP_SHAPES, [0xFFFF] * 5)
    assert all(torch.equal(a, b) for a, b in zip(images, jittered))
    dev, got = _check(images, rows, jittered, APP_OUT, 32, 32)
    assert torch.equal(_bits(got), _bits(ops.transform_batch(dev, APP_OUT, MEAN, STD, 32, 32)))


@pytest.mark.parametrize("hue", [-0.5, 0.5, -1e-7])
def test_hue_extremes_on_special_pixels(hue):
    images, rows, jittered = _app_rows(APP_SHAPES[:3], [order_of([3]), order_of([3, 2]), order_of([0, 3])], factors=(2.5, 1.0, 0.0, hue))
    _check(images, rows, jittered, APP_OUT[:3], 32, 32)


def test_the_second_launch_reads_its_own_coefficients():
    "B = 65: image 64 is the second launch's first; its coefficients are row 64's."
    shapes = [(4, 4)] * 65
    orders = [order_of(ORDERS6[k % 6]) for k in range(65)]
    images, rows, jittered = _app_rows(shapes, orders)
    rows = [((f[0] + 0.01 * k, f[1], f[2], f[3]), o, m) for k, (f, o, m) in enumerate(rows)]
    jittered = [restate(x, f, o, m) for x, (f, o, m) in zip(images, rows)]
    _check(images, rows, jittered, [(4, 4)] * 65, 4, 4)


# ---- 4. the transform module ------------------------------------------------------------------------------------------
SHAPES = [(24, 40), (33, 21), (40, 40), (17, 30)]
SIZES = (24, 32)


def _module():
    from pytorch_retinanet_amd.augment import ColorJitter, RandomHorizontalFlip, RandomShortSide
    from pytorch_retinanet_amd.transform import GeneralizedRCNNTransform
    t = GeneralizedRCNNTransform(SIZES, 48, MEAN, STD, size_divisible=32).train()
    t.hflip = RandomHorizontalFlip(0.5, seed=3)
    t.scale_jitter = RandomShortSide(SIZES, seed=4)
    return t, ColorJitter(p=0.8, seed=SEED, **RANGES)


def _check_module_call(got, coef, draws, images):
    rows = _rows(coef)
    assert [(f, o) for f, o, _ in rows] == draws                                # factors and orders: the Python draw, bit for bit
    jittered = []
    for x, (fac, order, mean) in zip(images, rows):
        pre = restate_pre(x, fac, order)
        if pre is not None:
            assert _ulp_apart(mean, np.float32(restate_mean64(pre))) <= 1
        jittered.append(restate(x, fac, order, mean))                          # the restatement fed the device's means
    return jittered


@pytest.mark.parametrize("staged", [False, True], ids=["list", "staged"])
def test_whole_path_equals_the_restatement_with_every_augmentation_installed(staged):
    from pytorch_retinanet_amd import ops
    images = [special_image(h, w, seed=30 + k) for k, (h, w) in enumerate(SHAPES)]
    boxes = [torch.tensor([[2.0, 3.0, 15.0, 16.0]]) for _ in SHAPES]
    labels = [torch.tensor([1]) for _ in SHAPES]
    t, cj = _module()
    plain, _ = _module()
    t.color_jitter = cj
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
        draws = cj.draw(k, 4)
        seen |= {o for _, o in draws}
        jittered = _check_module_call(got, cj.coef, draws, images)
        im, tg, kw = inputs(jittered)
        want, _ = plain(im, tg, **kw)
        assert torch.equal(_bits(got.tensors), _bits(want.tensors)), k
        assert cj.counter == k + 1
    assert len(seen) >= 3


def test_eval_mode_and_missing_targets_leave_the_counter_and_the_image_alone():
    images = [special_image(h, w, seed=40 + k).to(DEV) for k, (h, w) in enumerate(SHAPES)]
    t, cj = _module()
    plain, _ = _module()
    t.color_jitter = cj
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
    assert cj.counter == 0 and cj.coef is None and cj._block is None


# ---- 5. the captured step ---------------------------------------------------------------------------------------------
def test_captured_step_draws_anew_at_every_replay_and_equals_its_eager_twin():
    "The bars of tests/test_image_capacity_gpu.py's step tests: losses rtol 2e-2, parameters atol 2e-3."
    from pytorch_retinanet_amd.augment import ColorJitter, RandomHorizontalFlip
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from test_graph_gpu import _setup
    from test_hflip_gpu import _const_batches
    data = _const_batches(5)
    res = {}
    for enabled in (False, True):
        net, opt = _setup()
        cj = net.transform.color_jitter = ColorJitter(p=0.9, seed=SEED, **RANGES)
        net.transform.hflip = RandomHorizontalFlip(p=0.5, seed=21)
        step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=2, enabled=enabled)
        losses, drawn = [], []
        for k, (images, targets) in enumerate(data):
            losses.append(float(step(images, targets)["loss"]))
            drawn.append([(f, o) for f, o, _ in _rows(cj.coef)])
            assert drawn[-1] == cj.draw(k, len(images)), (enabled, k)
        torch.cuda.synchronize()
        assert cj.counter == 5 and len({str(d) for d in drawn}) == 5
        res[enabled] = (np.array(losses), {n: (p.master if hasattr(p, "master") else p.data).detach().float().cpu()
                                           for n, p in net.named_parameters()}, step)
    step = res[True][2]
    assert step.captures == 1 and step.replays == 3, (step.captures, step.replays)
    assert res[False][2].captures == 0 and np.all(np.isfinite(res[True][0]))
    np.testing.assert_allclose(res[True][0], res[False][0], rtol=2e-2)
    for k, a in res[False][1].items():
        torch.testing.assert_close(res[True][1][k], a, rtol=0, atol=2e-3, msg=k)


def test_rewritten_ranges_replay_the_same_graph_and_another_object_is_another_key():
    from pytorch_retinanet_amd.augment import ColorJitter
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from test_graph_gpu import _setup
    from test_hflip_gpu import _const_batches
    net, opt = _setup()
    cj = net.transform.color_jitter = ColorJitter(brightness=0.4, contrast=0.4, seed=SEED)
    step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=1)
    data = _const_batches(5, seed=8)
    for images, targets in data[:2]:
        step(images, targets)
    cj.brightness = (0.5, 0.5)
    for images, targets in data[2:4]:
        out = step(images, targets)
        rows = _rows(cj.coef)
        assert all(f[0] == 0.5 for f, _, _ in rows) and np.isfinite(float(out["loss"]))
    assert step.captures == 1 and step.replays == 3 and cj.counter == 4
    key = step._signature(*data[4])
    assert ("color_jitter", cj) in key
    net.transform.color_jitter = ColorJitter(brightness=0.4, contrast=0.4, seed=SEED)
    assert step._signature(*data[4]) != key
    net.transform.color_jitter = None
    assert not any(isinstance(k, tuple) and k and k[0] == "color_jitter" for k in step._signature(*data[4]))
