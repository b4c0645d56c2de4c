"""GPU: multi-scale training drawn on the device -- the draw (``rn_short_side_draw``) against its Python restatement, the transform
reading its sizes from the device (``rn_transform_batch_dev``) and the box kernels reading their ratios there
(``rn_gt_flip_scale_many_dev`` / ``_packed_dev``) bit for bit against the host-size kernels, the transform module against its own
PyTorch path, and ``CapturedTrainStep`` replaying ONE graph while the sizes vary."""
import numpy as np
import pytest
import torch

import synth
from test_scale_jitter import MAX_SIZE, MEAN, SEED, SHAPES, SIZES, STD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HP = WP = 64                    # SHAPES at the largest of SIZES under MAX_SIZE, rounded up to 32


def _images(seed=3, shapes=SHAPES):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand((3, h, w), generator=g).to(DEV) for h, w in shapes]


def _restated(seed, counter, shapes=SHAPES, sizes=SIZES, max_size=MAX_SIZE):
    from pytorch_retinanet_amd.augment import RandomShortSide
    j = RandomShortSide(sizes, seed=seed)
    hw = j.draw(counter, shapes, max_size)
    return hw, j.ratios(shapes, hw)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---- 1. the draw ------------------------------------------------------------------------------------------------------
def test_draw_equals_the_restatement_bit_for_bit_and_advances_the_counter():
    from pytorch_retinanet_amd import draw_state, ops
    block = draw_state.new(draw_state.SHORT_SIDE, torch.device(DEV), seed=SEED, counter=0, sizes=SIZES)
    assert draw_state.read(draw_state.SHORT_SIDE, block) == (SEED, 0, SIZES)
    seen = set()
    for k in range(6):
        out_hw, ratios = ops.short_side_draw(block, SHAPES, MAX_SIZE)
        hw, rr = _restated(SEED, k)
        assert out_hw.dtype == torch.int32 and [tuple(r) for r in out_hw.tolist()] == hw, k
        want = torch.tensor([v for r in rr for v in r], dtype=torch.float32)
        assert torch.equal(_bits(ratios.cpu()), _bits(want)), k
        assert draw_state.read(draw_state.SHORT_SIDE, block)[1] == k + 1                  # the counter = the number of calls
        seen.add(tuple(hw))
    assert len(seen) >= 4
    draw_state.write(draw_state.SHORT_SIDE, block, sizes=(32,), counter=0)                # one candidate: every image gets it, the seed is kept
    out_hw, _ = ops.short_side_draw(block, SHAPES, MAX_SIZE)
    assert [tuple(r) for r in out_hw.tolist()] == _restated(SEED, 0, sizes=(32,))[0]
    assert draw_state.read(draw_state.SHORT_SIDE, block) == (SEED, 1, (32,))


def test_draw_across_the_64_image_launch_table():
    "B = 66: two launches share one counter value; the images past the table boundary get their own sizes, the counter moves once."
    from pytorch_retinanet_amd import draw_state, ops
    shapes = [(8, 8)] * 66
    block = draw_state.new(draw_state.SHORT_SIDE, torch.device(DEV), seed=7, counter=0, sizes=(4, 8))
    for k in range(3):
        out_hw, ratios = ops.short_side_draw(block, shapes, 8)
        hw, rr = _restated(7, k, shapes, (4, 8), 8)
        assert [tuple(r) for r in out_hw.tolist()] == hw, k
        assert ratios.tolist() == [v for r in rr for v in r]
        assert {hw[64], hw[65]} <= {(4, 4), (8, 8)} and len(set(hw)) == 2
        assert draw_state.read(draw_state.SHORT_SIDE, block)[1] == k + 1
    assert len({_restated(7, k, shapes, (4, 8), 8)[0][64] for k in range(3)} |
               {_restated(7, k, shapes, (4, 8), 8)[0][65] for k in range(3)}) == 2      # both sizes occur past the boundary


def test_object_state_lives_on_the_device():
    from pytorch_retinanet_amd.augment import RandomShortSide
    j = RandomShortSide(SIZES, seed=SEED)
    for k in range(3):
        hw, _ = j.next_sizes(SHAPES, MAX_SIZE, torch.device(DEV))
        assert hw.is_cuda and [tuple(r) for r in hw.tolist()] == _restated(SEED, k)[0]
    assert j.state_dict() == {"seed": SEED, "counter": 3, "sizes": list(SIZES)}
    j.sizes = (24, 32)                                                       # written into the block: no new object, the counter stays
    hw, _ = j.next_sizes(SHAPES, MAX_SIZE, DEV)
    assert [tuple(r) for r in hw.tolist()] == _restated(SEED, 3, sizes=(24, 32))[0] and j.counter == 4
    with pytest.raises(ValueError, match="canvas"):
        j.sizes = (24, 56)
    with pytest.raises(RuntimeError, match="lives on the GPU"):
        j.next_sizes(SHAPES, MAX_SIZE, "cpu")
    k = RandomShortSide((48,))
    k.next_sizes(SHAPES, MAX_SIZE, DEV)
    k.load_state_dict(j.state_dict())
    hw, _ = k.next_sizes(SHAPES, MAX_SIZE, DEV)
    assert [tuple(r) for r in hw.tolist()] == _restated(SEED, 4, sizes=(24, 32))[0] and k.counter == 5


# ---- 2. the transform -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
def test_transform_with_device_sizes_equals_the_transform_with_host_sizes(dtype, channels_last, flip):
    from pytorch_retinanet_amd import draw_state, ops
    images = _images()
    flags = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8, device=DEV) if flip else None
    block = draw_state.new(draw_state.SHORT_SIDE, torch.device(DEV), seed=SEED, counter=0, sizes=SIZES)
    identity = 0
    for k in range(2):
        out_hw, _ = ops.short_side_draw(block, SHAPES, MAX_SIZE)
        sizes = _restated(SEED, k)[0]
        identity += sum(s == hw for s, hw in zip(sizes, SHAPES))
        got = ops.transform_batch_dev(images, out_hw, MEAN, STD, HP, WP, dtype, channels_last, flags=flags)
        want = ops.transform_batch(images, sizes, MEAN, STD, HP, WP, dtype, channels_last, flags=flags)
        assert got.shape == want.shape == (5, 3, HP, WP)
        assert got.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
        assert torch.equal(got, want) and torch.equal(_bits(got), _bits(want)), k
        for b, (nh, nw) in enumerate(sizes):                                 # padding outside each drawn size: exactly zero
            assert not got[b, :, nh:, :].any() and not got[b, :, :, nw:].any(), (k, b)
            assert bool(got[b, :, :nh, :nw].float().abs().sum() > 0)
    assert identity >= 2, "the seed should draw the identity size (the one-tap branch) for some image"


def test_transform_clamps_a_device_size_above_the_canvas():
    """Sizes are device data: one above the canvas is clamped to it, one <= 0 leaves padding.  (The kernel's stores are addressed by the
    grid alone, which the host sizes from Hp x Wp: no value in ``out_hw`` moves a store.)"""
    from pytorch_retinanet_amd import ops
    images = _images(shapes=[(16, 16)] * 3)
    out_hw = torch.tensor([[40, 1000], [0, -5], [32, 32]], dtype=torch.int32, device=DEV)
    got = ops.transform_batch_dev(images, out_hw, MEAN, STD, 32, 32)
    want = ops.transform_batch(images, [(32, 32)] * 3, MEAN, STD, 32, 32)
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]) and not got[1].any()


# ---- 3. the boxes -----------------------------------------------------------------------------------------------------
def _boxes(rng, counts, W=64, H=48):
    return [torch.from_numpy(synth.gt_boxes(rng, c, H, W, num_classes=5, wh_lo=4.0, wh_hi=30.0)[0].astype(np.float32)).reshape(-1, 4).to(DEV)
            for c in counts]


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
@pytest.mark.parametrize("counts", [[3, 0, 5, 1, 2], [0, 0, 0, 0, 0]], ids=["B5", "no-boxes"])
def test_box_kernels_with_device_ratios_equal_their_host_ratio_forms_and_torch(counts, flip):
    from pytorch_retinanet_amd import draw_state, ops
    from pytorch_retinanet_amd.transform import hflip_boxes, resize_boxes
    rng = np.random.default_rng(1 + sum(counts))
    B = len(SHAPES)
    boxes = _boxes(rng, counts)
    widths = [float(w) for _, w in SHAPES]
    flags_l = [True, False, True, True, False] if flip else [False] * B
    flags = torch.tensor(flags_l, dtype=torch.uint8, device=DEV)
    block = draw_state.new(draw_state.SHORT_SIDE, torch.device(DEV), seed=SEED, counter=1, sizes=SIZES)          # counter 1: two images keep their size (ratio 1)
    _, ratios_dev = ops.short_side_draw(block, SHAPES, MAX_SIZE)
    sizes, ratios = _restated(SEED, 1)
    assert (1.0, 1.0) in ratios
    # torch on the CPU: the flip formula, then transform.resize_boxes
    want = []
    for b, (h, w), new, f in zip(boxes, SHAPES, sizes, flags_l):
        b = b.cpu()
        want.append(resize_boxes(hflip_boxes(b, float(w)) if f else b, (h, w), new).reshape(-1, 4))
    want = torch.cat(want)
    n = sum(counts)
    got = ops.gt_flip_scale_many_dev(boxes, widths, ratios_dev, flags if flip else None)
    host = ops.gt_flip_scale_many(boxes, widths, ratios, flags)
    assert got.shape == (n, 4) and torch.equal(_bits(got), _bits(host)) and torch.equal(got.cpu(), want)
    packed = ops.PackedGT.empty(B, max(max(counts), 1) + 1, torch.device(DEV))
    ops.gt_stage(boxes, [torch.ones(c, dtype=torch.int64, device=DEV) for c in counts], packed)
    out = ops.gt_flip_scale_packed_dev(packed, widths, ratios_dev, flags if flip else None)
    host = ops.gt_flip_scale_packed(packed, widths, ratios, flags)
    assert out.gt_off is packed.gt_off and out.gt_boxes is not packed.gt_boxes
    assert torch.equal(_bits(out.gt_boxes[:n]), _bits(host.gt_boxes[:n])) and torch.equal(out.gt_boxes[:n].cpu(), want)


# ---- 4. the transform module ------------------------------------------------------------------------------------------
def _targets(rng, counts=(3, 0, 5, 1, 2)):
    out = []
    for (h, w), c in zip(SHAPES, counts):
        b = synth.gt_boxes(rng, c, h, w, num_classes=5, wh_lo=3.0, wh_hi=20.0)[0].astype(np.float32).reshape(-1, 4)
        out.append({"boxes": torch.from_numpy(b), "labels": torch.arange(1, c + 1)})
    return out


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "with-flip"])
def test_fused_module_with_a_jitter_equals_its_pytorch_path(flip):
    "The bars of tests/test_model_gpu.py::test_transform_module_fused_equals_torch_path for the pixels; the boxes exactly."
    from pytorch_retinanet_amd.augment import RandomHorizontalFlip, RandomShortSide
    from pytorch_retinanet_amd.transform import GeneralizedRCNNTransform
    images = [im.cpu() for im in _images(5)]
    targets = _targets(np.random.default_rng(6))
    pair = []
    for _ in range(2):
        t = GeneralizedRCNNTransform(SIZES, MAX_SIZE, MEAN, STD, size_divisible=32).train()
        t.scale_jitter = RandomShortSide(SIZES, seed=SEED)
        if flip:
            t.hflip = RandomHorizontalFlip(0.5, seed=3)
        pair.append(t)
    cpu, gpu = pair
    for k in range(3):
        ref, rt = cpu(images, [dict(x) for x in targets])
        got, gt = gpu([i.to(DEV) for i in images], [{n: v.to(DEV) for n, v in x.items()} for x in targets])
        sizes = _restated(SEED, k)[0]
        assert gpu.scale_jitter.sizes_drawn.is_cuda and [tuple(r) for r in gpu.scale_jitter.sizes_drawn.tolist()] == sizes
        assert [tuple(r) for r in cpu.scale_jitter.sizes_drawn.tolist()] == sizes
        assert got.image_sizes == ref.image_sizes and tuple(got.tensors.shape) == tuple(ref.tensors.shape) == (5, 3, HP, WP)
        torch.testing.assert_close(got.tensors.cpu(), ref.tensors, rtol=0, atol=2e-5)
        for a, b in zip(gt, rt):
            assert torch.equal(a["boxes"].cpu(), b["boxes"]) and torch.equal(a["labels"].cpu(), b["labels"])
        for b, (nh, nw) in enumerate(sizes):
            assert not got.tensors[b, :, nh:, :].any() and not got.tensors[b, :, :, nw:].any()
    cl, _ = gpu([i.to(DEV) for i in images], [{n: v.to(DEV) for n, v in x.items()} for x in targets], out_dtype=torch.bfloat16,
                channels_last=True)
    ref, _ = cpu(images, [dict(x) for x in targets])
    assert cl.tensors.dtype == torch.bfloat16 and cl.tensors.is_contiguous(memory_format=torch.channels_last)
    torch.testing.assert_close(cl.tensors.float().cpu(), ref.tensors, rtol=1e-2, atol=1e-2)
    assert gpu.scale_jitter.counter == cpu.scale_jitter.counter == 4


def test_eval_mode_runs_no_draw_on_the_fused_path():
    from pytorch_retinanet_amd.augment import RandomShortSide
    from pytorch_retinanet_amd.transform import GeneralizedRCNNTransform
    images = _images(5)
    t = GeneralizedRCNNTransform(48, MAX_SIZE, MEAN, STD).eval()
    plain, _ = t(images, None)
    t.scale_jitter = RandomShortSide(SIZES, seed=SEED)
    got, _ = t(images, None)
    assert torch.equal(got.tensors, plain.tensors) and got.image_sizes == plain.image_sizes
    assert t.scale_jitter.counter == 0 and t.scale_jitter.sizes_drawn is None


# ---- 5. the captured step ---------------------------------------------------------------------------------------------
STEP_SIZES, STEP_SEED, STEP_SHAPES = (96, 112, 128), 2, [(128, 160)] * 2        # the model of test_graph_gpu._setup: max_size = 160


@pytest.mark.parametrize("flip, gt_capacity", [(False, None), (True, "auto")], ids=["jitter", "jitter-flip-capacity"])
def test_captured_step_replays_one_graph_while_the_sizes_vary(flip, gt_capacity):
    from pytorch_retinanet_amd.augment import RandomHorizontalFlip, RandomShortSide
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from test_graph_gpu import _setup
    from test_hflip_gpu import _const_batches
    data = _const_batches(6)
    want = [_restated(STEP_SEED, k, STEP_SHAPES, STEP_SIZES, 160)[0] for k in range(6)]
    assert len({tuple(w) for w in want[2:]}) == 4, "the seed should give the four replays four different size rows"
    assert any(s == (128, 160) for w in want[2:] for s in w) and len({s for w in want for s in w}) == 3
    res = {}
    for enabled in (False, True):
        net, opt = _setup()
        net.transform.scale_jitter = RandomShortSide(STEP_SIZES, seed=STEP_SEED)
        if flip:
            net.transform.hflip = RandomHorizontalFlip(p=0.5, seed=21)
        step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=2, enabled=enabled, gt_capacity=gt_capacity)
        losses = []
        for k, (images, targets) in enumerate(data):
            losses.append(float(step(images, targets)["loss"]))
            assert [tuple(r) for r in net.transform.scale_jitter.sizes_drawn.tolist()] == want[k], (enabled, k)
        torch.cuda.synchronize()
        assert net.transform.scale_jitter.counter == 6
        if flip:
            assert net.transform.hflip.counter == 6
        res[enabled] = (np.array(losses), {n: (p.master if hasattr(p, "master") else p.data).detach().float().cpu()
                                           for n, p in net.named_parameters()}, step)
    step = res[True][2]
    assert step.captures == 1 and step.replays == len(data) - step.eager_steps == 4, (step.captures, step.replays)
    assert res[False][2].captures == 0 and res[False][2].replays == 0
    assert np.all(np.isfinite(res[True][0]))
    np.testing.assert_allclose(res[True][0], res[False][0], rtol=2e-2)          # (the equality test_hflip_gpu's captured test asserts)
    for k, a in res[False][1].items():
        torch.testing.assert_close(res[True][1][k], a, rtol=0, atol=2e-3, msg=k)


def test_new_candidates_replay_the_same_graph():
    from pytorch_retinanet_amd.augment import RandomShortSide
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from test_graph_gpu import _setup
    from test_hflip_gpu import _const_batches
    net, opt = _setup()
    sj = net.transform.scale_jitter = RandomShortSide((96, 128), seed=STEP_SEED)
    step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=1)
    data = _const_batches(4, seed=8)
    for images, targets in data[:2]:
        step(images, targets)
    sj.sizes = (112,)
    for images, targets in data[2:]:
        out = step(images, targets)
        assert [tuple(r) for r in sj.sizes_drawn.tolist()] == [(112, 140)] * 2 and np.isfinite(float(out["loss"]))
    assert step.captures == 1 and step.replays == 3 and sj.counter == 4
