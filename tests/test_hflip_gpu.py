"""GPU: the train-time horizontal flip -- the device draw (``rn_hflip_draw``) against its Python restatement, the flipped transform
(``rn_transform_batch_flip``) and box kernels (``rn_gt_flip_scale_many`` / ``_packed``) bit for bit against the unflipped kernels
on torch-flipped inputs, the model's losses and gradients, ``CapturedTrainStep`` replaying the draw, and ``SimpleTrainer`` on a csv
dataset with the shipped hparams."""
import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def _restated(seed, counter, B, p):
    from pytorch_retinanet_amd.augment import RandomHorizontalFlip
    return [int(v) for v in RandomHorizontalFlip.draw_flags(seed, counter, B, p)]


# ---- 1. the draw ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 64, 65, 130])
def test_draw_equals_the_restatement_and_advances_the_counter(B):
    from pytorch_retinanet_amd import draw_state, ops
    seed = 0x1234_5678_9ABC_DEF0 + B
    block = draw_state.new(draw_state.HFLIP, torch.device(DEV), seed=seed, counter=0, p=0.5)
    for k in range(6):
        flags = ops.hflip_draw(block, B)
        assert flags.tolist() == _restated(seed, k, B, 0.5), k
        assert draw_state.read(draw_state.HFLIP, block) == (seed, k + 1, 0.5)
    draw_state.write(draw_state.HFLIP, block, p=0.0)
    assert int(ops.hflip_draw(block, B).sum()) == 0
    draw_state.write(draw_state.HFLIP, block, p=1.0)
    assert int(ops.hflip_draw(block, B).sum()) == B
    assert draw_state.read(draw_state.HFLIP, block) == (seed, 8, 1.0)


def test_flip_object_state_dict_reads_the_device_counter():
    from pytorch_retinanet_amd.augment import RandomHorizontalFlip
    f = RandomHorizontalFlip(0.5, seed=77)
    for k in range(3):
        assert f.next_flags(9, torch.device(DEV)).tolist() == _restated(77, k, 9, 0.5)
    assert f.state_dict() == {"seed": 77, "counter": 3, "p": 0.5}
    f.p = 0.25                                                      # p only: the counter stays
    assert f.next_flags(9, DEV).tolist() == _restated(77, 3, 9, 0.25)
    g = RandomHorizontalFlip()
    g.next_flags(2, DEV)
    g.load_state_dict(f.state_dict())
    assert g.next_flags(9, DEV).tolist() == _restated(77, 4, 9, 0.25) and g.counter == 5


# ---- 2. the transform -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("resize", [True, False], ids=["resized", "identity"])
def test_flipped_transform_equals_the_transform_of_flipped_images(dtype, channels_last, resize):
    from pytorch_retinanet_amd import ops
    g = torch.Generator().manual_seed(3)
    shapes = [(3, 37, 53), (3, 48, 40), (3, 30, 61), (3, 44, 44)]
    images = [torch.rand(s, generator=g).to(DEV) for s in shapes]
    sizes = [(int(s[1] * 1.3), int(s[2] * 1.3)) if resize else (s[1], s[2]) for s in shapes]
    Hp = (max(s[0] for s in sizes) + 31) // 32 * 32
    Wp = (max(s[1] for s in sizes) + 31) // 32 * 32
    flags = torch.tensor([1, 0, 1, 0], dtype=torch.uint8, device=DEV)
    got = ops.transform_batch(images, sizes, MEAN, STD, Hp, Wp, dtype, channels_last, flags=flags)
    plain = ops.transform_batch(images, sizes, MEAN, STD, Hp, Wp, dtype, channels_last)
    flipped = ops.transform_batch([im.flip(-1).contiguous() for im in images], sizes, MEAN, STD, Hp, Wp, dtype, channels_last)
    torch.cuda.synchronize()
    for b, f in enumerate(flags.tolist()):
        want = flipped[b] if f else plain[b]
        assert torch.equal(got[b].float(), want.float()), b
        assert torch.equal(got[b].view(torch.int16 if dtype != torch.float32 else torch.int32),
                           want.view(torch.int16 if dtype != torch.float32 else torch.int32)), b
    assert got.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)


def test_flipped_transform_across_the_64_image_launch_boundary():
    from pytorch_retinanet_amd import ops
    g = torch.Generator().manual_seed(4)
    images = [torch.rand(3, 8 + b % 3, 12 + b % 5, generator=g).to(DEV) for b in range(70)]
    sizes = [(im.shape[1], im.shape[2]) for im in images]
    flags = torch.tensor(_restated(5, 0, 70, 0.5), dtype=torch.uint8, device=DEV)
    got = ops.transform_batch(images, sizes, MEAN, STD, 32, 32, torch.float32, True, flags=flags)
    want = ops.transform_batch([im.flip(-1).contiguous() if f else im for im, f in zip(images, flags.tolist())], sizes, MEAN, STD,
                               32, 32, torch.float32, True)
    assert torch.equal(got, want)


# ---- 3. the boxes -----------------------------------------------------------------------------------------------------
def _boxes(rng, counts, W=160, H=128):
    return [torch.from_numpy(synth.gt_boxes(rng, c, H, W, num_classes=5, wh_lo=4.0, wh_hi=60.0)[0].astype(np.float32)).reshape(-1, 4).to(DEV)
            for c in counts]


def _torch_flip_resize(boxes, widths, ratios, flags):
    from pytorch_retinanet_amd.transform import hflip_boxes, resize_boxes
    out = []
    for b, w, (rh, rw), f in zip(boxes, widths, ratios, flags):
        b = hflip_boxes(b, w) if f else b
        out.append(resize_boxes(b, (1.0, 1.0), (rh, rw)) if (rh, rw) != (1.0, 1.0) else b)
    return out


@pytest.mark.parametrize("counts", [[3, 0, 5, 1], [0], [(i * 3) % 5 for i in range(70)]], ids=["B4", "B1-empty", "B70"])
def test_box_flip_scale_entry_points_equal_torch(counts):
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.transform import _ratios
    rng = np.random.default_rng(len(counts))
    B = len(counts)
    boxes = _boxes(rng, counts)
    widths = [float(160 - (b % 3) * 7) for b in range(B)]
    news = [(128, 160), (96, 120), (128, 160), (77, 101)]
    ratios = [_ratios((128, widths[b]), news[b % 4]) if b % 4 != 2 else (1.0, 1.0) for b in range(B)]
    flags_l = [(b * 7 + 1) % 3 != 0 for b in range(B)]
    flags = torch.tensor(flags_l, dtype=torch.uint8, device=DEV)
    want = _torch_flip_resize(boxes, widths, ratios, flags_l)
    got = ops.gt_flip_scale_many(boxes, widths, ratios, flags)
    assert got.shape == (sum(counts), 4)
    assert torch.equal(got, torch.cat(want)) if sum(counts) else got.numel() == 0
    cap = max(max(counts), 1)
    packed = ops.PackedGT.empty(B, cap + 1, torch.device(DEV))
    ops.gt_stage(boxes, [torch.ones(c, dtype=torch.int64, device=DEV) for c in counts], packed)
    out = ops.gt_flip_scale_packed(packed, widths, ratios, flags)
    n = sum(counts)
    assert torch.equal(out.gt_boxes[:n], torch.cat(want)) and out.gt_off is packed.gt_off
    ones = [(1.0, 1.0)] * B                                         # ratio 1 everywhere: the flip still runs
    out1 = ops.gt_flip_scale_packed(packed, widths, ones, flags)
    assert torch.equal(out1.gt_boxes[:n], torch.cat(_torch_flip_resize(boxes, widths, ones, flags_l)))


# ---- 4. the model (fused path) ----------------------------------------------------------------------------------------
def _flipped_inputs(images, targets):
    fi = [im.flip(-1).contiguous() for im in images]
    ft = []
    for im, t in zip(images, targets):
        b = t["boxes"].clone()
        b[:, [0, 2]] = im.shape[-1] - b[:, [2, 0]]
        ft.append({"boxes": b, "labels": t["labels"]})
    return fi, ft


def _losses_and_grads(net, images, targets, amp):
    net.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        losses = net(list(images), [dict(t) for t in targets])
    (losses["classification_loss"] + losses["regression_loss"]).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().float().cpu().clone() for n, p in net.named_parameters() if p.grad is not None}
    return {k: v.detach().float().cpu() for k, v in losses.items()}, grads


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "bf16"])
def test_model_with_p1_equals_the_model_fed_flipped_inputs(amp):
    """Losses and every parameter gradient bit for bit.  MIOpen's default weight-gradient algorithms accumulate atomically and do
    not repeat themselves bit for bit from call to call, so the comparison runs with ``cudnn.deterministic``."""
    import pytorch_retinanet_amd as P
    from pytorch_retinanet_amd.augment import RandomHorizontalFlip
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        torch.manual_seed(5)
        net = P.Retinanet(num_classes=5, backbone_kind="resnet18", pretrained=False, min_size=128, max_size=160).to(DEV)
        net = net.to(memory_format=torch.channels_last).train()
        if amp:
            from pytorch_retinanet_amd.optim import use_bf16_conv_weights
            use_bf16_conv_weights(net)
        rng = np.random.default_rng(2)
        images = [torch.from_numpy(rng.random((3, 120, 150), dtype=np.float32)).to(DEV) for _ in range(2)]     # resized to 128 x 160
        targets = [{"boxes": b, "labels": torch.randint(1, 6, (b.shape[0],), device=DEV)} for b in _boxes(rng, [4, 6], W=150, H=120)]
        fi, ft = _flipped_inputs(images, targets)
        ref_l, ref_g = _losses_and_grads(net, fi, ft, amp)
        net.transform.hflip = RandomHorizontalFlip(p=1.0, seed=3)
        got_l, got_g = _losses_and_grads(net, images, targets, amp)
        assert net.transform.hflip.counter == 1 and net.transform.hflip.flags.tolist() == [1, 1]
    finally:
        torch.backends.cudnn.deterministic = old
    assert float(got_l["regression_loss"]) > 0
    for k in ref_l:
        assert torch.equal(got_l[k], ref_l[k]), (k, got_l[k], ref_l[k])
    assert set(got_g) == set(ref_g) and len(ref_g) > 0
    for k in ref_g:
        assert torch.equal(got_g[k], ref_g[k]), k


# ---- 5. the captured step ---------------------------------------------------------------------------------------------
def _const_batches(n, seed=5, H=128, W=160, T=(3, 5)):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        images = [torch.from_numpy(rng.random((3, H, W), dtype=np.float32)).to(DEV) for _ in T]
        targets = [{"boxes": b, "labels": torch.from_numpy(rng.integers(1, 6, b.shape[0])).to(DEV)} for b in _boxes(rng, list(T), W, H)]
        out.append((images, targets))
    return out


@pytest.mark.parametrize("gt_capacity", [None, "auto"], ids=["exact", "capacity"])
def test_captured_step_draws_at_every_replay_and_matches_an_eager_twin(gt_capacity):
    from pytorch_retinanet_amd.augment import RandomHorizontalFlip
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from test_graph_gpu import _setup
    data = _const_batches(6)
    seed = 21
    res = {}
    for enabled in (False, True):
        net, opt = _setup()
        net.transform.hflip = RandomHorizontalFlip(p=0.5, seed=seed)
        step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=2, enabled=enabled, gt_capacity=gt_capacity)
        losses, flags = [], []
        for images, targets in data:
            losses.append(float(step(images, targets)["loss"]))
            flags.append(net.transform.hflip.flags.tolist())
        torch.cuda.synchronize()
        assert flags == [_restated(seed, k, 2, 0.5) for k in range(6)], flags
        assert net.transform.hflip.counter == 6
        res[enabled] = (np.array(losses), {n: (p.master if hasattr(p, "master") else p.data).detach().float().cpu()
                                           for n, p in net.named_parameters()}, step)
    flat = [f for k in range(6) for f in _restated(seed, k, 2, 0.5)]
    assert 0 < sum(flat) < len(flat), "the seed should give a mix of flipped and unflipped images"
    step = res[True][2]
    assert step.captures == 1 and step.replays >= 3, (step.captures, step.replays)
    assert np.all(np.isfinite(res[True][0]))
    np.testing.assert_allclose(res[True][0], res[False][0], rtol=2e-2)
    for k, a in res[False][1].items():
        torch.testing.assert_close(res[True][1][k], a, rtol=0, atol=2e-3, msg=k)


def test_segmented_step_draws_inside_its_first_segment():
    from pytorch_retinanet_amd.augment import RandomHorizontalFlip
    from pytorch_retinanet_amd.graph import CapturedTrainStep, retinanet_stage_of
    from pytorch_retinanet_amd.parallel import BucketedGradAllReduce
    from test_graph_gpu import _setup
    net, opt = _setup()
    net.transform.hflip = RandomHorizontalFlip(p=0.5, seed=21)
    ddp = BucketedGradAllReduce(net, stage_of=retinanet_stage_of)        # world 1, no process group
    step = CapturedTrainStep(net, opt, ddp=ddp, amp_dtype=torch.bfloat16, eager_steps=2, gt_capacity="auto")
    assert step.segmented
    losses = []
    for k, (images, targets) in enumerate(_const_batches(5, seed=9)):
        losses.append(float(step(images, targets)["loss"]))
        assert net.transform.hflip.flags.tolist() == _restated(21, k, 2, 0.5), k
    assert step.captures == 1 and step.replays == 3 and np.all(np.isfinite(losses))
    assert net.transform.hflip.counter == 5


def test_changing_p_replays_the_same_graph():
    from pytorch_retinanet_amd.augment import RandomHorizontalFlip
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from test_graph_gpu import _setup
    net, opt = _setup()
    net.transform.hflip = RandomHorizontalFlip(p=0.0, seed=2)
    step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=1)
    data = _const_batches(4, seed=8)
    for images, targets in data[:2]:
        step(images, targets)
    assert net.transform.hflip.flags.tolist() == [0, 0]
    net.transform.hflip.p = 1.0
    for images, targets in data[2:]:
        step(images, targets)
        assert net.transform.hflip.flags.tolist() == [1, 1]
    assert step.captures == 1 and step.replays == 3


# ---- 6. the trainer ---------------------------------------------------------------------------------------------------
def test_simple_trainer_on_a_csv_dataset_replays_with_the_flip(tmp_path):
    from PIL import Image
    import pytorch_retinanet_amd as P
    H, W = 128, 160
    rng = np.random.default_rng(0)
    rows = ["filename,width,height,class,xmin,ymin,xmax,ymax,labels"]
    for i in range(12):
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(tmp_path / f"im{i}.png")
        rows += [f"im{i}.png,{W},{H},a,{4 + i},10,{70 + i},80,1", f"im{i}.png,{W},{H},b,60,{20 + i},150,{100 + i},3"]
    (tmp_path / "train.csv").write_text("\n".join(rows) + "\n")
    torch.manual_seed(7)
    conf = P.load_hparams()                                         # the shipped transforms: albumentations.HorizontalFlip, p = 0.5
    conf.model.update(backbone_kind="resnet18", pretrained=False, num_classes=5, min_size=128, max_size=160)
    conf.dataset.kind = "csv"
    conf.dataset.trn_paths = str(tmp_path / "train.csv")
    conf.dataloader.train_bs = 2
    conf.dataloader.args.pin_memory = False
    model = P.RetinaNetModel(conf)
    model.prepare_data()
    hf = model.net.transform.hflip
    assert hf is not None and hf.p == 0.5
    trainer = P.SimpleTrainer(max_epochs=1, device=DEV)
    steps = trainer.fit(model)
    assert steps == 6 and trainer.captured_steps > 0, (steps, trainer.captured_steps)
    assert hf.counter == 6 and hf.flags is not None and hf.flags.is_cuda
    assert bool(torch.isfinite(model.net.retinanet_head.classification_head.class_subnet_output.bias.float()).all())
