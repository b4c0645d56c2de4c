"""GPU: the GT capacity mode -- ragged GT staged into fixed-size buffers (``rn_gt_stage``), the transform's box resize on packed GT
(``rn_gt_scale_packed``), the dense-head loss on packed GT against the exact-shape path, a captured loss replayed with other GT
counts, and ``graph.CapturedTrainStep(gt_capacity=...)`` replaying one graph for batches whose box counts differ.

Bars: the packed path runs the same K2 / K3 kernels on the same rows as the exact-shape path, with upper bounds for the host-side
hints -- losses and gradients bit for bit when the K3 form is the same; whole train steps against an eager twin at the tolerances
of ``tests/test_graph_gpu.py`` (bf16 conv stack, MIOpen's atomically accumulated weight gradients)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RN_EINVAL, RN_EALIGN = -1, -2


def _gt(rng, counts, H=128, W=160, K=5):
    boxes, labels = [], []
    for c in counts:
        b, l = synth.gt_boxes(rng, c, H, W, num_classes=K, wh_lo=12.0, wh_hi=0.6 * min(H, W))
        boxes.append(torch.from_numpy(b.astype(np.float32)).reshape(-1, 4).to(DEV))
        labels.append(torch.from_numpy(l.astype(np.int64)).reshape(-1).to(DEV))
    return boxes, labels


def _poisoned(B, cap):
    "Packed buffers whose every row starts as NaN boxes / label 10^6 (rows past the batch's GT keep that)."
    from pytorch_retinanet_amd import ops
    p = ops.PackedGT.empty(B, cap, torch.device(DEV))
    p.gt_boxes.fill_(float("nan")); p.gt_labels.fill_(10 ** 6); p.gt_off.fill_(-7); p.num_fg.fill_(123)
    return p


# ---- 1. rn_gt_stage ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", [[5], [0], [3, 0, 9], [0, 0, 0], [(i * 5) % 8 for i in range(64)], [(i * 3) % 7 for i in range(65)]],
                         ids=["B1", "B1-zero", "B3", "B3-total0", "B64", "B65"])
def test_stage_equals_cat(counts):
    from pytorch_retinanet_amd import ops
    rng = np.random.default_rng(len(counts))
    boxes, labels = _gt(rng, counts)
    cap = max(max(counts), 1)
    p = _poisoned(len(counts), cap + 2)
    sentinel_b, sentinel_l = p.gt_boxes.clone(), p.gt_labels.clone()
    ops.gt_stage(boxes, labels, p)
    torch.cuda.synchronize()
    n = sum(counts)
    assert torch.equal(p.gt_boxes[:n], torch.cat(boxes)) and torch.equal(p.gt_labels[:n], torch.cat(labels))
    assert p.gt_off.tolist() == [int(v) for v in np.concatenate([[0], np.cumsum(counts)])]
    assert int(p.num_fg.abs().sum()) == 0
    assert torch.equal(p.gt_boxes[n:].isnan(), sentinel_b[n:].isnan()) and torch.equal(p.gt_labels[n:], sentinel_l[n:])


def test_stage_rejects_overflow_negative_counts_and_misalignment():
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd._lib import lib
    rng = np.random.default_rng(9)
    boxes, labels = _gt(rng, [3, 4])
    p = _poisoned(2, 4)
    st = torch.cuda.current_stream().cuda_stream

    def call(bp, lp, counts, rows=p.rows):
        return lib.rn_gt_stage((C.c_void_p * 2)(*bp), (C.c_void_p * 2)(*lp), (C.c_int64 * 2)(*counts), 2, p.gt_boxes.data_ptr(),
                               p.gt_labels.data_ptr(), rows, p.gt_off.data_ptr(), p.num_fg.data_ptr(), C.c_void_p(st))
    bp, lp = [b.data_ptr() for b in boxes], [l.data_ptr() for l in labels]
    assert call(bp, lp, [3, 4], rows=6) == RN_EINVAL                      # sum T > R
    assert call(bp, lp, [3, -1]) == RN_EINVAL
    assert call([bp[0] + 4, bp[1]], lp, [3, 4]) == RN_EALIGN             # boxes need 16 bytes
    assert call(bp, [lp[0], lp[1] + 4], [3, 4]) == RN_EALIGN             # labels 8
    assert call([bp[0], 0], lp, [3, 4]) == RN_EINVAL
    torch.cuda.synchronize()
    assert bool(p.gt_boxes.isnan().all()) and int((p.gt_labels != 10 ** 6).sum()) == 0 and p.gt_off.tolist() == [-7] * 3   # nothing ran
    with pytest.raises(ValueError):
        ops.gt_stage(*_gt(rng, [5, 1]), p)                               # more boxes than the capacity per image
    # misaligned / strided / other-dtype tensors are converted by the wrapper
    buf = torch.zeros(13, device=DEV)
    buf[1:].copy_(boxes[0].reshape(-1))
    mis = buf[1:].view(3, 4)                                               # 4 bytes past a 16-byte boundary
    strided = boxes[1].t().contiguous().t()
    assert mis.data_ptr() % 16 and not strided.is_contiguous()
    ops.gt_stage([mis, strided], [labels[0].int(), labels[1]], p)
    torch.cuda.synchronize()
    assert torch.equal(p.gt_boxes[3:7], boxes[1]) and torch.equal(p.gt_labels[:3], labels[0])


# ---- 2. rn_gt_scale_packed ---------------------------------------------------------------------------------------------
def test_scale_packed_equals_resize_boxes_bit_for_bit():
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.transform import _ratios, resize_boxes
    rng = np.random.default_rng(4)
    counts = [(i * 11) % 13 for i in range(67)]
    boxes, labels = _gt(rng, counts, H=800, W=1333)
    boxes = [b * float(rng.uniform(0.3, 1.7)) for b in boxes]
    p = _poisoned(len(counts), 13)
    ops.gt_stage(boxes, labels, p)
    sizes = [(int(rng.integers(200, 1400)), int(rng.integers(200, 1400))) for _ in counts]
    news = [(int(h * 0.61), int(w * 0.97)) if i % 3 else (h, w) for i, (h, w) in enumerate(sizes)]
    q = ops.gt_scale_packed(p, [_ratios(o, n) for o, n in zip(sizes, news)])
    torch.cuda.synchronize()
    assert q.gt_boxes.data_ptr() != p.gt_boxes.data_ptr() and q.gt_off is p.gt_off and q.gt_labels is p.gt_labels
    off = 0
    for b, o, n in zip(boxes, sizes, news):
        want = resize_boxes(b, o, n)
        assert torch.equal(q.gt_boxes[off:off + b.shape[0]], want)
        off += b.shape[0]
    assert torch.equal(p.gt_boxes[:off], torch.cat(boxes))                # the staged buffer is left as it was


# ---- 3. the dense-head loss on packed GT -------------------------------------------------------------------------------
def _head(B, H=224, W=160, K=5, seed=0):
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.anchors import AnchorGenerator
    levels = synth.levels_for(H, W)
    anc = ops.anchors_emit(levels, list(AnchorGenerator().to(DEV).cell_anchors), 0.0)
    g = torch.Generator(device=DEV).manual_seed(seed)
    cls = [(torch.randn((B, h * w * 9, K), device=DEV, generator=g) - 4.6).to(torch.bfloat16) for h, w, _ in levels]
    box = [(torch.randn((B, h * w * 9, 4), device=DEV, generator=g) * 0.1).to(torch.bfloat16) for h, w, _ in levels]
    return anc, cls, box


def _loss(crit, targets, anc, cls, box):
    cl = [c.detach().clone().requires_grad_() for c in cls]
    bl = [b.detach().clone().requires_grad_() for b in box]
    out = crit.forward_levels(targets, cl, bl, [anc] * cls[0].shape[0])
    (out["classification_loss"] + out["regression_loss"]).backward()
    return torch.stack([out["classification_loss"].detach(), out["regression_loss"].detach()]), [t.grad for t in cl + bl]


BATCHES = [([0, 1, 7, 8], 8), ([8, 31, 1, 0], 32), ([33, 0, 7, 1], 128), ([0, 1, 7, 8, 31, 33, 200, 500], 512)]


@pytest.mark.parametrize("counts, cap", BATCHES, ids=[f"cap{c}" for _, c in BATCHES])
def test_packed_loss_equals_the_exact_shape_loss(counts, cap):
    from pytorch_retinanet_amd import losses, ops
    crit = losses.RetinaNetLosses(5)
    rng = np.random.default_rng(cap)
    boxes, labels = _gt(rng, counts, H=224, W=160)
    anc, cls, box = _head(len(counts), seed=cap)
    exact = [{"boxes": b, "labels": l} for b, l in zip(boxes, labels)]
    p = _poisoned(len(counts), cap)
    old_form, old_fuse = losses.K3_FORM, losses.FUSE_MATCH
    try:
        variants = [(f, False) for f in (0, 1, 2)] + ([(0, True), (2, True)] if cap <= 64 else []) + [("auto", False)]
        for form, fuse in variants:
            losses.K3_FORM, losses.FUSE_MATCH = form, fuse
            le, ge = _loss(crit, exact, anc, cls, box)
            ops.gt_stage(boxes, labels, p)                           # (one loss call per staging: K2 adds into the zeroed num_fg)
            lp, gp = _loss(crit, p, anc, cls, box)
            for a, b in zip(ge, gp):
                assert torch.equal(a, b), (form, fuse)
            if form == "auto":
                np.testing.assert_allclose(lp.cpu().numpy(), le.cpu().numpy(), rtol=1e-6, atol=1e-9)
            else:
                assert torch.equal(lp, le), (form, fuse, lp.tolist(), le.tolist())
            assert bool(torch.isfinite(lp).all())
    finally:
        losses.K3_FORM, losses.FUSE_MATCH = old_form, old_fuse


# ---- 4. one captured loss, replayed with other GT ----------------------------------------------------------------------
def test_captured_packed_loss_replays_with_other_counts():
    from pytorch_retinanet_amd import graph, losses, ops
    crit = losses.RetinaNetLosses(5)
    B, cap = 3, 32
    anc, cls, box = _head(B, seed=5)
    cl = [c.detach().clone().requires_grad_() for c in cls]
    bl = [b.detach().clone().requires_grad_() for b in box]
    rng = np.random.default_rng(12)
    sets = [[4, 0, 32], [1, 1, 1], [0, 0, 0], [32, 17, 9], [2, 30, 5], [9, 9, 0]]
    gts = [_gt(rng, c, H=224, W=160) for c in sets]
    p = _poisoned(B, cap)
    old = losses.K3_FORM
    losses.K3_FORM = 2
    try:
        def run(targets):
            out = crit.forward_levels(targets, cl, bl, [anc] * B)
            total = out["classification_loss"] + out["regression_loss"]
            return [torch.stack([out["classification_loss"], out["regression_loss"]]).detach()] + list(torch.autograd.grad(total, cl + bl))
        state = ops.new_match_state(torch.device(DEV))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), ops.use_match_state(state):      # (warm-up off the capture)
            ops.gt_stage(*gts[0], p)
            run(p)
        torch.cuda.current_stream().wait_stream(side)
        ops.gt_stage(*gts[0], p)
        torch.cuda.synchronize()
        g = graph._new_graph()
        with ops.use_match_state(state), torch.cuda.graph(g, capture_error_mode="thread_local"):
            static = run(p)
        graph._repair_memset_nodes(g)
        for boxes, labels in gts[1:]:
            ops.gt_stage(boxes, labels, p)
            g.replay()
            want = run([{"boxes": b, "labels": l} for b, l in zip(boxes, labels)])
            torch.cuda.synchronize()
            for a, b in zip(want, static):
                assert torch.equal(a, b)
    finally:
        losses.K3_FORM = old


# ---- 5. whole train steps ---------------------------------------------------------------------------------------------
def _var_batches(count_sets, seed=5, H=128, W=160):
    rng = np.random.default_rng(seed)
    out = []
    for counts in count_sets:
        images = [torch.from_numpy(rng.random((3, H, W), dtype=np.float32)).to(DEV) for _ in counts]
        boxes, labels = _gt(rng, counts, H, W)
        out.append((images, [{"boxes": b, "labels": l} for b, l in zip(boxes, labels)]))
    return out


def _params(net):
    return {n: (p.master if hasattr(p, "master") else p.data).detach().float().cpu() for n, p in net.named_parameters()}


def _compare_to_eager(data, make, **kw):
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    res = {}
    for cap in (None, "auto"):
        net, opt = make()
        step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=2, enabled=cap is not None, gt_capacity=cap, **kw)
        losses = [float(step(im, tg)["loss"]) for im, tg in data]
        torch.cuda.synchronize()
        res[cap] = (np.array(losses), _params(net), step)
    assert np.all(np.isfinite(res["auto"][0]))
    np.testing.assert_allclose(res["auto"][0], res[None][0], rtol=2e-2)
    for k, a in res[None][1].items():
        torch.testing.assert_close(res["auto"][1][k], a, rtol=0, atol=2e-3, msg=k)
    return res["auto"][2]


def test_one_graph_serves_a_capacity_class():
    from test_graph_gpu import _setup
    counts = [[3, 9], [32, 1], [0, 17], [12, 12], [31, 2], [5, 20], [9, 0], [25, 30]]      # all in class 32
    step = _compare_to_eager(_var_batches(counts), _setup)
    assert step.captures == 1 and step.replays == 6


def test_class_changes_recapture_and_oversized_batches_keep_exact_keys():
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from test_graph_gpu import _setup
    net, opt = _setup()
    step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=1, gt_capacity="auto")
    counts = [[1, 8], [8, 2], [0, 5], [9, 3], [20, 1], [2, 32]]          # class 8 three times, then class 32 three times
    losses = [float(step(im, tg)["loss"]) for im, tg in _var_batches(counts, seed=8)]
    assert step.captures == 2 and step.replays == 4 and np.all(np.isfinite(losses))
    big = _var_batches([[513, 3], [514, 3]], seed=9)
    losses = [float(step(im, tg)["loss"]) for im, tg in big]             # above the last class: exact keys, one eager call each
    assert np.all(np.isfinite(losses)) and step.captures == 2 and step.replays == 4
    keys = list(step._entries)
    assert keys[-1][1] != ("gt_cap", 512) and keys[-1] != keys[-2]


def test_fp16_scaler_and_segmented_steps_replay_with_changing_counts():
    from pytorch_retinanet_amd.graph import CapturedTrainStep, retinanet_stage_of
    from pytorch_retinanet_amd.parallel import BucketedGradAllReduce
    import pytorch_retinanet_amd as P
    from pytorch_retinanet_amd.optim import MasterSGD, use_16bit_conv_weights
    from test_graph_gpu import _setup
    data = _var_batches([[3, 9], [1, 16], [12, 0], [10, 11], [2, 29]], seed=3)          # all in class 32
    torch.manual_seed(11)
    net = P.Retinanet(num_classes=5, backbone_kind="resnet18", pretrained=False, min_size=128, max_size=160).to(DEV)
    net = net.to(memory_format=torch.channels_last).train()
    use_16bit_conv_weights(net, torch.float16)
    opt = MasterSGD(net.parameters(), lr=1e-2, momentum=0.9, weight_decay=1e-3)
    step = CapturedTrainStep(net, opt, amp_dtype=torch.float16, eager_steps=2, scaler=torch.amp.GradScaler("cuda"), gt_capacity="auto")
    l16 = [float(step(im, tg)["loss"]) for im, tg in data]
    assert step.captures == 1 and step.replays == 3 and np.all(np.isfinite(l16))
    net, opt = _setup()
    ddp = BucketedGradAllReduce(net, stage_of=retinanet_stage_of)        # world 1, no process group
    step = CapturedTrainStep(net, opt, ddp=ddp, amp_dtype=torch.bfloat16, eager_steps=2, gt_capacity="auto")
    assert step.segmented
    ls = [float(step(im, tg)["loss"]) for im, tg in data]
    assert step.captures == 1 and step.replays == 3 and np.all(np.isfinite(ls))


def test_resized_images_rescale_packed_boxes_in_the_step():
    import pytorch_retinanet_amd as P
    from pytorch_retinanet_amd.optim import MasterSGD, use_bf16_conv_weights

    def make():
        torch.manual_seed(11)
        net = P.Retinanet(num_classes=5, backbone_kind="resnet18", pretrained=False, min_size=96, max_size=120).to(DEV)
        net = net.to(memory_format=torch.channels_last).train()
        use_bf16_conv_weights(net)
        return net, MasterSGD(net.parameters(), lr=1e-2, momentum=0.9, weight_decay=1e-3)
    step = _compare_to_eager(_var_batches([[3, 9], [1, 16], [12, 0], [10, 11], [2, 29]], seed=6), make)     # 128 x 160 -> 96 x 120
    assert step.captures == 1 and step.replays == 3


def test_simple_trainer_replays_batches_with_varying_box_counts():
    import pytorch_retinanet_amd as P

    class Varying(torch.utils.data.Dataset):
        def __init__(self, ds):
            self.ds = ds

        def __len__(self):
            return len(self.ds)

        def __getitem__(self, i):
            img, t, idx = self.ds[i]
            n = (i * 5) % 8 + 1
            return img, {**t, "boxes": t["boxes"][:n], "labels": t["labels"][:n]}, idx
    torch.manual_seed(7)
    conf = P.load_hparams()
    conf.model.update(backbone_kind="resnet18", pretrained=False, num_classes=5, min_size=128, max_size=160)
    conf.dataset.kind = "synthetic"
    conf.dataset.update(length=12, height=128, width=160, boxes_per_image=8)
    conf.dataloader.train_bs = 2
    conf.dataloader.valid_bs = 2
    conf.dataloader.args.pin_memory = False
    model = P.RetinaNetModel(conf)
    model.prepare_data()
    model.trn_ds, model.val_ds = Varying(model.trn_ds), None
    trainer = P.SimpleTrainer(max_epochs=1, device=DEV, gt_capacity="auto")
    steps = trainer.fit(model)
    assert steps == 6 and trainer.captured_steps > 0, (steps, trainer.captured_steps)
    assert bool(torch.isfinite(model.net.retinanet_head.classification_head.class_subnet_output.bias.float()).all())


# ---- 6. out-of-bounds guard -------------------------------------------------------------------------------------------
def test_stage_and_scale_stay_inside_their_operands():
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "guard_probe.py"), "gt"], capture_output=True, text=True, env=env,
                       timeout=300, cwd=ROOT)
    tail = (r.stdout + r.stderr)[-1500:]
    assert r.returncode == 0, f"probe gt died (GPU memory access fault?):\n{tail}"
    assert "ok gt" in r.stdout, tail
