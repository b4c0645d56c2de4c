"""GPU: ``rn_box_iou_loss`` (GIoU / DIoU on the matched rows, behind K3) against the float64 evaluation of its restatement
(``losses.box_iou_loss_reference``) on the same, already rounded inputs.

Bars: fp32 ``rtol=1e-5, atol=1e-7`` for ``out_loss[1]`` and every box gradient; bf16 / fp16 one output rounding
(``rtol=2**-8`` / ``2**-10``, ``atol=1e-7``) for the gradients, as ``test_hip_parity.py``.  fp32 holds that bar only while the
coordinates stay small (at 1333-pixel coordinates an fp32 evaluation of the same formula does not), so anchors and boxes live on a
64-pixel canvas, and every case first asserts ON THE CPU that the restatement run in fp32 meets HALF the fp32 bar against float64 on
its inputs, that no min / max of the rule ties and that no slot is clipped (but in the clip case).

Shapes: four levels of 8 x 8, 4 x 4, 2 x 2 and 1 x 1 locations with 9 anchors each: A = 765, no multiple of 64 (the last flag word is
partial).  B = 3: an image without GT, one with a single box, one with enough boxes that more than 64 of its rows are flagged.  One
case with B = 2 and A = 1 048 805: the launch is at most 128 workgroups of 4 waves, a wave per strip of 64 flag words of one image,
so one grid pass covers 512 strips; that case has 2 x 257 = 514."""
import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 5
LEVELS = ((8, 8.0), (4, 16.0), (2, 32.0), (1, 64.0))            # (locations per side, stride = base anchor size): a 64-pixel canvas
SIZES = [g * g * 9 for g, _ in LEVELS]
A = sum(SIZES)
RTOL = {torch.float32: 1e-5, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}
ATOL = 1e-7
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT_IDS = ["fp32", "bf16", "fp16"]
GRID_STRIPS = 128 * 4                                            # strips of 64 flag words one pass of the launch covers


def _anchor_set():
    "[765, 4] fp32: per location 3 scales x 3 aspect ratios around the stride, levels in order, row-major, cell anchor fastest."
    rows = []
    for g, s in LEVELS:
        shapes = [(s * 2 ** (k / 3) / np.sqrt(r), s * 2 ** (k / 3) * np.sqrt(r)) for k in range(3) for r in (0.5, 1.0, 2.0)]
        for y in range(g):
            for x in range(g):
                cx, cy = (x + 0.5) * s, (y + 0.5) * s
                rows += [[cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2] for w, h in shapes]
    return torch.tensor(np.asarray(rows, np.float32))


def _gts(seed=0):
    rng = np.random.default_rng(seed)
    box = lambda T: torch.from_numpy(synth.gt_boxes(rng, T, 64, 64, num_classes=K, wh_lo=6.0, wh_hi=40.0)[0].astype(np.float32)).reshape(-1, 4)
    # the single box sits on the 16 x 16 anchor of level 1's location (1, 1), (16, 16, 32, 32), so that the max-IoU rule matches it too
    gts = [torch.zeros((0, 4)), torch.tensor([[15.5, 16.5, 31.0, 33.0]]), box(12)]
    labels = [torch.from_numpy(rng.integers(1, K + 1, size=g.shape[0])) for g in gts]
    return gts, labels


def _head(B, dtype, seed=0, reg_w=(1.0, 1.0, 1.0, 1.0)):
    "Per-level (cls, box) outputs on the device, already rounded to ``dtype``."
    g = torch.Generator().manual_seed(seed)
    cls = [(torch.randn((B, s, K), generator=g) - 4.6).to(dtype).to(DEV) for s in SIZES]
    box = [(torch.randn((B, s, 4), generator=g) * 0.2 * torch.tensor(reg_w)).to(dtype).to(DEV) for s in SIZES]
    return cls, box


def _matches(matcher, anc, gts):
    "(matches i64 [B,A] dense, num_fg i32 [B]) of the named matcher, on the CPU."
    from pytorch_retinanet_amd import ops
    boxes = torch.cat(gts).to(DEV)
    off = ops.gt_offsets([g.shape[0] for g in gts], torch.device(DEV))
    if matcher == "atss":
        m, n = ops.atss_match(anc, boxes, off, len(gts), SIZES, 9, 9)
    else:
        m, n = ops.iou_match(anc, boxes, off, len(gts), 0.5, 0.4)
    torch.cuda.synchronize()
    return m.cpu(), n.cpu()


def _decoded(deltas, anc, reg_w):
    "Step 1 in fp32 on the CPU: (t2, t3, px1, py1, px2, py2) of rows [N,4]."
    t = deltas / torch.tensor(reg_w, dtype=torch.float32)
    acx, acy, aw, ah = (anc[:, 0] + anc[:, 2]) / 2, (anc[:, 1] + anc[:, 3]) / 2, anc[:, 2] - anc[:, 0], anc[:, 3] - anc[:, 1]
    cx, cy = aw * t[:, 0] + acx, ah * t[:, 1] + acy
    w, h = aw * torch.exp(t[:, 2].clamp(max=4.135)), ah * torch.exp(t[:, 3].clamp(max=4.135))
    return t[:, 2], t[:, 3], cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2


def _restate(rows, nfg, B, kind, weight, reg_w, dtype):
    """Steps 1-5 on the CPU in ``dtype``: ``rows`` = per image (deltas [n,4], anchors [n,4], GT [n,4]) of its matched rows (fp32
    values).  Returns (loss, [gradient [n,4] per image])."""
    from pytorch_retinanet_amd.losses import box_iou_loss_reference
    total, leaves = torch.zeros((), dtype=dtype), []
    for b, (d, an, g) in enumerate(rows):
        d = d.to(dtype).clone().requires_grad_()
        leaves.append(d)
        if d.shape[0]:
            scale = torch.tensor(1.0, dtype=dtype) / max(int(nfg[b]), 1) / B
            total = total + box_iou_loss_reference(d, an.to(dtype), g.to(dtype), kind, reg_w).sum() * scale
    total = total * weight
    if total.requires_grad:
        total.backward()
    return total.detach(), [torch.zeros_like(d) if d.grad is None else d.grad for d in leaves]


def _reference(rows, nfg, B, kind, weight=1.0, reg_w=(1.0, 1.0, 1.0, 1.0), clipped_ok=False):
    """The float64 reference of a case, after the CPU checks of its inputs: no tie, no clipped slot, and the fp32 evaluation of the
    restatement within HALF the fp32 bar of the float64 one."""
    for d, an, g in rows:
        t2, t3, px1, py1, px2, py2 = _decoded(d.float(), an, reg_w)
        assert not bool(((px1 == g[:, 0]) | (py1 == g[:, 1]) | (px2 == g[:, 2]) | (py2 == g[:, 3])).any()), "a min / max of the rule ties"
        assert clipped_ok or not bool(((t2 >= 4.1) | (t3 >= 4.1)).any()), "a clipped slot"
    l64, g64 = _restate(rows, nfg, B, kind, weight, reg_w, torch.float64)
    l32, g32 = _restate(rows, nfg, B, kind, weight, reg_w, torch.float32)
    half = lambda a, b: bool(((a.double() - b).abs() <= 0.5 * (ATOL + RTOL[torch.float32] * b.abs())).all())
    worst = max([float((a.double() - b).abs().max()) for a, b in zip(g32, g64) if b.numel()] or [0.0])
    print(f"fp32 restatement vs float64: loss {float(l32):.9g} / {float(l64):.9g}, worst gradient difference {worst:.3g}, "
          f"largest gradient {max([float(b.abs().max()) for b in g64 if b.numel()] or [0.0]):.3g}")
    assert half(l32, l64) and all(half(a, b) for a, b in zip(g32, g64)), "the fp32 restatement misses half the bar on these inputs"
    return l64, g64


def _close(got, want, rtol, what):
    err = (got.double() - want).abs()
    bound = ATOL + rtol * want.abs()
    print(f"{what}: worst error {float(err.max()) if err.numel() else 0.0:.3g}, worst error / bound {float((err / bound).max()) if err.numel() else 0.0:.3g}")
    assert bool((err <= bound).all()), what


def _matched_rows(box_levels, anc, gts, m):
    "Per image: (deltas, anchors, GT boxes) of the matched rows on the CPU, and their indices."
    cat = torch.cat([b.float().cpu() for b in box_levels], 1)
    rows, idx = [], []
    for b in range(m.shape[0]):
        i = (m[b] >= 0).nonzero().flatten()
        idx.append(i)
        rows.append((cat[b, i], (anc if anc.dim() == 2 else anc[b])[i], gts[b][m[b, i]] if i.numel() else torch.zeros((0, 4))))
    return rows, idx


def _losses_run(matcher, kind, cls, box, anc, gts, labels, weight=1.0, prescale=None):
    "forward_levels + backward of a RetinaNetLosses -> (f32[2] losses, [grad per cls level], [grad per box level])."
    from pytorch_retinanet_amd import losses
    crit = losses.RetinaNetLosses(K, matcher=matcher, box_loss=kind, box_loss_weight=weight)
    cl = [c.clone().requires_grad_() for c in cls]
    bl = [b.clone().requires_grad_() for b in box]
    targets = [{"boxes": g.to(DEV), "labels": l.to(DEV)} for g, l in zip(gts, labels)]
    out = crit.forward_levels(targets, cl, bl, [anc.to(DEV)] * len(gts))
    (out["classification_loss"] + out["regression_loss"]).backward()
    torch.cuda.synchronize()
    return torch.stack([out["classification_loss"], out["regression_loss"]]).detach().cpu(), [t.grad.cpu() for t in cl], [t.grad.cpu() for t in bl]


_SMOOTH = {}


def _smooth_run(matcher, dtype, cls, box, anc, gts, labels):
    "The smooth-L1 run of (matcher, dtype), once."
    if (matcher, dtype) not in _SMOOTH:
        _SMOOTH[(matcher, dtype)] = _losses_run(matcher, "smooth_l1", cls, box, anc, gts, labels)
    return _SMOOTH[(matcher, dtype)]


# ---- against float64, through RetinaNetLosses, with both matchers ------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", ["giou", "diou"])
@pytest.mark.parametrize("matcher", ["iou", "atss"])
def test_loss_and_gradients_against_float64_and_nothing_else_moves(matcher, kind, dtype):
    anc = _anchor_set()
    assert anc.shape[0] == A == 765 and A % 64 != 0
    gts, labels = _gts()
    cls, box = _head(3, dtype)
    m, nfg = _matches(matcher, anc.to(DEV), gts)
    flagged = (m != -1).sum(1)
    # (K2 flags EVERY row of an image without GT as ignored, ATSS none: either way it has no matched row)
    assert int((m[0] >= 0).sum()) == 0 and int(nfg[1]) > 0 and int(flagged[2]) > 64, (flagged.tolist(), nfg.tolist())
    rows, idx = _matched_rows(box, anc, gts, m)
    want_l, want_g = _reference(rows, nfg, 3, kind)
    loss, gcls, gbox = _losses_run(matcher, kind, cls, box, anc, gts, labels)
    loss0, gcls0, gbox0 = _smooth_run(matcher, dtype, cls, box, anc, gts, labels)
    # what must not move: the class loss, every class gradient, the box gradient of every row that is not matched
    assert torch.equal(loss[0], loss0[0]) and not torch.equal(loss[1], loss0[1])
    for a, b in zip(gcls, gcls0):
        assert torch.equal(a, b)
    got, got0 = torch.cat(gbox, 1), torch.cat(gbox0, 1)
    keep = m < 0
    assert torch.equal(got[keep], got0[keep])
    assert int(keep[0].sum()) == A and not bool(got[0].any())              # the image without GT: all zeros, as K3 left it
    # what must: the loss at the fp32 bar, the matched rows' gradients at the dtype's
    _close(loss[1], want_l, RTOL[torch.float32], "regression loss")
    for b in range(3):
        _close(got[b, idx[b]].float(), want_g[b], RTOL[dtype], f"box gradient, image {b}")
    assert float(want_l) > 0 and max(float(g.abs().max()) for g in want_g if g.numel()) > 1e-3


def test_the_weight_multiplies_loss_and_gradient():
    anc = _anchor_set()
    gts, labels = _gts(seed=4)
    cls, box = _head(3, torch.float32, seed=4)
    m, nfg = _matches("iou", anc.to(DEV), gts)
    rows, idx = _matched_rows(box, anc, gts, m)
    want_l, want_g = _reference(rows, nfg, 3, "giou", weight=2.0)
    loss, _, gbox = _losses_run("iou", "giou", cls, box, anc, gts, labels, weight=2.0)
    _close(loss[1], want_l, RTOL[torch.float32], "regression loss, weight 2")
    got = torch.cat(gbox, 1)
    for b in range(3):
        _close(got[b, idx[b]], want_g[b], RTOL[torch.float32], f"box gradient, image {b}, weight 2")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_a_clipped_slot_has_zero_gradient_and_a_finite_loss(dtype):
    anc = _anchor_set()
    gts, labels = _gts()
    cls, box = _head(3, dtype, seed=2)
    m, nfg = _matches("iou", anc.to(DEV), gts)
    # the first matched rows of levels 0 and 1 (the smaller anchors) of the last image: two get dw above the clip, two dh
    first = [(i, int(a)) for i, a in enumerate((m[2] >= 0).nonzero().flatten().tolist()) if a < SIZES[0] + SIZES[1]][:4]
    assert len(first) == 4
    for n, (_, a) in enumerate(first):
        lvl = 0 if a < SIZES[0] else 1
        box[lvl][2, a - lvl * SIZES[0], 2 if n < 2 else 3] = 6.0 if n % 2 else 60000.0       # (60000: finite in fp16, exp of it is not)
    rows, idx = _matched_rows(box, anc, gts, m)
    want_l, want_g = _reference(rows, nfg, 3, "giou", clipped_ok=True)
    loss, _, gbox = _losses_run("iou", "giou", cls, box, anc, gts, labels)
    got = torch.cat(gbox, 1)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(got).all())
    for n, (i, a) in enumerate(first):
        slot = 2 if n < 2 else 3
        assert float(got[2, a, slot]) == 0.0 and float(want_g[2][i, slot]) == 0.0
    _close(loss[1], want_l, RTOL[torch.float32], "regression loss with clipped slots")
    for b in range(3):
        _close(got[b, idx[b]].float(), want_g[b], RTOL[dtype], f"box gradient with clipped slots, image {b}")


# ---- the op alone ------------------------------------------------------------------------------------------------------------
def _k3_then_op(dtype, kind, anc, gts, labels, cls, box, prescale=None, want_grad=True, weight=1.0):
    "K3 and then the op, as the loss Function calls them, with K2's flagged-only buffers -> (loss f32[2], gbox list or None), on the CPU."
    from pytorch_retinanet_amd import losses, ops
    dev = torch.device(DEV)
    B = len(gts)
    gt_boxes, gt_labels, gt_off, _ = ops.gt_pack([g.to(DEV) for g in gts], [l.to(DEV) for l in labels], dev)
    matches, num_fg, special = ops.iou_match(anc.to(DEV), gt_boxes, gt_off, B, 0.5, 0.4, want_special=True, flagged_only=True)
    params = losses.RetinaNetLosses(K)._params()
    loss, gcls, gbox = ops.loss_fwd_bwd_levels(cls, box, anc.to(DEV), gt_boxes, gt_labels, gt_off, matches, num_fg, params, want_grad,
                                               special=special, in_kernel_finalize=True, grad_prescale=prescale,
                                               form=losses.k3_form(int(gt_boxes.shape[0]), B))
    out = ops.box_iou_loss(box, anc.to(DEV), gt_boxes, gt_off, matches, num_fg, special, loss, gbox, kind, weight=weight,
                           grad_prescale=prescale)
    assert out is loss
    torch.cuda.synchronize()
    return loss.cpu(), None if gbox is None else [g.cpu() for g in gbox]


def test_two_calls_give_the_same_bits_and_value_only_gives_the_same_loss():
    anc = _anchor_set()
    gts, labels = _gts()
    cls, box = _head(3, torch.bfloat16, seed=1)
    first = _k3_then_op(torch.bfloat16, "diou", anc, gts, labels, cls, box)
    second = _k3_then_op(torch.bfloat16, "diou", anc, gts, labels, cls, box)
    assert torch.equal(first[0], second[0]) and all(torch.equal(a, b) for a, b in zip(first[1], second[1]))
    value, none = _k3_then_op(torch.bfloat16, "diou", anc, gts, labels, cls, box, want_grad=False)
    assert none is None and torch.equal(value, first[0])
    # and the op is what RetinaNetLosses runs
    loss, _, gbox = _losses_run("iou", "diou", cls, box, anc, gts, labels)
    assert torch.equal(loss, first[0]) and all(torch.equal(a, b) for a, b in zip(gbox, first[1]))


def test_the_fp16_prescale_goes_in_before_the_one_rounding():
    anc = _anchor_set()
    gts, labels = _gts()
    cls, box = _head(3, torch.float16, seed=3)
    pre = torch.full((1,), 1024.0, device=DEV)
    loss, gbox = _k3_then_op(torch.float16, "giou", anc, gts, labels, cls, box, prescale=pre)
    plain, _ = _k3_then_op(torch.float16, "giou", anc, gts, labels, cls, box)
    assert torch.equal(loss, plain)                                        # the losses are not scaled
    m, nfg = _matches("iou", anc.to(DEV), gts)
    rows, idx = _matched_rows(box, anc, gts, m)
    want_l, want_g = _reference(rows, nfg, 3, "giou")
    _close(loss[1], want_l, RTOL[torch.float32], "regression loss")
    got = torch.cat(gbox, 1)
    for b in range(3):
        _close(got[b, idx[b]].float(), want_g[b] * 1024.0, RTOL[torch.float16], f"box gradient x 1024, image {b}")
    assert max(float(g.abs().max()) for g in want_g if g.numel()) * 1024.0 > 1.0


def test_flag_words_past_one_grid_pass_with_ignored_rows_a_stale_index_and_unflagged_garbage():
    from pytorch_retinanet_amd import ops
    big = 64 * 64 * 256 + 64 * 3 + 37                                      # 16 388 flag words per image -> 257 strips, the last one 4 words
    sizes = [1_000_000, 40_000, big - 1_040_000]
    B, T = 2, 5
    strips = (((big + 63) // 64) + 63) // 64
    assert B * strips == 514 > GRID_STRIPS and big % 64 != 0
    assert ops.lib.rn_box_iou_loss_workspace_bytes(B, big) == 128 * 8
    rng = np.random.default_rng(9)
    reg_w = (10.0, 10.0, 5.0, 5.0)
    base = _anchor_set()
    anc = base[torch.arange(big) % A].contiguous()
    gts = [torch.from_numpy(synth.gt_boxes(rng, T, 64, 64, num_classes=K, wh_lo=6.0, wh_hi=40.0)[0].astype(np.float32)).reshape(-1, 4) for _ in range(B)]
    edge = [0, 1, 63, 64, 4095, 4096, 999_999, 1_000_000, 1_039_999, 1_040_000, big - 37, big - 1]
    flagged = [np.unique(np.concatenate([edge, np.arange(500_000, 500_070), rng.integers(0, big, 150)])),      # > 64 rows in one strip
               np.unique(np.concatenate([[0, 256 * 4096, 256 * 4096 + 24, big - 1], rng.integers(256 * 4096, big, 40), rng.integers(0, big, 100)]))]
    assert all(int((f >= 256 * 4096).sum()) > 0 for f in flagged)          # both images have rows in their last strip (strips 256 and 513)
    m = torch.full((B, big), 3, dtype=torch.int64)                         # unflagged entries hold a VALID index: reading one would show
    dense = torch.full((B, big), -1, dtype=torch.int64)
    bits = np.zeros((B, (big + 63) // 64 * 64), np.uint64)
    for b, f in enumerate(flagged):
        code = rng.integers(0, T, f.shape[0])
        code[rng.random(f.shape[0]) < 0.2] = -2                            # ignored rows: flagged, not matched
        code[0] = 2
        dense[b, f] = torch.from_numpy(code)
        m[b, f] = torch.from_numpy(code)
        bits[b, f] = 1
    stale = int(flagged[1][-1])                                            # a stale word beyond the image's rows is clamped to its last row
    m[1, stale], dense[1, stale] = 99, T - 1
    words = torch.from_numpy((bits.reshape(B, -1, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64).view(np.int64))
    nfg = (dense >= 0).sum(1).to(torch.int32)
    g = torch.Generator().manual_seed(6)
    box = [(torch.randn((B, s, 4), generator=g) * 0.2 * torch.tensor(reg_w)).to(DEV) for s in sizes]
    gbox = [torch.full_like(b, 7.0) for b in box]
    loss = torch.tensor([3.5, 9.0], device=DEV)
    off = ops.gt_offsets([T] * B, torch.device(DEV))
    ops.box_iou_loss(box, anc.to(DEV), torch.cat(gts).to(DEV), off, m.to(DEV), nfg.to(DEV), words.to(DEV), loss, gbox, "giou", reg_w=reg_w)
    torch.cuda.synchronize()
    got = torch.cat(gbox, 1)
    written = (got != 7.0).any(-1).cpu()
    assert torch.equal(written, dense >= 0)                                # exactly the matched rows were written; the rest keep the fill
    assert bool((got[~written.to(DEV)] == 7.0).all())
    cat = torch.cat(box, 1)
    rows, idx = [], []
    for b in range(B):
        i = (dense[b] >= 0).nonzero().flatten()
        idx.append(i)
        rows.append((cat[b, i.to(DEV)].cpu(), anc[i], gts[b][dense[b, i]]))
    want_l, want_g = _reference(rows, nfg, B, "giou", reg_w=reg_w)
    assert float(loss[0]) == 3.5
    _close(loss[1].cpu(), want_l, RTOL[torch.float32], "regression loss")
    for b in range(B):
        _close(got[b, idx[b].to(DEV)].cpu(), want_g[b], RTOL[torch.float32], f"box gradient, image {b}")


# ---- through the model -------------------------------------------------------------------------------------------------------
def test_the_models_regression_loss_is_the_restatement_of_its_own_head_outputs():
    import pytorch_retinanet_amd as P
    from pytorch_retinanet_amd import losses, ops
    torch.manual_seed(5)
    net = P.Retinanet(num_classes=K, backbone_kind="resnet18", pretrained=False, min_size=128, max_size=160, box_loss="giou").to(DEV)
    net = net.to(memory_format=torch.channels_last).train()
    images, tg = synth.e2e_inputs()
    images = [torch.from_numpy(i).to(DEV) for i in images]
    targets = [{"boxes": torch.from_numpy(np.asarray(b, np.float32)).to(DEV), "labels": torch.from_numpy(np.asarray(l, np.int64)).to(DEV)} for b, l in tg]
    seen = {}
    head = net.retinanet_head
    inner = head.compute_loss_levels

    def spy(targets, outputs, anchors, ahead=None):
        seen.update(targets=targets, box=[b.detach().clone() for b in outputs["bbox_levels"]], anchors=losses._stack_anchors(anchors))
        return inner(targets, outputs, anchors, ahead=ahead)
    head.compute_loss_levels = spy
    out = net(images, targets)
    plain = P.Retinanet(num_classes=K, backbone_kind="resnet18", pretrained=False, min_size=128, max_size=160).to(DEV)
    plain = plain.to(memory_format=torch.channels_last).train()
    plain.load_state_dict(net.state_dict())
    out0 = plain(images, targets)
    torch.cuda.synchronize()
    assert torch.equal(out["classification_loss"], out0["classification_loss"])
    assert not torch.equal(out["regression_loss"], out0["regression_loss"])
    gts = [t["boxes"].reshape(-1, 4).float() for t in seen["targets"]]
    anc = seen["anchors"]
    B = len(gts)
    m, nfg = ops.iou_match(anc, torch.cat(gts), ops.gt_offsets([g.shape[0] for g in gts], torch.device(DEV)), B, 0.5, 0.4)
    torch.cuda.synchronize()
    m, nfg, anc = m.cpu(), nfg.cpu(), anc.cpu()
    assert int(nfg.sum()) > 0
    rows, _ = _matched_rows(seen["box"], anc, [g.cpu() for g in gts], m)
    want_l, _ = _restate(rows, nfg, B, "giou", 1.0, (1.0, 1.0, 1.0, 1.0), torch.float64)
    _close(out["regression_loss"].detach().cpu(), want_l, RTOL[torch.float32], "the model's regression loss")
    (out["classification_loss"] + out["regression_loss"]).backward()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p.grad).all()) for p in net.retinanet_head.regression_head.parameters() if p.grad is not None)


class _Tiny(torch.nn.Module):
    "Per-level head outputs straight from parameters (plus the images' means): a net without convolutions, so a step is reproducible."

    def __init__(self, anchors, kind):
        super().__init__()
        from pytorch_retinanet_amd.losses import RetinaNetLosses
        g = torch.Generator().manual_seed(3)
        self.cls = torch.nn.ParameterList([torch.nn.Parameter(torch.randn((1, s, K), generator=g) * 0.5 - 4.6) for s in SIZES])
        self.box = torch.nn.ParameterList([torch.nn.Parameter(torch.randn((1, s, 4), generator=g) * 0.2) for s in SIZES])
        self.retinanet_head = torch.nn.Module()
        self.retinanet_head.losses = RetinaNetLosses(K, box_loss=kind, box_loss_weight=2.0)
        self.register_buffer("anchors", anchors.clone())

    def forward(self, images, targets):
        s = torch.stack(list(images)).mean(dim=(1, 2, 3)).view(-1, 1, 1)
        cls = [p + s for p in self.cls]
        box = [p * (1.0 + s) for p in self.box]
        return self.retinanet_head.losses.forward_levels(targets, cls, box, [self.anchors] * len(images))


def test_a_captured_step_replays_one_graph_over_changing_gt_counts():
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from pytorch_retinanet_amd.optim import MasterSGD
    anc = _anchor_set().to(DEV)
    net, twin = _Tiny(anc, "giou").to(DEV), _Tiny(anc, "giou").to(DEV)
    step = CapturedTrainStep(net, MasterSGD(net.parameters(), lr=1e-2, momentum=0.9), amp_dtype=None, eager_steps=1, gt_capacity="auto")
    rng = np.random.default_rng(13)
    counts = [[3, 8], [1, 0], [8, 8], [0, 5]]                              # all in capacity class 8
    reg = []
    for i, cs in enumerate(counts):
        images = [torch.from_numpy(rng.random((3, 64, 64), dtype=np.float32)).to(DEV) for _ in cs]
        targets = [{"boxes": torch.from_numpy(synth.gt_boxes(rng, c, 64, 64, num_classes=K, wh_lo=6.0, wh_hi=40.0)[0].astype(np.float32)).reshape(-1, 4).to(DEV),
                    "labels": torch.from_numpy(rng.integers(1, K + 1, size=c)).to(DEV)} for c in cs]
        twin.load_state_dict(net.state_dict())                             # the eager step on the same weights
        want = twin(images, targets)
        got = step(images, targets)
        torch.cuda.synchronize()
        for k in ("classification_loss", "regression_loss"):
            _close(got[k].detach().cpu(), want[k].detach().double().cpu(), RTOL[torch.float32], f"step {i} {k}")
        reg.append(float(got["regression_loss"]))
    assert step.captures == 1 and step.replays == len(counts) - 1
    assert all(np.isfinite(reg)) and reg[0] > 0 and reg[2] > 0 and reg[0] != reg[2]
    assert any(isinstance(k, tuple) and k and k[0] == "box_loss" for k in next(iter(step._entries)))
