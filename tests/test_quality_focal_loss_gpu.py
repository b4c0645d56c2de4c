"""GPU: ``rn_quality_focal_loss`` (the soft-target term of Quality Focal Loss on the matched rows' label elements, behind K3 run with
``alpha = 1, gamma = beta``) against the float64 evaluation of its restatement (``losses.box_quality_reference`` +
``losses.quality_focal_loss_reference``) on the same, already rounded inputs.

Bars: fp32 ``rtol=1e-5, atol=1e-7`` for ``out_loss[0]`` (against ``double(K3's value) + the float64 sum``) and the label-element
gradients; bf16 / fp16 one output rounding (``rtol=2**-8`` / ``2**-10``, ``atol=1e-7``) for the gradients.  As in
``test_box_iou_loss_gpu.py`` anchors and boxes live on a 64-pixel canvas, and every case first asserts ON THE CPU that the restatement
run in fp32 meets HALF the fp32 bar against float64 on its inputs (the positives' sum against the bar of the sum alone, which is
stricter than the bar of the whole classification loss) and that no min / max of the IoU ties.

Shapes: that file's A = 765 on four levels (the last flag word is partial), K = 5, and K = 3 in 16-bit cases: rows of an odd K start
at odd element offsets, so the one-element store is not 4-byte aligned.  B = 3: an image without GT, one with a single box, one with
more than 64 flagged rows.  One case with B = 2, K = 1 and A = 64 * 64 * 257: 514 strips, more than the 512 of one grid pass."""
import numpy as np
import pytest
import torch

import synth
from test_box_iou_loss_gpu import A, GRID_STRIPS, SIZES, _anchor_set, _close, _decoded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = {torch.float32: 1e-5, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}
ATOL = 1e-7
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT_IDS = ["fp32", "bf16", "fp16"]
ONES = (1.0, 1.0, 1.0, 1.0)


def _gts(K, seed=0):
    rng = np.random.default_rng(seed)
    box = lambda T: torch.from_numpy(synth.gt_boxes(rng, T, 64, 64, num_classes=K, wh_lo=6.0, wh_hi=40.0)[0].astype(np.float32)).reshape(-1, 4)
    # the single box sits on the 16 x 16 anchor of level 1's location (1, 1), so that the max-IoU rule matches it too
    gts = [torch.zeros((0, 4)), torch.tensor([[15.5, 16.5, 31.0, 33.0]]), box(12)]
    labels = [torch.from_numpy(rng.integers(1, K + 1, size=g.shape[0])) for g in gts]
    return gts, labels


def _head(B, K, dtype, seed=0, sizes=SIZES):
    "Per-level (cls, box) outputs on the device, already rounded to ``dtype``: logits around the prior and around zero."
    g = torch.Generator().manual_seed(seed)
    cls = [(torch.randn((B, s, K), generator=g) * 1.5 - 2.0).to(dtype).to(DEV) for s in sizes]
    box = [(torch.randn((B, s, 4), generator=g) * 0.2).to(dtype).to(DEV) for s in sizes]
    return cls, box


def _dense_matches(matcher, anc, gts):
    "(matches i64 [B,A] dense, num_fg i32 [B]) of the named matcher, on the CPU."
    from pytorch_retinanet_amd import ops
    boxes = torch.cat(gts).to(DEV)
    off = ops.gt_offsets([g.shape[0] for g in gts], torch.device(DEV))
    if matcher == "atss":
        m, n = ops.atss_match(anc.to(DEV), boxes, off, len(gts), SIZES, 9, 9)
    else:
        m, n = ops.iou_match(anc.to(DEV), boxes, off, len(gts), 0.5, 0.4)
    torch.cuda.synchronize()
    return m.cpu(), n.cpu()


def _matched(cls, box, anc, gts, labels, m):
    "Per image the matched rows on the CPU: (rows, label index c, logits [n], deltas [n,4], anchors [n,4], GT [n,4])."
    ccat, bcat = torch.cat([c.float().cpu() for c in cls], 1), torch.cat([b.float().cpu() for b in box], 1)
    out = []
    for b in range(m.shape[0]):
        i = (m[b] >= 0).nonzero().flatten()
        c = labels[b][m[b, i]] - 1 if i.numel() else torch.zeros((0,), dtype=torch.int64)
        g = gts[b][m[b, i]] if i.numel() else torch.zeros((0, 4))
        out.append((i, c, ccat[b, i, c], bcat[b, i], (anc if anc.dim() == 2 else anc[b])[i], g))
    return out


def _restate(rows, nfg, B, beta, reg_w, dtype, shift):
    "Steps 1-4 on the CPU in ``dtype`` -> (the positives' sum, [label-element gradient [n] per image], [quality [n] per image])."
    from pytorch_retinanet_amd.losses import box_quality_reference, quality_focal_loss_reference
    total, grads, quals = torch.zeros((), dtype=dtype), [], []
    for b, (_, _, x, d, an, g) in enumerate(rows):
        x = x.to(dtype).clone().requires_grad_()
        if x.shape[0] == 0:
            grads.append(torch.zeros((0,), dtype=dtype))
            quals.append(torch.zeros((0,), dtype=dtype))
            continue
        q = box_quality_reference(d.to(dtype), an.to(dtype), g.to(dtype), reg_w)
        scale = torch.tensor(1.0, dtype=dtype) / max(int(nfg[b]), 1) / B
        l = quality_focal_loss_reference(x, q, beta, shift).sum() * scale
        l.backward()
        total = total + l.detach()
        grads.append(x.grad)
        quals.append(q)
    return total, grads, quals


def _reference(rows, nfg, B, beta, reg_w=ONES, clipped_ok=False):
    """The float64 reference of a case, after the CPU checks of its inputs: no tie in the IoU, no clipped slot, and the fp32 evaluation
    of the restatement within HALF the fp32 bar of the float64 one."""
    from pytorch_retinanet_amd.config import LOGIT_SHIFT
    for _, _, _, d, an, g in rows:
        t2, t3, px1, py1, px2, py2 = _decoded(d.float(), an, reg_w)
        assert not bool(((px1 == g[:, 0]) | (py1 == g[:, 1]) | (px2 == g[:, 2]) | (py2 == g[:, 3])).any()), "a min / max of the IoU ties"
        assert clipped_ok or not bool(((t2 >= 4.1) | (t3 >= 4.1)).any()), "a clipped slot"
    s64, g64, q64 = _restate(rows, nfg, B, beta, reg_w, torch.float64, LOGIT_SHIFT)
    s32, g32, _ = _restate(rows, nfg, B, beta, reg_w, torch.float32, LOGIT_SHIFT)
    half = lambda a, b: bool(((a.double() - b).abs() <= 0.5 * (ATOL + RTOL[torch.float32] * b.abs())).all())
    worst = max([float(((a.double() - b).abs() / (ATOL + RTOL[torch.float32] * b.abs())).max()) for a, b in zip(g32, g64) if b.numel()] or [0.0])
    print(f"fp32 restatement vs float64: positives' sum {float(s32):.9g} / {float(s64):.9g}, worst gradient error / bar {worst:.3g}, "
          f"largest gradient {max([float(b.abs().max()) for b in g64 if b.numel()] or [0.0]):.3g}, "
          f"qualities {min([float(q.min()) for q in q64 if q.numel()] or [0.0]):.3g} .. {max([float(q.max()) for q in q64 if q.numel()] or [0.0]):.3g}")
    assert half(s32, s64) and all(half(a, b) for a, b in zip(g32, g64)), "the fp32 restatement misses half the bar on these inputs"
    return s64, g64


def _k3_then_qfl(matcher, K, beta, anc, gts, labels, cls, box, prescale=None, want_grad=True, reg_w=ONES, capacity=None):
    """K3 with ``alpha = 1, gamma = beta`` and then the op, as the loss Function calls them, with the matcher's flagged-only buffers.
    Returns CPU copies: K3's (loss, gcls, gbox) as cloned between the two calls, and (loss, gcls, gbox) after the op."""
    from pytorch_retinanet_amd import losses, ops
    from pytorch_retinanet_amd.config import LOGIT_SHIFT
    dev = torch.device(DEV)
    B = len(gts)
    boxes, labs = [g.to(DEV) for g in gts], [l.to(DEV) for l in labels]
    if capacity is not None:
        p = ops.gt_stage(boxes, labs, ops.PackedGT.empty(B, capacity, dev))
        gt_boxes, gt_labels, gt_off = p.gt_boxes, p.gt_labels, p.gt_off
        assert gt_boxes.shape[0] == B * capacity > sum(g.shape[0] for g in gts)          # padded GT rows behind every image's own
    else:
        gt_boxes, gt_labels, gt_off, _ = ops.gt_pack(boxes, labs, dev)
    if matcher == "atss":
        matches, num_fg, special = ops.atss_match(anc.to(DEV), gt_boxes, gt_off, B, SIZES, 9, 9, want_special=True, flagged_only=True)
    else:
        matches, num_fg, special = ops.iou_match(anc.to(DEV), gt_boxes, gt_off, B, 0.5, 0.4, want_special=True, flagged_only=True)
    crit = losses.RetinaNetLosses(K, cls_loss="qfl", qfl_beta=beta)
    params = crit._params()
    assert (params.alpha, params.gamma) == (1.0, beta)
    params.reg_w[:] = reg_w
    loss, gcls, gbox = ops.loss_fwd_bwd_levels(cls, box, anc.to(DEV), gt_boxes, gt_labels, gt_off, matches, num_fg, params, want_grad,
                                               special=special, in_kernel_finalize=True, grad_prescale=prescale,
                                               form=losses.k3_form(int(gt_boxes.shape[0]), B))
    cp = lambda ts: None if ts is None else [t.clone() for t in ts]
    k3 = (loss.clone(), cp(gcls), cp(gbox))
    out = ops.quality_focal_loss(cls, box, anc.to(DEV), gt_boxes, gt_labels, gt_off, matches, num_fg, special, loss, gcls, beta=beta,
                                 reg_w=reg_w, logit_shift=LOGIT_SHIFT, grad_prescale=prescale)
    assert out is loss
    torch.cuda.synchronize()
    cpu = lambda ts: None if ts is None else [t.cpu() for t in ts]
    return (k3[0].cpu(), cpu(k3[1]), cpu(k3[2])), (loss.cpu(), cpu(gcls), cpu(gbox))


def _label_mask(rows, B, K):
    "bool [B, A, K]: the matched rows' label elements."
    mask = torch.zeros((B, A, K), dtype=torch.bool)
    for b, (i, c, *_) in enumerate(rows):
        mask[b, i, c] = True
    return mask


def _check(k3, got, rows, nfg, B, K, want_s, want_g, dtype, scale=1.0):
    "Everything a case asserts about one K3 + op run."
    (loss0, gcls0, gbox0), (loss, gcls, gbox) = k3, got
    mask = _label_mask(rows, B, K)
    before, after = torch.cat(gcls0, 1), torch.cat(gcls, 1)
    # K3's zero: the contract the rule rests on -- with alpha = 1 every matched label element has loss weight and gradient 0 / -0
    assert bool((before[mask] == 0).all()), "K3 left a non-zero gradient at a matched label element"
    # untouched: every other class gradient element, every box gradient, the regression loss
    assert torch.equal(after[~mask], before[~mask])
    assert all(torch.equal(a, b) for a, b in zip(gbox, gbox0)) and torch.equal(loss[1], loss0[1])
    # the loss: K3's value plus the float64 sum, at the fp32 bar
    _close(loss[0], loss0[0].double() + want_s, RTOL[torch.float32], "classification loss")
    assert float(want_s) > 0 and float(loss[0]) > float(loss0[0])
    for b, (i, c, *_) in enumerate(rows):
        _close(after[b, i, c].float(), want_g[b] * scale, RTOL[dtype], f"label-element gradient, image {b}")
    assert max(float(g.abs().max()) for g in want_g if g.numel()) * scale > 1e-4


# ---- against float64, with both matchers, every beta -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("beta", [2.0, 1.5, 0.0])
@pytest.mark.parametrize("matcher", ["iou", "atss"])
def test_loss_and_label_gradients_against_float64_and_nothing_else_moves(matcher, beta, dtype):
    K = 5
    anc = _anchor_set()
    assert anc.shape[0] == A == 765 and A % 64 != 0
    gts, labels = _gts(K)
    cls, box = _head(3, K, dtype)
    m, nfg = _dense_matches(matcher, anc, gts)
    flagged = (m != -1).sum(1)
    assert int((m[0] >= 0).sum()) == 0 and int(nfg[1]) > 0 and int(flagged[2]) > 64, (flagged.tolist(), nfg.tolist())
    rows = _matched(cls, box, anc, gts, labels, m)
    want_s, want_g = _reference(rows, nfg, 3, beta)
    k3, got = _k3_then_qfl(matcher, K, beta, anc, gts, labels, cls, box)
    _check(k3, got, rows, nfg, 3, K, want_s, want_g, dtype)
    assert not bool(torch.cat(got[1], 1)[0][_label_mask(rows, 3, K)[0]].any())           # (the image without GT has no label element)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_an_odd_k_stores_single_elements_at_odd_offsets(dtype):
    K = 3
    anc = _anchor_set()
    gts, labels = _gts(K, seed=5)
    cls, box = _head(3, K, dtype, seed=5)
    m, nfg = _dense_matches("iou", anc, gts)
    rows = _matched(cls, box, anc, gts, labels, m)
    offs = torch.cat([i * K + c for i, c, *_ in rows])
    assert int((offs % 2 == 1).sum()) > 0 and int((offs % 2 == 0).sum()) > 0             # both halves of a dword are stored to
    want_s, want_g = _reference(rows, nfg, 3, 2.0)
    k3, got = _k3_then_qfl("iou", K, 2.0, anc, gts, labels, cls, box)
    _check(k3, got, rows, nfg, 3, K, want_s, want_g, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_a_clipped_dw_gives_the_clipped_boxs_quality(dtype):
    K = 5
    anc = _anchor_set()
    gts, labels = _gts(K)
    cls, box = _head(3, K, dtype, seed=2)
    m, nfg = _dense_matches("iou", anc, gts)
    first = [int(a) for a in (m[2] >= 0).nonzero().flatten().tolist() if a < SIZES[0] + SIZES[1]][:2]
    assert len(first) == 2
    for n, a in enumerate(first):
        lvl = 0 if a < SIZES[0] else 1
        box[lvl][2, a - lvl * SIZES[0], 2] = 6.0 if n else 60000.0                       # (60000: finite in fp16, exp of it is not)
    rows = _matched(cls, box, anc, gts, labels, m)
    want_s, want_g = _reference(rows, nfg, 3, 2.0, clipped_ok=True)
    k3, got = _k3_then_qfl("iou", K, 2.0, anc, gts, labels, cls, box)
    assert bool(torch.isfinite(got[0]).all()) and all(bool(torch.isfinite(g).all()) for g in got[1])
    _check(k3, got, rows, nfg, 3, K, want_s, want_g, dtype)


# ---- the op's other arguments ----------------------------------------------------------------------------------------------------
def test_the_fp16_prescale_goes_in_before_the_one_rounding_and_keeps_what_would_flush():
    from pytorch_retinanet_amd.config import LOGIT_SHIFT
    from pytorch_retinanet_amd.losses import box_quality_reference
    K, S = 5, 65536.0
    anc = _anchor_set()
    gts, labels = _gts(K)
    cls, box = _head(3, K, torch.float16, seed=3)
    m, nfg = _dense_matches("iou", anc, gts)
    rows = _matched(cls, box, anc, gts, labels, m)
    # four label elements of the last image get a logit whose sigma sits right at the row's quality: |sigma - q|^3 / (num_fg B) is
    # then far below fp16's smallest subnormal (6e-8)
    i, c, _, d, an, g = rows[2]
    q = box_quality_reference(d.double(), an.double(), g.double())
    near = [n for n in range(i.numel()) if 0.05 < float(q[n]) < 0.95][:4]
    assert len(near) == 4
    ccat = torch.cat(cls, 1)
    for n in near:
        ccat[2, i[n], c[n]] = float(torch.logit(q[n])) - LOGIT_SHIFT + 0.02
    cls = [t.contiguous() for t in torch.split(ccat, SIZES, dim=1)]
    rows = _matched(cls, box, anc, gts, labels, m)
    want_s, want_g = _reference(rows, nfg, 3, 2.0)
    tiny = [n for n in near if 0 < abs(float(want_g[2][n])) < 2.0 ** -26]
    assert len(tiny) >= 2, want_g[2][near]
    pre = torch.full((1,), S, device=DEV)
    k3, got = _k3_then_qfl("iou", K, 2.0, anc, gts, labels, cls, box, prescale=pre)
    _, plain = _k3_then_qfl("iou", K, 2.0, anc, gts, labels, cls, box)
    assert torch.equal(got[0], plain[0])                                   # the losses are not scaled
    _check(k3, got, rows, nfg, 3, K, want_s, want_g, torch.float16, scale=S)
    scaled, unscaled = torch.cat(got[1], 1), torch.cat(plain[1], 1)
    for n in tiny:
        assert float(unscaled[2, i[n], c[n]]) == 0.0 and float(scaled[2, i[n], c[n]]) != 0.0


def test_two_calls_give_the_same_bits_and_value_only_writes_no_gradient():
    K = 5
    anc = _anchor_set()
    gts, labels = _gts(K)
    cls, box = _head(3, K, torch.bfloat16, seed=1)
    _, first = _k3_then_qfl("atss", K, 1.5, anc, gts, labels, cls, box)
    _, second = _k3_then_qfl("atss", K, 1.5, anc, gts, labels, cls, box)
    assert torch.equal(first[0], second[0]) and all(torch.equal(a, b) for a, b in zip(first[1], second[1]))
    k3, value = _k3_then_qfl("atss", K, 1.5, anc, gts, labels, cls, box, want_grad=False)
    assert value[1] is None and value[2] is None and k3[1] is None
    assert torch.equal(value[0], first[0]) and float(value[0][0]) > float(k3[0][0])


def test_gt_capacity_staging_with_padded_gt_rows():
    K = 5
    anc = _anchor_set()
    gts, labels = _gts(K, seed=4)
    cls, box = _head(3, K, torch.float32, seed=4)
    m, nfg = _dense_matches("iou", anc, gts)
    rows = _matched(cls, box, anc, gts, labels, m)
    want_s, want_g = _reference(rows, nfg, 3, 2.0)
    k3, got = _k3_then_qfl("iou", K, 2.0, anc, gts, labels, cls, box, capacity=32)
    _check(k3, got, rows, nfg, 3, K, want_s, want_g, torch.float32)
    _, listed = _k3_then_qfl("iou", K, 2.0, anc, gts, labels, cls, box)
    assert all(torch.equal(a, b) for a, b in zip(got[1], listed[1]))       # the same gradients as from the plain GT list


def test_flag_words_past_one_grid_pass_with_ignored_rows_a_stale_index_a_bad_label_and_unflagged_garbage():
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.config import LOGIT_SHIFT
    big = 64 * 64 * 257                                                    # 16 448 flag words per image -> 257 strips
    sizes = [1_000_000, 40_000, big - 1_040_000]
    B, T, K = 2, 5, 1
    strips = ((big // 64) + 63) // 64
    assert B * strips == 514 > GRID_STRIPS
    assert ops.lib.rn_quality_focal_loss_workspace_bytes(B, big) == 128 * 8
    rng = np.random.default_rng(9)
    base = _anchor_set()
    anc = base[torch.arange(big) % A].contiguous()
    gts = [torch.from_numpy(synth.gt_boxes(rng, T, 64, 64, num_classes=K, wh_lo=6.0, wh_hi=40.0)[0].astype(np.float32)).reshape(-1, 4) for _ in range(B)]
    edge = [0, 1, 63, 64, 4095, 4096, 999_999, 1_000_000, 1_039_999, 1_040_000, big - 64, big - 1]
    flagged = [np.unique(np.concatenate([edge, np.arange(500_000, 500_070), rng.integers(0, big, 150)])),      # > 64 rows in one strip
               np.unique(np.concatenate([[0, 256 * 4096, 256 * 4096 + 24, big - 1], rng.integers(256 * 4096, big, 40), rng.integers(0, big, 100)]))]
    assert all(int((f >= 256 * 4096).sum()) > 0 for f in flagged)          # both images have rows in their last strip (strips 256 and 513)
    m = torch.full((B, big), 3, dtype=torch.int64)                         # unflagged entries hold a VALID index: reading one would show
    dense = torch.full((B, big), -1, dtype=torch.int64)
    bits = np.zeros((B, big), np.uint64)
    for b, f in enumerate(flagged):
        code = rng.integers(0, T, f.shape[0])
        code[rng.random(f.shape[0]) < 0.2] = -2                            # ignored rows: flagged, not matched
        code[0] = 2
        dense[b, f] = torch.from_numpy(code)
        m[b, f] = torch.from_numpy(code)
        bits[b, f] = 1
    stale = int(flagged[1][-1])                                            # a stale word beyond the image's rows is clamped to its last row
    m[1, stale], dense[1, stale] = 99, T - 1
    labels = [torch.ones(T, dtype=torch.int64) for _ in range(B)]
    labels[0][4] = 2                                                       # a label outside 1..K: its rows add nothing and write nothing
    bad = (dense[0] == 4)
    assert int(bad.sum()) > 0
    words = torch.from_numpy((bits.reshape(B, -1, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64).view(np.int64))
    nfg = (dense >= 0).sum(1).to(torch.int32)
    cls, box = _head(B, K, torch.float32, seed=6, sizes=sizes)
    gcls = [torch.full_like(c, 7.0) for c in cls]
    loss = torch.tensor([3.5, 9.0], device=DEV)
    off = ops.gt_offsets([T] * B, torch.device(DEV))
    ops.quality_focal_loss(cls, box, anc.to(DEV), torch.cat(gts).to(DEV), torch.cat(labels).to(DEV), off, m.to(DEV), nfg.to(DEV),
                           words.to(DEV), loss, gcls, beta=2.0, logit_shift=LOGIT_SHIFT)
    torch.cuda.synchronize()
    got = torch.cat(gcls, 1)[:, :, 0].cpu()
    live = dense.clone()
    live[0][bad] = -1
    assert torch.equal(got != 7.0, live >= 0)                              # exactly the matched rows with a valid label were written
    ccat, bcat = torch.cat(cls, 1).cpu(), torch.cat(box, 1).cpu()
    rows = []
    for b in range(B):
        i = (live[b] >= 0).nonzero().flatten()
        rows.append((i, torch.zeros_like(i), ccat[b, i, 0], bcat[b, i], anc[i], gts[b][live[b, i]]))
    want_s, want_g = _reference(rows, nfg, B, 2.0)
    assert float(loss[1]) == 9.0
    _close(loss[0].cpu(), 3.5 + want_s, RTOL[torch.float32], "classification loss")
    for b in range(B):
        _close(got[b, rows[b][0]], want_g[b], RTOL[torch.float32], f"label-element gradient, image {b}")


# ---- through the module and the model ------------------------------------------------------------------------------------------
def _losses_run(K, matcher, box_loss, cls_loss, beta, cls, box, anc, gts, labels, count=False):
    "forward_levels + backward of a RetinaNetLosses -> (f32[2] losses, [grad per cls level], [grad per box level], launches)."
    from pytorch_retinanet_amd import losses, ops
    crit = losses.RetinaNetLosses(K, matcher=matcher, box_loss=box_loss, cls_loss=cls_loss, qfl_beta=beta)
    cl = [c.clone().requires_grad_() for c in cls]
    bl = [b.clone().requires_grad_() for b in box]
    targets = [{"boxes": g.to(DEV), "labels": l.to(DEV)} for g, l in zip(gts, labels)]
    launches = None
    ops.enable_timing(True)
    try:
        out = crit.forward_levels(targets, cl, bl, [anc.to(DEV)] * len(gts))
        launches = {name: len(ev) for name, ev in ops.timing_events().items()}
    finally:
        ops.enable_timing(False)
    (out["classification_loss"] + out["regression_loss"]).backward()
    torch.cuda.synchronize()
    return (torch.stack([out["classification_loss"], out["regression_loss"]]).detach().cpu(), [t.grad.cpu() for t in cl],
            [t.grad.cpu() for t in bl], launches)


@pytest.mark.parametrize("matcher,box_loss", [("iou", "smooth_l1"), ("atss", "giou")])
def test_the_module_gives_the_op_level_numbers_and_backward_delivers_the_label_gradients(matcher, box_loss):
    K, beta = 5, 2.0
    anc = _anchor_set()
    gts, labels = _gts(K)
    cls, box = _head(3, K, torch.bfloat16, seed=1)
    loss, gcls, gbox, launches = _losses_run(K, matcher, box_loss, "qfl", beta, cls, box, anc, gts, labels)
    assert launches.get("quality_focal_loss") == 1 and launches.get("box_iou_loss", 0) == (1 if box_loss == "giou" else 0)
    _, want = _k3_then_qfl(matcher, K, beta, anc, gts, labels, cls, box)
    assert torch.equal(loss[0], want[0][0])
    assert all(torch.equal(a, b) for a, b in zip(gcls, want[1]))
    m, nfg = _dense_matches(matcher, anc, gts)
    mask = _label_mask(_matched(cls, box, anc, gts, labels, m), 3, K)
    assert int(mask.sum()) == int(nfg.sum()) and bool((torch.cat(gcls, 1)[mask] != 0).any())
    # against the focal run of the same module: the box side is the same, the class side is not
    loss_f, _, gbox_f, launches_f = _losses_run(K, matcher, box_loss, "focal", beta, cls, box, anc, gts, labels)
    assert "quality_focal_loss" not in launches_f                          # the default path launches nothing new
    assert {k: v for k, v in launches.items() if k != "quality_focal_loss"} == launches_f
    assert torch.equal(loss[1], loss_f[1]) and all(torch.equal(a, b) for a, b in zip(gbox, gbox_f)) and not torch.equal(loss[0], loss_f[0])


def test_the_default_models_loss_call_launches_nothing_new():
    import pytorch_retinanet_amd as P
    from pytorch_retinanet_amd import ops
    torch.manual_seed(5)
    images, tg = synth.e2e_inputs()
    images = [torch.from_numpy(i).to(DEV) for i in images]
    targets = [{"boxes": torch.from_numpy(np.asarray(b, np.float32)).to(DEV), "labels": torch.from_numpy(np.asarray(l, np.int64)).to(DEV)} for b, l in tg]
    seen = {}
    for kind in ("focal", "qfl"):
        net = P.Retinanet(num_classes=5, backbone_kind="resnet18", pretrained=False, min_size=128, max_size=160, cls_loss=kind,
                          box_decode="standard").to(DEV)
        net = net.to(memory_format=torch.channels_last).train()
        ops.enable_timing(True)
        try:
            out = net(images, targets)
            seen[kind] = {name: len(ev) for name, ev in ops.timing_events().items()}
        finally:
            ops.enable_timing(False)
        (out["classification_loss"] + out["regression_loss"]).backward()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out["classification_loss"])) and float(out["classification_loss"].detach()) > 0
        assert all(bool(torch.isfinite(p.grad).all()) for p in net.retinanet_head.classification_head.parameters() if p.grad is not None)
    assert "quality_focal_loss" not in seen["focal"] and seen["qfl"].get("quality_focal_loss") == 1
    assert {k: v for k, v in seen["qfl"].items() if k != "quality_focal_loss"} == seen["focal"]


class _Tiny(torch.nn.Module):
    "Per-level head outputs straight from parameters (plus the images' means): a net without convolutions, so a step is reproducible."

    def __init__(self, anchors, K):
        super().__init__()
        from pytorch_retinanet_amd.losses import RetinaNetLosses
        g = torch.Generator().manual_seed(3)
        self.cls = torch.nn.ParameterList([torch.nn.Parameter(torch.randn((1, s, K), generator=g) * 0.5 - 2.0) for s in SIZES])
        self.box = torch.nn.ParameterList([torch.nn.Parameter(torch.randn((1, s, 4), generator=g) * 0.2) for s in SIZES])
        self.retinanet_head = torch.nn.Module()
        self.retinanet_head.losses = RetinaNetLosses(K, matcher="atss", box_loss="giou", cls_loss="qfl")
        self.register_buffer("anchors", anchors.clone())

    def forward(self, images, targets):
        s = torch.stack(list(images)).mean(dim=(1, 2, 3)).view(-1, 1, 1)
        cls = [p + s for p in self.cls]
        box = [p * (1.0 + s) for p in self.box]
        return self.retinanet_head.losses.forward_levels(targets, cls, box, [self.anchors] * len(images))


def test_a_captured_step_replays_one_graph_over_changing_gt_counts():
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from pytorch_retinanet_amd.optim import MasterSGD
    K = 5
    anc = _anchor_set().to(DEV)
    net, twin = _Tiny(anc, K).to(DEV), _Tiny(anc, K).to(DEV)
    step = CapturedTrainStep(net, MasterSGD(net.parameters(), lr=1e-2, momentum=0.9), amp_dtype=None, eager_steps=1, gt_capacity="auto")
    rng = np.random.default_rng(13)
    counts = [[3, 8], [1, 0], [8, 8]]                                      # all in capacity class 8
    seen = []
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
        seen.append(float(got["classification_loss"]))
    assert step.captures == 1 and step.replays == len(counts) - 1
    assert all(np.isfinite(seen)) and seen[0] > 0 and seen[0] != seen[2]
    assert any(isinstance(k, tuple) and k and k[0] == "cls_loss" for k in next(iter(step._entries)))
