"""GPU: the task-aligned matcher kernel (``rn_tal_match``) against its restatement (``box_utils.task_aligned_matcher`` on CPU
tensors), bit for bit: ``matches``, ``num_fg`` and the special-row flag words; a captured call replayed over changing GT counts and
logits; a tiny net trained with ``matcher="tal"``, eagerly and inside ``CapturedTrainStep``.

Shapes: five levels of 8x8, 4x4, 2x2, 1x1, 1x1 locations x 9 anchors for a 64 x 64 image (A = 774, no multiple of 64), and one
16 x 16 x 9 level whose boxes cover fewer / more candidates than a workgroup's list holds (``ops.tal_list_keys()``).

The device's ``expf`` may differ from the restatement's by an ulp, so equality needs a margin, asserted ON THE RESTATEMENT ALONE
(``_margins``): in every case each object's k-th and (k+1)-th metric differ by more than 1e-4 relative, and the two best IoUs of a
conflicted anchor differ by more than 1e-4 relative unless the two rows' boxes are bit-identical (then the IoUs are too, on the
device as well, and the rule's tie-break decides).  A case that misses the margin FAILS; the seeds are fixed so that none does.
The reference of a case is computed once on the CPU."""
import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IMG = 64
PYRAMID = ((8, 8, 8), (4, 4, 16), (2, 2, 32), (1, 1, 64), (1, 1, 128))
WIDTHS = [8, 4, 2, 1, 1]
MARGIN = 1e-4
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
_CACHE = {}


def _anchors(levels):
    "(anchors on the device, the same on the CPU, anchors per level) of a grid layout, cached."
    key = tuple(levels)
    if key not in _CACHE:
        from pytorch_retinanet_amd import ops
        from pytorch_retinanet_amd.anchors import AnchorGenerator
        cells = list(AnchorGenerator().to(DEV).cell_anchors)
        cells = [cells[min(i, len(cells) - 1)] for i in range(len(levels))]
        anc = ops.anchors_emit(list(levels), cells, 0.0)
        _CACHE[key] = (anc, anc.cpu(), [h * w * 9 for h, w, _ in levels])
    return _CACHE[key]


def _words(matches):
    "The flag words of a [B, A] match tensor: bit (a & 63) of word a >> 6 = [matches != -1], as int64."
    B, A = matches.shape
    bits = np.zeros((B, (A + 63) // 64 * 64), np.uint64)
    bits[:, :A] = (matches.numpy() != -1)
    w = (bits.reshape(B, -1, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)
    return torch.from_numpy(w.view(np.int64))


def _margins(picks, boxes):
    """The margin condition of one image from its rows' ``task_aligned_candidates`` results: (the smallest relative gap between a
    k-th and a (k+1)-th metric, the smallest relative gap between the two best IoUs of a conflicted anchor; duplicated boxes exempt)."""
    gap_m, gap_u, wanted = np.inf, np.inf, {}
    for g, (sel, u, order, m, k) in enumerate(picks):
        if len(order) > k:
            gap_m = min(gap_m, float((m[k - 1] - m[k]) / m[k - 1]))
        for i, v in zip(sel.tolist(), u.tolist()):
            wanted.setdefault(i, []).append((v, g))
    for lst in wanted.values():
        if len(lst) > 1:
            lst.sort(key=lambda e: (-e[0], e[1]))
            (u0, g0), (u1, g1) = lst[0], lst[1]
            if not (u0 == u1 and np.array_equal(boxes[g0], boxes[g1])):
                gap_u = min(gap_u, (u0 - u1) / u0 if u0 > 0 else 0.0)
    return gap_m, gap_u


def _reference(cls_levels, box_levels, anchors_cpu, gts, labels, topk=13, alpha=1, beta=6, reg_w=(1.0, 1.0, 1.0, 1.0), shift=1.0):
    """(matches i64 [B,A], num_fg i32 [B], flag words) of the restatement on CPU copies of the head outputs (any dtype: widened),
    with the margin condition asserted.  ``gts`` / ``labels``: per image."""
    from pytorch_retinanet_amd.box_utils import task_aligned_candidates
    cls = torch.cat([c.detach().float().cpu() for c in cls_levels], 1).numpy()
    box = torch.cat([b.detach().float().cpu() for b in box_levels], 1).numpy()
    out, gap_m, gap_u = [], np.inf, np.inf
    for b, (g, l) in enumerate(zip(gts, labels)):
        a = (anchors_cpu if anchors_cpu.dim() == 2 else anchors_cpu[b]).numpy()
        t = g.detach().float().cpu().reshape(-1, 4).numpy()
        lab = l.detach().cpu().reshape(-1).numpy()
        m = np.full((a.shape[0],), -1, np.int64)
        best = np.full((a.shape[0],), -1.0, np.float32)
        picks = []
        for r in range(t.shape[0]):
            sel, u, order, mm = task_aligned_candidates(cls[b], box[b], a, t[r], int(lab[r]), topk, alpha, beta, reg_w, shift)
            picks.append((sel, u, order, mm, topk))
            for i, v in zip(sel, u):
                if v > best[i]:
                    best[i], m[i] = v, r
        gm, gu = _margins(picks, t)
        gap_m, gap_u = min(gap_m, gm), min(gap_u, gu)
        out.append(torch.from_numpy(m))
    print(f"margins: metric {gap_m:.3e} iou {gap_u:.3e}")
    assert gap_m > MARGIN and gap_u > MARGIN, ("the case misses the margin condition", gap_m, gap_u)
    m = torch.stack(out) if out else torch.zeros((0, anchors_cpu.shape[-2]), dtype=torch.int64)
    return m, (m >= 0).sum(1).to(torch.int32), _words(m)


def _head(sizes, B, K, dtype, seed, clip_every=0):
    "CPU head outputs in ``dtype``: logits around -2, deltas of 0.2; ``clip_every``: every n-th row's dw lies above the clip."
    g = torch.Generator().manual_seed(seed)
    cls = [(torch.randn((B, s, K), generator=g) * 1.5 - 2.0).to(dtype) for s in sizes]
    box = [(torch.randn((B, s, 4), generator=g) * 0.2) for s in sizes]
    if clip_every:
        for t in box:
            t[:, ::clip_every, 2] = 10.0
    return cls, [t.to(dtype) for t in box]


def _gts(counts, K, seed, size=IMG, lo=6.0, hi=56.0):
    rng = np.random.default_rng(seed)
    gts = [torch.from_numpy(synth.gt_boxes(rng, c, size, size, num_classes=K, wh_lo=lo, wh_hi=hi)[0].astype(np.float32)).reshape(-1, 4) for c in counts]
    labels = [torch.from_numpy(rng.integers(1, K + 1, size=c).astype(np.int64)) for c in counts]
    return gts, labels


def _run(cls, box, anchors, gts, labels, sizes, topk=13, alpha=1, beta=6, **kw):
    from pytorch_retinanet_amd import ops
    dev = torch.device(DEV)
    boxes = torch.cat([g.reshape(-1, 4) for g in gts]).to(DEV) if gts else torch.zeros((0, 4), device=DEV)
    lab = torch.cat([l.reshape(-1) for l in labels]).to(DEV) if labels else torch.zeros((0,), dtype=torch.int64, device=DEV)
    off = ops.gt_offsets([g.shape[0] for g in gts], dev)
    out = ops.tal_match([c.to(DEV) for c in cls], [b.to(DEV) for b in box], anchors, boxes, lab, off, len(gts), sizes, 9, topk, alpha, beta,
                        want_special=True, **kw)
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


def _check(got, want):
    for g, w, name in zip(got, want, ("matches", "num_fg", "special")):
        assert g.dtype == w.dtype and torch.equal(g, w), (name, int((g != w).sum()))


# ---- the pyramid -------------------------------------------------------------------------------------------------------
COUNTS = [0, 1, 13, 64, 65]
RESEED = {("fp16", 1, 1): 321}          # (the formula's seed puts one row's two best metrics 2e-5 apart: outside the margin condition)


@pytest.mark.parametrize("topk", [1, 13])
@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_the_pyramid_at_every_row_count_dtype_k_and_topk(dtype, K, topk):
    anc, anc_cpu, sizes = _anchors(PYRAMID)
    assert anc.shape[0] == 774 and sizes == [576, 144, 36, 9, 9]
    seed = RESEED.get((dtype, K, topk), 100 + 10 * list(DTYPES).index(dtype) + K)
    cls, box = _head(sizes, len(COUNTS), K, DTYPES[dtype], seed)
    gts, labels = _gts(COUNTS, K, seed)
    want = _reference(cls, box, anc_cpu, gts, labels, topk)
    assert int(want[1][0]) == 0 and int(want[1][3:].min()) > 0
    _check(_run(cls, box, anc, gts, labels, sizes, topk, level_w=WIDTHS), want)        # the cells under each box
    _check(_run(cls, box, anc, gts, labels, sizes, topk), want)                        # every level walked whole: the same bits


@pytest.mark.parametrize("alpha,beta", [(0, 1), (1, 0), (2, 3), (8, 8)])
def test_other_exponents_and_a_clipped_dw(alpha, beta):
    from pytorch_retinanet_amd import ops
    anc, anc_cpu, sizes = _anchors(PYRAMID)
    reg_w = (1.0, 1.0, 2.0, 2.0)
    cls, box = _head(sizes, 3, 5, torch.bfloat16, 7 + alpha, clip_every=2)   # every second row: dw = 10, t2 = dw / reg_w[2] = 5 > the clip
    gts, labels = _gts([6, 0, 13], 5, 21 + beta)
    # a clipped box is 62.5 anchors wide, so its IoU is small and it is selected only where candidates are scarce: a box around the one
    # centre (24, 24) of the first level has nine candidates, four of them clipped, and topk = 7 takes at least two of those
    gts[0] = torch.cat([gts[0], torch.tensor([[21.0, 21.0, 27.0, 27.0]])])
    labels[0] = torch.cat([labels[0], torch.tensor([3])])
    want = _reference(cls, box, anc_cpu, gts, labels, 7, alpha, beta, reg_w=reg_w, shift=0.5)
    t2 = torch.cat(box, 1)[..., 2].float() / reg_w[2]
    clipped = int(((want[0] >= 0) & (t2 > ops.BOX_XFORM_CLIP)).sum())
    print("selected rows above the clip:", clipped, "of", int(want[1].sum()))
    assert clipped > 0                                                       # the clip decides the IoU of rows that ARE selected
    got = _run(cls, box, anc, gts, labels, sizes, 7, alpha, beta, reg_w=reg_w, logit_shift=0.5, level_w=WIDTHS)
    _check(got, want)


def test_per_image_anchors_bad_labels_and_boxes_without_candidates():
    anc, anc_cpu, sizes = _anchors(PYRAMID)
    per = torch.stack([anc_cpu + 1.5 * b for b in range(3)])                # image b's anchors moved by 1.5 b pixels
    cls, box = _head(sizes, 3, 5, torch.float32, 3)
    gts, labels = _gts([5, 4, 7], 5, 4)
    labels[0][1], labels[2][0] = 0, 6                                        # outside 1..K: rows without candidates
    gts[1][2] = torch.tensor([30.0, 30.0, 30.0, 50.0])                       # an empty box
    gts[2][3] = torch.tensor([10.0, 10.0, float("inf"), 50.0])               # a non-finite one
    gts[0][4] = torch.tensor([33.0, 33.0, 39.0, 39.0])                       # a box that holds no anchor centre (they lie at multiples of 8)
    want = _reference(cls, box, per, gts, labels)
    _check(_run(cls, box, per.to(DEV), gts, labels, sizes, level_w=WIDTHS), want)
    _check(_run(cls, box, per.to(DEV), gts, labels, sizes), want)


def test_duplicated_boxes_and_logits_tie_to_the_lower_anchor_and_row():
    anc, anc_cpu, sizes = _anchors(PYRAMID)
    cls = [torch.full((1, s, 2), -1.0) for s in sizes]                       # every score equal, every delta zero: u is the anchor's IoU,
    box = [torch.zeros((1, s, 4)) for s in sizes]                            # equal for the mirrored anchors of a centred box
    gts = [torch.tensor([[8.0, 8.0, 56.0, 56.0], [8.0, 8.0, 56.0, 56.0], [16.0, 16.0, 48.0, 48.0]])]
    labels = [torch.tensor([1, 1, 1])]
    from pytorch_retinanet_amd.box_utils import task_aligned_matcher
    want_m = torch.stack([task_aligned_matcher(torch.cat(cls, 1)[0], torch.cat(box, 1)[0], anc_cpu, gts[0], labels[0], 13)])
    want = (want_m, (want_m >= 0).sum(1).to(torch.int32), _words(want_m))   # (exact ties by construction: no margin to assert)
    assert 1 not in want_m[0].tolist() and 0 in want_m[0].tolist()
    _check(_run(cls, box, anc, gts, labels, sizes, level_w=WIDTHS), want)


@pytest.mark.parametrize("zeroed", [False, True], ids=["clear-num_fg", "num_fg-zeroed"])
@pytest.mark.parametrize("flagged_only", [False, True], ids=["dense", "flagged-only"])
def test_every_flag_combination_and_packed_gt_with_padding_rows(zeroed, flagged_only):
    from pytorch_retinanet_amd import ops
    anc, anc_cpu, sizes = _anchors(PYRAMID)
    cls, box = _head(sizes, 3, 5, torch.bfloat16, 11)
    gts, labels = _gts([3, 0, 6], 5, 12)
    want = _reference(cls, box, anc_cpu, gts, labels)
    B, A, cap = 3, anc.shape[0], 8
    rows_c = torch.full((B * cap, 4), float("nan"), device=DEV)             # capacity 8 per image: 9 real rows, then padding rows
    lab_c = torch.full((B * cap,), 99, dtype=torch.int64, device=DEV)       # that are never read (gt_off ends in front of them)
    rows_c[:9], lab_c[:9] = torch.cat(gts).to(DEV), torch.cat(labels).to(DEV)
    off = torch.tensor([0, 3, 3, 9], dtype=torch.int32, device=DEV)
    matches = torch.full((B, A), -7, dtype=torch.int64, device=DEV)
    num_fg = torch.full((B,), 0 if zeroed else 99, dtype=torch.int32, device=DEV)
    special = torch.full((B, (A + 63) // 64), -1, dtype=torch.int64, device=DEV)
    ops.tal_match([c.to(DEV) for c in cls], [b.to(DEV) for b in box], anc, rows_c, lab_c, off, B, sizes, 9, out=(matches, num_fg, special),
                  flagged_only=flagged_only, zeroed_num_fg=num_fg if zeroed else None, level_w=WIDTHS)
    torch.cuda.synchronize()
    assert torch.equal(num_fg.cpu(), want[1]) and torch.equal(special.cpu(), want[2])
    flagged = want[0] != -1
    assert torch.equal(matches.cpu()[flagged], want[0][flagged])
    assert bool((matches.cpu()[~flagged] == (-7 if flagged_only else -1)).all())
    with pytest.raises(ValueError):
        ops.tal_match([c.to(DEV) for c in cls], [b.to(DEV) for b in box], anc, rows_c, lab_c, off, B, sizes, 9, flagged_only=True)


# ---- a box over more candidates than the list holds ----------------------------------------------------------------------
@pytest.mark.parametrize("side", ["below", "above", "far-above"])
@pytest.mark.parametrize("topk", [1, 13])
def test_each_side_of_the_list_capacity(side, topk):
    """"below": the list never fills.  "above": one compaction, in the step that carries the last candidates.  "far-above": a box over
    more than 1.5 lists (14 x 14 locations = 1 764 candidates) -- several hundred candidates arrive AFTER the first compaction, so
    they are tested against the running threshold, and what they add is compacted a second time at the end."""
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.box_utils import task_aligned_candidates
    keys = ops.tal_list_keys()
    anc, anc_cpu, sizes = _anchors(((16, 16, 8),))
    assert sizes == [2304] and 9 * 110 <= keys < 9 * 121 and 9 * 196 > keys + keys // 2
    # centres lie at 8 j: (4, 4)-(84, 92) holds 10 x 11 locations = 990 candidates, (4, 4)-(92, 92) 11 x 11 = 1089, (4, 4)-(116, 116) 14 x 14
    big = {"below": [4.0, 4.0, 84.0, 92.0], "above": [4.0, 4.0, 92.0, 92.0], "far-above": [4.0, 4.0, 116.0, 116.0]}[side]
    gts, labels = [torch.tensor([big, [100.0, 90.0, 127.0, 120.0]])], [torch.tensor([2, 1])]
    cls, box = _head(sizes, 1, 3, torch.bfloat16, 40 + topk)
    n = len(task_aligned_candidates(torch.cat(cls, 1)[0].float().numpy(), torch.cat(box, 1)[0].float().numpy(), anc_cpu.numpy(),
                                    gts[0][0].numpy(), 2, topk)[2])
    assert (n <= keys) if side == "below" else (n > keys if side == "above" else n > keys + keys // 2), (n, keys)
    want = _reference(cls, box, anc_cpu, gts, labels, topk)
    _check(_run(cls, box, anc, gts, labels, sizes, topk, level_w=[16]), want)
    _check(_run(cls, box, anc, gts, labels, sizes, topk), want)              # walked whole: 2304 anchors, several steps and compactions


# ---- the table ---------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_leave_the_table_zero():
    from pytorch_retinanet_amd import ops
    anc, anc_cpu, sizes = _anchors(PYRAMID)
    cls, box = _head(sizes, 2, 5, torch.float16, 5)
    gts, labels = _gts([9, 13], 5, 6)
    ws = ops.tal_workspace(torch.device(DEV), 2, anc.shape[0], 22, len(sizes), 13)
    table = ws[:2 * anc.shape[0] * 8].view(torch.int64)
    assert int(table.abs().sum()) == 0
    first = _run(cls, box, anc, gts, labels, sizes, workspace=ws, level_w=WIDTHS)
    assert int(table.abs().sum()) == 0
    second = _run(cls, box, anc, gts, labels, sizes, workspace=ws, level_w=WIDTHS)
    assert int(table.abs().sum()) == 0
    _check(second, first)
    _check(first, _reference(cls, box, anc_cpu, gts, labels))
    assert ops.tal_workspace(torch.device(DEV), 2, anc.shape[0], 22, len(sizes), 13) is ws


def test_a_captured_call_replays_over_changing_gt_counts_and_logits():
    from pytorch_retinanet_amd import ops
    dev = torch.device(DEV)
    anc, anc_cpu, sizes = _anchors(PYRAMID)
    B, K, cap = 2, 5, 16
    cls_d = [torch.zeros((B, s, K), dtype=torch.bfloat16, device=DEV) for s in sizes]
    box_d = [torch.zeros((B, s, 4), dtype=torch.bfloat16, device=DEV) for s in sizes]
    rows = torch.zeros((B * cap, 4), device=DEV)
    lab = torch.ones((B * cap,), dtype=torch.int64, device=DEV)
    off = torch.zeros((B + 1,), dtype=torch.int32, device=DEV)
    out = ops.iou_match_outputs(B, anc.shape[0], dev)
    ws = ops.tal_workspace(dev, B, anc.shape[0], B * cap, len(sizes), 13)

    def call():
        ops.tal_match(cls_d, box_d, anc, rows, lab, off, B, sizes, 9, out=out, workspace=ws, level_w=WIDTHS)

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for i, counts in enumerate([[3, 16], [0, 7], [16, 0], [5, 5], [0, 0]]):
        cls, box = _head(sizes, B, K, torch.bfloat16, 60 + i)
        gts, labels = _gts(counts, K, 70 + i)
        for d, s in zip(cls_d + box_d, cls + box):
            d.copy_(s.to(DEV))
        n = sum(counts)
        rows.fill_(float("nan"))
        lab.fill_(99)
        if n:
            rows[:n] = torch.cat(gts).to(DEV)
            lab[:n] = torch.cat(labels).to(DEV)
        off.copy_(torch.tensor([0, counts[0], n], dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        _check([t.cpu() for t in out], _reference(cls, box, anc_cpu, gts, labels))
    assert int(ws[:B * anc.shape[0] * 8].view(torch.int64).abs().sum()) == 0


# ---- end to end --------------------------------------------------------------------------------------------------------
def _net(seed=11):
    import pytorch_retinanet_amd as P
    from pytorch_retinanet_amd.optim import MasterSGD, use_16bit_conv_weights
    torch.manual_seed(seed)
    net = P.Retinanet(num_classes=5, backbone_kind="resnet18", pretrained=False, min_size=96, max_size=120, matcher="tal", cls_loss="qfl",
                      box_loss="giou", box_decode="standard").to(DEV)
    net = net.to(memory_format=torch.channels_last).train()
    use_16bit_conv_weights(net, torch.bfloat16)
    return net, MasterSGD(net.parameters(), lr=1e-2, momentum=0.9, weight_decay=1e-3)


def _batches(size_sets, count_sets, seed):
    rng = np.random.default_rng(seed)
    out = []
    for sizes, counts in zip(size_sets, count_sets):
        images = [torch.from_numpy(rng.random((3, h, w), dtype=np.float32)).to(DEV) for h, w in sizes]
        targets = []
        for (h, w), c in zip(sizes, counts):
            b = torch.from_numpy(synth.gt_boxes(rng, c, h, w, num_classes=5, wh_lo=20.0, wh_hi=70.0)[0].astype(np.float32)).reshape(-1, 4)
            targets.append({"boxes": b.to(DEV), "labels": torch.from_numpy(rng.integers(1, 6, size=c).astype(np.int64)).to(DEV)})
        out.append((images, targets))
    return out


class _Spy:
    "Keeps what the loss's matcher launch read and wrote (``losses._launch_matcher``), by reference."

    def __init__(self, monkeypatch):
        from pytorch_retinanet_amd import losses
        self.calls, real = [], losses._launch_matcher

        def spy(h, out=None, heads=None):
            real(h, out, heads)
            if not torch.cuda.is_current_stream_capturing():                 # (nothing of a capture is kept: its buffers belong to the graph's pool)
                self.calls.append((h, heads))
        monkeypatch.setattr(losses, "_launch_matcher", spy)

    def check_last(self):
        "The last launch's outputs against the restatement on the head outputs it read."
        h, (cls, box, params) = self.calls[-1]
        torch.cuda.synchronize()
        assert h.rule[0] == "tal" and h.rule[6] is not None                  # the model passed its grid widths
        off = h.gt_off.cpu().tolist()
        gts = [h.gt_boxes[off[b]:off[b + 1]].cpu() for b in range(h.B)]
        labels = [h.gt_labels[off[b]:off[b + 1]].cpu() for b in range(h.B)]
        want = _reference(cls, box, h.anchors.cpu(), gts, labels, h.rule[3], h.rule[4], h.rule[5], tuple(params.reg_w), params.logit_shift)
        assert torch.equal(h.num_fg.cpu(), want[1]) and torch.equal(h.special.cpu(), want[2])
        flagged = want[0] != -1
        assert torch.equal(h.matches.cpu()[flagged], want[0][flagged])       # (written at the flagged rows only)
        return int(want[1].sum())


def test_a_training_step_of_the_model_matches_by_its_own_outputs(monkeypatch):
    spy = _Spy(monkeypatch)
    net, opt = _net()
    (images, targets), = _batches([[(96, 120), (80, 120)]], [[3, 2]], seed=2)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = net(images, targets)
    (out["classification_loss"] + out["regression_loss"]).backward()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(out[k])) and float(out[k].detach()) > 0 for k in ("classification_loss", "regression_loss"))
    assert all(bool(torch.isfinite(p.grad).all()) for p in net.parameters() if p.grad is not None)
    assert len(spy.calls) == 1 and spy.check_last() > 0


def test_one_capture_serves_several_replays_with_both_capacity_modes(monkeypatch):
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    spy = _Spy(monkeypatch)
    net, opt = _net()
    step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=1, gt_capacity="auto", image_capacity="auto")
    sets = [[(128, 160), (100, 150)], [(64, 80), (60, 60)], [(112, 140), (90, 160)], [(96, 120), (120, 121)]]
    data = _batches(sets, [[3, 5], [8, 0], [1, 7], [4, 4]], seed=3)          # all in GT class 8 and canvas class 96 x 128
    losses = []
    for i, (images, targets) in enumerate(data):
        losses.append(float(step(images, targets)["loss"]))
        if i == 0:
            # the step's first call runs eagerly, on the staged images and the packed GT the replays read: its matcher launch against
            # the restatement on the head outputs it read
            assert len(spy.calls) == 1 and spy.check_last() >= 0
            spy.calls.clear()                                                # (nothing of the eager step is held while the next one is captured)
    assert not spy.calls                                                     # the capture kept nothing, the replays went through the graph
    torch.cuda.synchronize()
    assert np.all(np.isfinite(losses)) and step.captures == 1 and step.replays == len(data) - 1
    assert any(isinstance(k, tuple) and k and k[0] == "matcher" and k[1:] == ("tal", 13, 1, 6) for k in next(iter(step._entries)))
