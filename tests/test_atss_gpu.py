"""GPU: the ATSS matcher kernel (``rn_atss_match``) against its restatement (``box_utils.atss_matcher`` on CPU tensors), bit for bit:
``matches``, ``num_fg`` and the special-row flag words; the loss with ``matcher="atss"`` against K3 fed the restatement's matches;
a captured train step replayed over batches whose GT counts differ.

Shapes: a real five-level anchor set for a 64 x 96 image (A = 1161, no multiple of 64; the top levels hold 18 and 9 anchors, fewer
than topk * cells = 81, so k_l = A_l there), and one 160 x 160 x 9 level (230 400 anchors: many steps of the selection's walk, with
compactions of its buffer).  The reference of a case is computed once on the CPU."""
import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 64, 96
SENTINEL = -7


# ---- anchors and the reference -----------------------------------------------------------------------------------------
_CACHE = {}


def _anchors(levels):
    "(anchors on the device, the same on the CPU, anchors per level) of an FPN-style layout, cached."
    key = tuple(levels)
    if key not in _CACHE:
        from pytorch_retinanet_amd import ops
        from pytorch_retinanet_amd.anchors import AnchorGenerator
        cells = list(AnchorGenerator().to(DEV).cell_anchors)[:len(levels)]
        anc = ops.anchors_emit(list(levels), cells, 0.0)
        _CACHE[key] = (anc, anc.cpu(), [h * w * 9 for h, w, _ in levels])
    return _CACHE[key]


def _pyramid():
    return _anchors(synth.levels_for(H, W))


def _words(matches):
    "The flag words of a [B, A] match tensor: bit (a & 63) of word a >> 6 = [matches != -1], as int64."
    B, A = matches.shape
    bits = np.zeros((B, (A + 63) // 64 * 64), np.uint64)
    bits[:, :A] = (matches.numpy() != -1)
    w = (bits.reshape(B, -1, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)
    return torch.from_numpy(w.view(np.int64))


def _reference(anchors_cpu, gts, sizes, topk=9):
    "(matches i64 [B,A], num_fg i32 [B], flag words) of the restatement; ``anchors_cpu`` [A,4] shared or [B,A,4]."
    from pytorch_retinanet_amd.box_utils import atss_matcher
    m = torch.stack([atss_matcher(anchors_cpu if anchors_cpu.dim() == 2 else anchors_cpu[b], g.cpu(), sizes, 9, topk) for b, g in enumerate(gts)])
    return m, (m >= 0).sum(1).to(torch.int32), _words(m)


def _run(anchors, gts, sizes, topk=9, **kw):
    from pytorch_retinanet_amd import ops
    boxes = torch.cat([g.reshape(-1, 4) for g in gts]).to(DEV) if gts else torch.zeros((0, 4), device=DEV)
    off = ops.gt_offsets([g.shape[0] for g in gts], torch.device(DEV))
    out = ops.atss_match(anchors, boxes, off, len(gts), sizes, 9, topk, want_special=True, **kw)
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


def _check(got, want):
    for g, w, name in zip(got, want, ("matches", "num_fg", "special")):
        assert g.dtype == w.dtype and torch.equal(g, w), (name, int((g != w).sum()))


def _boxes(rng, T):
    return torch.from_numpy(synth.gt_boxes(rng, T, H, W, num_classes=5, wh_lo=6.0, wh_hi=60.0)[0].astype(np.float32)).reshape(-1, 4)


# the hand-placed image: P3 centres lie on multiples of 8, so (20, 28) is a corner shared by four cells (a 4-way d2 tie) and (32, 24)
# is a centre (the nine anchors of the location tie, as everywhere); then two identical boxes and two nested ones
PLACED = torch.tensor([[10., 18., 30., 38.], [22., 10., 42., 38.], [40., 30., 70., 50.], [40., 30., 70., 50.],
                       [8., 8., 88., 56.], [30., 20., 60., 44.]])


def test_ties_conflicts_nested_boxes_and_an_empty_image_between_two():
    anc, anc_cpu, sizes = _pyramid()
    assert anc.shape[0] == 1161 and sizes[-2:] == [18, 9]
    gts = [PLACED, torch.zeros((0, 4)), _boxes(np.random.default_rng(0), 5)]
    want = _reference(anc_cpu, gts, sizes)
    _check(_run(anc, gts, sizes), want)
    m = want[0]
    assert int(want[1][0]) > 0 and int(want[1][1]) == 0 and int(want[1][2]) > 0 and int((m == -2).sum()) == 0
    assert 3 not in m[0].tolist() and 2 in m[0].tolist()                 # identical boxes: every conflict goes to the lower index
    assert 4 in m[0].tolist() and 5 in m[0].tolist()                     # both nested boxes keep anchors


@pytest.mark.parametrize("T", [1, 63, 64, 65])
def test_row_counts_around_a_wave(T):
    anc, anc_cpu, sizes = _pyramid()
    gts = [_boxes(np.random.default_rng(T), T), _boxes(np.random.default_rng(100 + T), 2)]
    _check(_run(anc, gts, sizes), _reference(anc_cpu, gts, sizes))


def test_per_image_anchors_and_another_topk():
    anc, anc_cpu, sizes = _pyramid()
    rng = np.random.default_rng(7)
    gts = [_boxes(rng, 4), _boxes(rng, 0), _boxes(rng, 7)]
    per = torch.stack([anc_cpu + 1.5 * b for b in range(3)])            # image b's anchors moved by 1.5 b pixels
    _check(_run(per.to(DEV), gts, sizes), _reference(per, gts, sizes))
    _check(_run(per.to(DEV), gts, sizes, topk=2), _reference(per, gts, sizes, topk=2))


@pytest.mark.parametrize("zeroed", [False, True], ids=["clear-num_fg", "num_fg-zeroed"])
@pytest.mark.parametrize("flagged_only", [False, True], ids=["dense", "flagged-only"])
def test_every_flag_combination(zeroed, flagged_only):
    from pytorch_retinanet_amd import ops
    anc, anc_cpu, sizes = _pyramid()
    gts = [PLACED, torch.zeros((0, 4)), _boxes(np.random.default_rng(0), 5)]
    want = _reference(anc_cpu, gts, sizes)
    B, A = 3, anc.shape[0]
    matches = torch.full((B, A), SENTINEL, dtype=torch.int64, device=DEV)
    num_fg = torch.full((B,), 0 if zeroed else 99, dtype=torch.int32, device=DEV)
    special = torch.full((B, (A + 63) // 64), -1, dtype=torch.int64, device=DEV)
    boxes = torch.cat(gts).to(DEV)
    off = ops.gt_offsets([g.shape[0] for g in gts], torch.device(DEV))
    ops.atss_match(anc, boxes, off, B, sizes, 9, out=(matches, num_fg, special), flagged_only=flagged_only,
                   zeroed_num_fg=num_fg if zeroed else None)
    torch.cuda.synchronize()
    assert torch.equal(num_fg.cpu(), want[1]) and torch.equal(special.cpu(), want[2])
    flagged = want[0] != -1
    assert torch.equal(matches.cpu()[flagged], want[0][flagged])
    rest = matches.cpu()[~flagged]
    assert bool((rest == (SENTINEL if flagged_only else -1)).all())      # FLAGGED_ONLY leaves every unflagged row as it was
    # the words are optional without FLAGGED_ONLY, and so is num_fg
    m2, n2 = ops.atss_match(anc, boxes, off, B, sizes, 9, want_num_fg=False)
    torch.cuda.synchronize()
    assert n2 is None and torch.equal(m2.cpu(), want[0])
    with pytest.raises(ValueError):
        ops.atss_match(anc, boxes, off, B, sizes, 9, flagged_only=True)


def test_a_row_bound_above_the_real_count_and_a_batch_without_rows():
    from pytorch_retinanet_amd import ops
    anc, anc_cpu, sizes = _pyramid()
    rng = np.random.default_rng(3)
    gts = [_boxes(rng, 3), _boxes(rng, 0), _boxes(rng, 6)]
    want = _reference(anc_cpu, gts, sizes)
    rows = torch.full((3 * 8, 4), float("nan"), device=DEV)             # capacity 8 per image: rows past gt_off[B] are never read
    rows[:9] = torch.cat(gts).to(DEV)
    off = torch.tensor([0, 3, 3, 9], dtype=torch.int32, device=DEV)
    got = ops.atss_match(anc, rows, off, 3, sizes, 9, want_special=True)
    torch.cuda.synchronize()
    _check([t.cpu() for t in got], want)
    none = [torch.zeros((0, 4))] * 2
    _check(_run(anc, none, sizes), _reference(anc_cpu, none, sizes))
    off0 = torch.zeros(3, dtype=torch.int32, device=DEV)                 # no rows on the device, a bound of 16 on the host
    got = ops.atss_match(anc, rows[:16], off0, 2, sizes, 9, want_special=True)
    torch.cuda.synchronize()
    _check([t.cpu() for t in got], _reference(anc_cpu, none, sizes))


def test_a_level_longer_than_one_selection_step():
    anc, anc_cpu, sizes = _anchors(((160, 160, 8),))
    assert sizes == [230400]
    rng = np.random.default_rng(11)
    big = torch.from_numpy(synth.gt_boxes(rng, 3, 1280, 1280, num_classes=5, wh_lo=30.0, wh_hi=400.0)[0].astype(np.float32)).reshape(-1, 4)
    gts = [torch.cat([big, torch.tensor([[600., 600., 680., 680.], [1236., 1240., 1280., 1280.]])]), big[:1] + 3.0]
    want = _reference(anc_cpu, gts, sizes)
    assert int(want[1].min()) > 0
    _check(_run(anc, gts, sizes), want)


def test_two_calls_give_the_same_bits_and_leave_the_table_zero():
    from pytorch_retinanet_amd import ops
    anc, anc_cpu, sizes = _pyramid()
    rng = np.random.default_rng(5)
    gts = [_boxes(rng, 9), PLACED]
    ws = ops.atss_workspace(torch.device(DEV), 2, anc.shape[0], 15, sizes, 9, 9)
    table = ws[:2 * anc.shape[0] * 8].view(torch.int64)
    assert int(table.abs().sum()) == 0
    first = _run(anc, gts, sizes, workspace=ws)
    assert int(table.abs().sum()) == 0
    second = _run(anc, gts, sizes, workspace=ws)
    assert int(table.abs().sum()) == 0
    _check(second, first)
    _check(first, _reference(anc_cpu, gts, sizes))
    assert ops.atss_workspace(torch.device(DEV), 2, anc.shape[0], 15, sizes, 9, 9) is ws            # cached: one zero-fill serves every call


# ---- the loss ----------------------------------------------------------------------------------------------------------
def _head(B, sizes, K=5, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    cls = [(torch.randn((B, s, K), device=DEV, generator=g) - 4.6).to(torch.bfloat16) for s in sizes]
    box = [(torch.randn((B, s, 4), device=DEV, generator=g) * 0.1).to(torch.bfloat16) for s in sizes]
    return cls, box


def test_the_atss_loss_is_k3_on_the_restatements_matches():
    from pytorch_retinanet_amd import losses, ops
    anc, anc_cpu, sizes = _pyramid()
    rng = np.random.default_rng(21)
    gts = [_boxes(rng, 6), _boxes(rng, 0), PLACED]
    labels = [torch.from_numpy(rng.integers(1, 6, size=g.shape[0])).to(DEV) for g in gts]
    B = len(gts)
    cls, box = _head(B, sizes)
    crit = losses.RetinaNetLosses(5, matcher="atss")
    cl = [c.clone().requires_grad_() for c in cls]
    bl = [b.clone().requires_grad_() for b in box]
    targets = [{"boxes": g.to(DEV), "labels": l} for g, l in zip(gts, labels)]
    out = crit.forward_levels(targets, cl, bl, [anc] * B)
    (out["classification_loss"] + out["regression_loss"]).backward()
    # K3 as the loss calls it, fed the restatement's matches
    m, nfg, words = _reference(anc_cpu, gts, sizes)
    gt_boxes, gt_labels, gt_off, _ = ops.gt_pack([t["boxes"] for t in targets], [t["labels"] for t in targets], torch.device(DEV))
    loss, gcls, gbox = ops.loss_fwd_bwd_levels(cls, box, anc, gt_boxes, gt_labels, gt_off, m.to(DEV), nfg.to(DEV), crit._params(), True,
                                               special=words.to(DEV), in_kernel_finalize=losses.IN_KERNEL_FINALIZE,
                                               form=losses.k3_form(int(gt_boxes.shape[0]), B))
    torch.cuda.synchronize()
    assert torch.equal(torch.stack([out["classification_loss"], out["regression_loss"]]).detach(), loss)
    for a, b in zip([t.grad for t in cl + bl], list(gcls) + list(gbox)):
        assert torch.equal(a, b)
    assert float(loss[1]) > 0
    # the side-stream launch gives the same handle contents
    ahead = crit.match_ahead(targets, [anc] * B, sizes)
    torch.cuda.current_stream().wait_event(ahead.done)
    torch.cuda.synchronize()
    assert torch.equal(ahead.num_fg.cpu(), nfg) and torch.equal(ahead.special.cpu(), words)
    flagged = m != -1
    assert torch.equal(ahead.matches.cpu()[flagged], m[flagged])
    # and the default matcher gives another answer on the same inputs (the two rules are not the same rule)
    iou = losses.RetinaNetLosses(5).forward_levels(targets, cls, box, [anc] * B)
    assert not torch.equal(iou["classification_loss"], out["classification_loss"].detach())


# ---- a captured step ---------------------------------------------------------------------------------------------------
class _Tiny(torch.nn.Module):
    "Per-level head outputs straight from parameters (plus the images' means): a net without convolutions, so a step is bit-reproducible."

    def __init__(self, anchors, sizes, K=5):
        super().__init__()
        from pytorch_retinanet_amd.losses import RetinaNetLosses
        g = torch.Generator().manual_seed(3)
        self.cls = torch.nn.ParameterList([torch.nn.Parameter(torch.randn((1, s, K), generator=g) * 0.5 - 4.6) for s in sizes])
        self.box = torch.nn.ParameterList([torch.nn.Parameter(torch.randn((1, s, 4), generator=g) * 0.1) for s in sizes])
        self.retinanet_head = torch.nn.Module()
        self.retinanet_head.losses = RetinaNetLosses(K, matcher="atss")
        self.register_buffer("anchors", anchors.clone())

    def forward(self, images, targets):
        s = torch.stack(list(images)).mean(dim=(1, 2, 3)).view(-1, 1, 1)
        cls = [p + s for p in self.cls]
        box = [p * (1.0 + s) for p in self.box]
        return self.retinanet_head.losses.forward_levels(targets, cls, box, [self.anchors] * len(images))


def test_a_captured_step_replays_one_graph_over_changing_gt_counts():
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from pytorch_retinanet_amd.optim import MasterSGD
    anc, _, sizes = _pyramid()
    net, twin = _Tiny(anc, sizes).to(DEV), _Tiny(anc, sizes).to(DEV)
    step = CapturedTrainStep(net, MasterSGD(net.parameters(), lr=1e-2, momentum=0.9), amp_dtype=None, eager_steps=1, gt_capacity="auto")
    rng = np.random.default_rng(13)
    counts = [[3, 8], [1, 0], [8, 8], [0, 5], [7, 2], [0, 0]]           # all in capacity class 8
    for i, cs in enumerate(counts):
        images = [torch.from_numpy(rng.random((3, H, W), dtype=np.float32)).to(DEV) for _ in cs]
        targets = [{"boxes": _boxes(rng, c).to(DEV), "labels": torch.from_numpy(rng.integers(1, 6, size=c)).to(DEV)} for c in cs]
        twin.load_state_dict(net.state_dict())                           # the eager step on the same weights
        want = twin(images, targets)
        got = step(images, targets)
        torch.cuda.synchronize()
        for k in ("classification_loss", "regression_loss"):
            assert torch.equal(got[k], want[k]), (i, k, float(got[k]), float(want[k]))
        assert bool(torch.isfinite(got["loss"]))
    assert step.captures == 1 and step.replays == len(counts) - 1
    (sig,) = step._entries.values()
    (entry,) = sig.steps.values()
    (ws, _), = entry.atss_ws.values()                                     # the entry's own table, zero after every replay
    assert int(ws[:2 * anc.shape[0] * 8].view(torch.int64).abs().sum()) == 0
    assert any(isinstance(k, tuple) and k and k[0] == "matcher" for k in next(iter(step._entries)))
