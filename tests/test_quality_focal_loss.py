"""CPU: Quality Focal Loss (``cls_loss="qfl"``) -- the torch restatements ``losses.quality_focal_loss_reference`` and
``losses.box_quality_reference`` of ``rn_quality_focal_loss``'s rule (include/retinanet_hip.h) in float64, the constructor / hparams
plumbing with its refusals and warning, the CPU-tensor loss path against a hand assembly, and the key of ``graph.CapturedTrainStep``.
(The kernel is in ``tests/test_quality_focal_loss_gpu.py``.)"""
import ctypes as C
import logging
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _logits_and_quality(n=64, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g, dtype=F64) * 3.0 - 1.0, torch.rand(n, generator=g, dtype=F64)


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", [2.0, 1.5])
def test_at_quality_one_it_is_the_focal_losss_positive_term_without_its_alpha(gamma):
    from pytorch_retinanet_amd.losses import RetinaNetLosses, quality_focal_loss_reference
    x, _ = _logits_and_quality()
    crit = RetinaNetLosses(3)
    crit.gamma = gamma
    l = quality_focal_loss_reference(x, torch.ones_like(x), beta=gamma, logit_shift=0.0)
    for i in range(x.shape[0]):                                            # (focal_loss is a sum: element by element)
        want = crit.focal_loss(x[i:i + 1], torch.ones(1, dtype=F64)) / (1.0 - crit.alpha)
        assert float(l[i]) == pytest.approx(float(want), rel=1e-12, abs=1e-300)


def test_at_quality_sigma_the_gradient_is_zero_and_the_loss_too():
    from pytorch_retinanet_amd.config import LOGIT_SHIFT
    from pytorch_retinanet_amd.losses import quality_focal_loss_reference
    x, _ = _logits_and_quality(seed=1)
    z = x + LOGIT_SHIFT
    e = torch.exp(-z.abs())
    q = torch.where(z >= 0, 1 / (1 + e), e * (1 / (1 + e)))                # sigma exactly as the restatement forms it
    x = x.requires_grad_()
    l = quality_focal_loss_reference(x, q)
    l.sum().backward()
    assert bool((x.grad == 0).all()) and bool((l == 0).all())


def test_beta_zero_is_plain_soft_target_bce():
    import torch.nn.functional as F
    from pytorch_retinanet_amd.losses import quality_focal_loss_reference
    x, q = _logits_and_quality(seed=2)
    l = quality_focal_loss_reference(x, q, beta=0.0, logit_shift=0.25)
    torch.testing.assert_close(l, F.binary_cross_entropy_with_logits(x + 0.25, q, reduction="none"), rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("beta", [2.0, 1.5, 0.0, 1.0])
def test_autograd_gives_the_detached_weight_times_sigma_minus_quality(beta):
    from pytorch_retinanet_amd.config import LOGIT_SHIFT
    from pytorch_retinanet_amd.losses import quality_focal_loss_reference
    x, q = _logits_and_quality(seed=3)
    x = x.requires_grad_()
    quality_focal_loss_reference(x, q, beta=beta).sum().backward()
    d = torch.sigmoid(x.detach() + LOGIT_SHIFT) - q
    torch.testing.assert_close(x.grad, d.abs().pow(beta) * d, rtol=1e-11, atol=1e-15)
    # mmdet differentiates through the weight; this restatement must not (the library's quirk Q3)
    if beta > 0:
        y = x.detach().clone().requires_grad_()
        s = torch.sigmoid(y + LOGIT_SHIFT)
        through = ((s - q).abs().pow(beta) * torch.nn.functional.binary_cross_entropy_with_logits(y + LOGIT_SHIFT, q, reduction="none")).sum()
        through.backward()
        assert not torch.allclose(y.grad, x.grad, rtol=1e-3, atol=0)


def test_the_quality_takes_no_gradient_and_keeps_the_dtype():
    from pytorch_retinanet_amd.losses import quality_focal_loss_reference
    x, q = _logits_and_quality(8, seed=4)
    q = q.requires_grad_()
    l = quality_focal_loss_reference(x.float().requires_grad_(), q)
    assert l.dtype == torch.float32
    l.sum().backward()
    assert q.grad is None


def _random_rows(n, seed):
    g = torch.Generator().manual_seed(seed)
    ctr = torch.rand((n, 2), generator=g, dtype=F64) * 48 + 8
    wh = torch.rand((n, 2), generator=g, dtype=F64) * 24 + 4
    anchors = torch.cat([ctr - wh / 2, ctr + wh / 2], 1)
    gctr = ctr + (torch.rand((n, 2), generator=g, dtype=F64) - 0.5) * 20
    gwh = torch.rand((n, 2), generator=g, dtype=F64) * 30 + 4
    gt = torch.cat([gctr - gwh / 2, gctr + gwh / 2], 1)
    return torch.randn((n, 4), generator=g, dtype=F64) * 0.3, anchors, gt


@pytest.mark.parametrize("reg_w", [(1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0)])
def test_the_quality_is_the_iou_inside_the_box_loss_restatement(reg_w):
    from pytorch_retinanet_amd.losses import box_iou_loss_reference, box_quality_reference
    from pytorch_retinanet_amd.ops import BOX_XFORM_CLIP
    deltas, anchors, gt = _random_rows(48, 7)
    deltas = deltas * torch.tensor(reg_w, dtype=F64)
    deltas[0, 2] = 9.0 * reg_w[2]                                          # a clipped slot goes the same way in both
    q = box_quality_reference(deltas.clone().requires_grad_(), anchors, gt, reg_w)
    assert not q.requires_grad and bool((q >= 0).all()) and bool((q <= 1).all())
    assert int((q > 0).sum()) > 10 and int((q == 0).sum()) > 0             # overlapping and disjoint pairs are both there
    # GIoU's row loss is (1 - iou) + (c - union) / c: take the penalty off again with the enclosing box computed here
    l = box_iou_loss_reference(deltas, anchors, gt, "giou", reg_w)
    t = deltas / torch.tensor(reg_w, dtype=F64)
    aw, ah = anchors[:, 2] - anchors[:, 0], anchors[:, 3] - anchors[:, 1]
    cx, cy = aw * t[:, 0] + (anchors[:, 0] + anchors[:, 2]) / 2, ah * t[:, 1] + (anchors[:, 1] + anchors[:, 3]) / 2
    w, h = aw * torch.exp(t[:, 2].clamp(max=BOX_XFORM_CLIP)), ah * torch.exp(t[:, 3].clamp(max=BOX_XFORM_CLIP))
    ew = torch.maximum(cx + w / 2, gt[:, 2]) - torch.minimum(cx - w / 2, gt[:, 0])
    eh = torch.maximum(cy + h / 2, gt[:, 3]) - torch.minimum(cy - h / 2, gt[:, 1])
    area = w * h + (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
    c = ew * eh
    # union = area - inter and iou = inter / union  =>  union = area / (1 + iou)
    pen = (c - area / (1 + q)) / c
    torch.testing.assert_close(1 - (l - pen), q, rtol=1e-9, atol=1e-9)
    # and the identical box has quality one
    same = torch.zeros((1, 4), dtype=F64)
    assert float(box_quality_reference(same, anchors[:1], anchors[:1])) == 1.0


# ---- plumbing ----------------------------------------------------------------------------------------------------------
def _net(**kw):
    import pytorch_retinanet_amd as P
    return P.Retinanet(num_classes=3, backbone_kind="resnet18", pretrained=False, **kw)


def test_constructors_carry_the_class_loss_to_the_loss():
    from pytorch_retinanet_amd.losses import RetinaNetLosses
    crit = RetinaNetLosses(3)
    assert (crit.cls_loss, crit.qfl_beta) == ("focal", 2.0)
    p = crit._params()
    assert (p.alpha, p.gamma) == (pytest.approx(crit.alpha), pytest.approx(crit.gamma))
    crit = RetinaNetLosses(3, cls_loss="qfl", qfl_beta=1.5)
    p = crit._params()
    assert (crit.cls_loss, crit.qfl_beta) == ("qfl", 1.5) and (p.alpha, p.gamma) == (1.0, 1.5)      # K3's contract: alpha = 1, gamma = beta
    crit = _net().retinanet_head.losses
    assert (crit.cls_loss, crit.qfl_beta) == ("focal", 2.0)
    crit = _net(cls_loss=None, qfl_beta=None).retinanet_head.losses
    assert (crit.cls_loss, crit.qfl_beta) == ("focal", 2.0)
    crit = _net(matcher="atss", box_loss="giou", box_decode="standard", cls_loss="qfl", qfl_beta=1.0).retinanet_head.losses
    assert (crit.matcher, crit.box_loss, crit.cls_loss, crit.qfl_beta) == ("atss", "giou", "qfl", 1.0)


def test_an_unknown_name_and_a_bad_beta_are_refused_with_the_choices():
    from pytorch_retinanet_amd.losses import RetinaNetLosses
    with pytest.raises(ValueError, match=r"cls_loss.*focal.*qfl"):
        RetinaNetLosses(3, cls_loss="vfl")
    with pytest.raises(ValueError, match=r"cls_loss.*focal.*qfl"):
        _net(cls_loss="varifocal")
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="qfl_beta"):
            RetinaNetLosses(3, cls_loss="qfl", qfl_beta=bad)
        with pytest.raises(ValueError, match="qfl_beta"):
            _net(cls_loss="qfl", qfl_beta=bad)
    RetinaNetLosses(3, cls_loss="qfl", qfl_beta=0.0)


def test_fused_matching_refuses_qfl(monkeypatch):
    from pytorch_retinanet_amd import losses
    monkeypatch.setattr(losses, "FUSE_MATCH", True)
    with pytest.raises(ValueError, match="RN_FUSE_MATCH"):
        losses.RetinaNetLosses(3, cls_loss="qfl")
    losses.RetinaNetLosses(3)                                              # the focal loss still takes the switch
    monkeypatch.setattr(losses, "FUSE_MATCH", False)
    crit = losses.RetinaNetLosses(3, cls_loss="qfl")
    monkeypatch.setattr(losses, "FUSE_MATCH", True)                        # switched on after construction: the call refuses
    with pytest.raises(ValueError, match="RN_FUSE_MATCH"):
        crit.forward_levels([], [torch.zeros(1, 4, 3)], [torch.zeros(1, 4, 4)], [torch.zeros(4, 4)])


def test_the_concatenated_path_refuses_qfl_instead_of_answering_with_the_focal_loss():
    from pytorch_retinanet_amd import losses
    targets = [{"boxes": torch.zeros(1, 4), "labels": torch.ones(1, dtype=torch.int64)}]
    crit = losses.RetinaNetLosses(3, cls_loss="qfl")
    with pytest.raises(ValueError, match="per-level"):
        crit(targets, {"cls_preds": torch.zeros(1, 5, 3), "bbox_preds": torch.zeros(1, 5, 4)}, [torch.zeros(5, 4)])
    with pytest.raises(ValueError, match="per-level"):
        crit.calc_loss(torch.zeros(5, 4), torch.zeros(5, 3), torch.zeros(5, 4), torch.ones(1, dtype=torch.int64), torch.zeros(1, 4))


@pytest.mark.parametrize("cls_loss,box_decode,warns", [("qfl", None, True), ("qfl", "reference", True), ("qfl", "standard", False),
                                                        ("focal", "reference", False), (None, None, False)])
def test_qfl_with_the_reference_decode_warns(cls_loss, box_decode, warns):
    seen = []

    class Catch(logging.Handler):
        def emit(self, record):
            seen.append(record.getMessage())
    log = logging.getLogger("qfl-test")
    h = Catch(level=logging.WARNING)
    log.addHandler(h)
    try:
        _net(cls_loss=cls_loss, box_decode=box_decode, logger=log)
    finally:
        log.removeHandler(h)
    hit = [m for m in seen if "qfl" in m and "box_decode" in m]
    assert bool(hit) == warns, seen


def test_hparams_reach_the_loss():
    import pytorch_retinanet_amd as P
    conf = P.load_hparams()
    assert conf.model.get("cls_loss") is None and conf.model.get("qfl_beta") is None         # commented out in the shipped file: the default holds
    conf.model.update(backbone_kind="resnet18", pretrained=False, num_classes=4, cls_loss="qfl", qfl_beta=1.5, box_decode="standard")
    crit = P.Retinanet(**conf.model).retinanet_head.losses
    assert (crit.cls_loss, crit.qfl_beta, crit.matcher, crit.box_loss) == ("qfl", 1.5, "iou", "smooth_l1")
    conf.model.update(cls_loss=None, qfl_beta=None)
    crit = P.Retinanet(**conf.model).retinanet_head.losses
    assert (crit.cls_loss, crit.qfl_beta) == ("focal", 2.0)
    text = open(os.path.join(ROOT, "pytorch_retinanet_amd", "hparams.yaml")).read()
    assert re.search(r"#\s*cls_loss:\s*qfl", text) and re.search(r"#\s*qfl_beta:", text)


def test_the_graph_key_names_the_class_loss_and_its_beta():
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from pytorch_retinanet_amd.losses import RetinaNetLosses
    from pytorch_retinanet_amd.optim import MasterSGD

    class Net(torch.nn.Module):
        def __init__(self, **kw):
            super().__init__()
            self.conv = torch.nn.Conv2d(3, 4, 1)
            self.retinanet_head = torch.nn.Module()
            self.retinanet_head.losses = RetinaNetLosses(3, **kw)

    def key(**kw):
        net = Net(**kw)
        step = CapturedTrainStep(net, MasterSGD(net.parameters(), lr=1e-2), amp_dtype=None, enabled=False)
        return step._signature([torch.zeros(3, 16, 16)], [{"boxes": torch.zeros(2, 4), "labels": torch.zeros(2, dtype=torch.int64)}])
    plain = key()
    assert key(cls_loss="focal") == plain
    assert not any(isinstance(k, tuple) and k and k[0] == "cls_loss" for k in plain)       # the default adds nothing to the key
    assert key(cls_loss="qfl") == plain + (("cls_loss", "qfl", 2.0),)
    assert key(cls_loss="qfl", qfl_beta=1.5) == plain + (("cls_loss", "qfl", 1.5),)
    assert key(cls_loss="qfl") != key(cls_loss="qfl", qfl_beta=1.5) != plain
    assert key(matcher="atss", box_loss="giou", cls_loss="qfl") == plain + (("matcher", "atss", 9), ("box_loss", "giou", 1.0), ("cls_loss", "qfl", 2.0))


# ---- the CPU-tensor loss path --------------------------------------------------------------------------------------------
def _cpu_batch():
    "Two levels (4 x 4 and 2 x 2 locations, 3 anchors each) on a 64-pixel canvas; B = 3 with an image without GT."
    rows = []
    for g, s in ((4, 16.0), (2, 32.0)):
        for y in range(g):
            for x in range(g):
                cx, cy = (x + 0.5) * s, (y + 0.5) * s
                rows += [[cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2] for w, h in ((s, s), (s * 1.4, s * 0.7), (s * 0.7, s * 1.4))]
    anc = torch.tensor(rows, dtype=torch.float32)
    sizes = [48, 12]
    gts = [torch.tensor([[14.0, 15.0, 33.0, 34.5], [30.0, 2.0, 62.0, 30.0]]), torch.zeros((0, 4)), torch.tensor([[1.0, 30.0, 31.5, 63.0]])]
    labels = [torch.tensor([2, 4]), torch.zeros((0,), dtype=torch.int64), torch.tensor([1])]
    g = torch.Generator().manual_seed(11)
    cls = [(torch.randn((3, s, 4), generator=g, dtype=F64) - 2.0).requires_grad_() for s in sizes]
    box = [(torch.randn((3, s, 4), generator=g, dtype=F64) * 0.2).requires_grad_() for s in sizes]
    return anc, sizes, gts, labels, cls, box


@pytest.mark.parametrize("box_loss", ["smooth_l1", "giou"])
@pytest.mark.parametrize("beta", [2.0, 1.5])
def test_the_cpu_tensor_path_is_the_restatements_hand_assembled(beta, box_loss):
    from pytorch_retinanet_amd import box_utils, losses
    from pytorch_retinanet_amd.config import LOGIT_SHIFT
    anc, sizes, gts, labels, cls, box = _cpu_batch()
    crit = losses.RetinaNetLosses(4, matcher="atss", atss_topk=3, cells=3, box_loss=box_loss, cls_loss="qfl", qfl_beta=beta)
    out = crit.forward_levels([{"boxes": g, "labels": l} for g, l in zip(gts, labels)], cls, box, [anc] * 3)
    # by hand: the restatement on the matched label elements, the focal restatement with alpha = 1 on everything else
    hand = losses.RetinaNetLosses(4)
    hand.alpha, hand.gamma = 1.0, beta
    c_all, b_all = torch.cat(cls, 1).detach(), torch.cat(box, 1).detach()
    want_c, want_r, matched = 0.0, 0.0, 0
    for b in range(3):
        z = c_all[b] + LOGIT_SHIFT
        if gts[b].shape[0] == 0:
            want_c += float(hand.focal_loss(z, torch.zeros_like(z)))       # / max(0, 1)
            continue
        m = box_utils.atss_matcher(anc, gts[b], sizes, 3, 3)
        rows = (m >= 0).nonzero().flatten()
        assert rows.numel() > 0
        matched += int(rows.numel())
        c = labels[b][m[rows]] - 1
        keep = torch.ones_like(z, dtype=torch.bool)
        keep[rows, c] = False
        neg = float(hand.focal_loss(z[keep], torch.zeros_like(z[keep])))
        q = losses.box_quality_reference(b_all[b, rows], anc[rows], gts[b][m[rows]])
        pos = float(losses.quality_focal_loss_reference(c_all[b, rows, c], q, beta).sum())
        want_c += (neg + pos) / int(rows.numel())
        if box_loss == "giou":
            want_r += float(losses.box_iou_loss_reference(b_all[b, rows], anc[rows], gts[b][m[rows]], "giou").sum()) / int(rows.numel())
    assert matched >= 3
    assert float(out["classification_loss"].detach()) == pytest.approx(want_c / 3, rel=1e-12)
    if box_loss == "giou":
        assert float(out["regression_loss"].detach()) == pytest.approx(want_r / 3, rel=1e-12)
    (out["classification_loss"] + out["regression_loss"]).backward()
    assert all(bool(torch.isfinite(t.grad).all()) for t in cls + box)
    assert bool(torch.cat([t.grad for t in cls], 1)[1].abs().sum() > 0)    # the image without GT still has its negatives' gradients
    assert not bool(torch.cat([t.grad for t in box], 1)[1].any())          # and no box gradient: the quality hands none down either


def test_the_cpu_tensor_path_has_no_max_iou_matcher():
    from pytorch_retinanet_amd import losses
    anc, sizes, gts, labels, cls, box = _cpu_batch()
    crit = losses.RetinaNetLosses(4, cls_loss="qfl")
    with pytest.raises(ValueError, match="atss"):
        crit.forward_levels([{"boxes": g, "labels": l} for g, l in zip(gts, labels)], cls, box, [anc] * 3)


# ---- the library's surface -------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_entry_points():
    from pytorch_retinanet_amd import _lib
    header = open(os.path.join(ROOT, "include", "retinanet_hip.h")).read()
    proto = re.search(r"\bint\s+rn_quality_focal_loss\s*\(([^;]*)\)\s*;", header)
    assert proto and re.search(r"\bsize_t\s+rn_quality_focal_loss_workspace_bytes\s*\(\s*int\s+B\s*,\s*int64_t\s+A\s*\)\s*;", header)
    names = [a.split()[-1].lstrip("*") for a in proto.group(1).replace("\n", " ").split(",")]
    assert names == ["cls_levels", "box_levels", "level_anchors", "L", "dtype", "B", "K", "anchors", "anchor_bstride", "gt_boxes", "gt_labels",
                     "gt_off", "matches", "special_rows", "num_fg", "reg_w", "beta", "logit_shift", "grad_prescale", "out_loss",
                     "grad_cls_levels", "workspace", "workspace_bytes", "stream"]
    assert len(_lib.SIGNATURES["rn_quality_focal_loss"][1]) == len(names)
    assert int(re.search(r"#define\s+RN_ABI_VERSION\s+(\d+)", header).group(1)) == 10 and _lib.lib.rn_version() == 10      # symbols only added
    for word in ("DETACHED", "mmdet", "num_fg", "alpha = 1", "gamma = beta"):
        assert word in header[header.index("Quality Focal Loss (round 34"):header.index("size_t rn_quality_focal_loss_workspace_bytes")]
    ws = _lib.lib.rn_quality_focal_loss_workspace_bytes
    assert ws(3, 765) == 8 and ws(8, 201600) == 100 * 8 and ws(2, 1 << 21) == 128 * 8
    assert ws(0, 765) == 0 and ws(3, 0) == 0 and ws(3, -5) == 0
    # arguments the call refuses before it launches anything (no device needed)
    f = _lib.lib.rn_quality_focal_loss
    one = (C.c_void_p * 1)(16)
    cnt, rw = (C.c_int64 * 1)(4), (C.c_float * 4)(1, 1, 1, 1)
    args = lambda **kw: [kw.get("cls", one), kw.get("box", one), cnt, kw.get("L", 1), kw.get("dtype", 0), 1, kw.get("K", 3), 16, 0, 16, 16, 16, 16,
                         kw.get("special", 16), 16, kw.get("rw", rw), kw.get("beta", 2.0), 1.0, None, 16, None, kw.get("ws", 16),
                         kw.get("nbytes", 8), None]
    EINVAL, EALIGN, EWORKSPACE = -1, f(*args(box=(C.c_void_p * 1)(8))), f(*args(nbytes=4))
    assert EALIGN != 0 and EWORKSPACE != 0 and len({EINVAL, EALIGN, EWORKSPACE}) == 3
    assert _lib.lib.rn_status_string(EALIGN) and _lib.lib.rn_status_string(EWORKSPACE)
    assert f(*args(special=None)) == EINVAL and f(*args(K=0)) == EINVAL and f(*args(L=0)) == EINVAL and f(*args(dtype=7)) == EINVAL
    for bad in (-0.5, float("inf"), float("nan")):
        assert f(*args(beta=bad)) == EINVAL
    assert f(*args(rw=(C.c_float * 4)(1, 0, 1, 1))) == EINVAL
    assert f(*args(cls=(C.c_void_p * 1)(6))) == EALIGN                     # an fp32 class tensor off its element alignment
