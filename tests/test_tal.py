"""CPU: the task-aligned matcher's restatement (``box_utils.task_aligned_matcher``) on hand-made cases with the expected matches
written out, the float64 bar of its fp32 metric, and the switch's surface: constructors, hparams, refusals, the graph key, the ABI.

The toy: six 8 x 8 anchors in a row, anchor i = [4 i, 0, 4 i + 8, 8], centres at x = 4, 8, ..., 24 and y = 4.  With zero deltas the
decoded box IS the anchor, so u is the anchor's IoU with the GT box; the score is the sigmoid of the logit + 1."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOY = torch.tensor([[4.0 * i, 0.0, 4.0 * i + 8.0, 8.0] for i in range(6)])
WIDE = [2.0, 0.0, 22.0, 8.0]            # centres 4 .. 20 (anchors 0-4) inside; anchors 1, 2, 3 lie inside it (u = 0.4), 0 and 4 stick out (u = 3/11)


def _t(rows):
    return torch.tensor(rows, dtype=torch.float32).reshape(-1, 4)


def _match(logits, gts, labels=None, deltas=None, **kw):
    from pytorch_retinanet_amd.box_utils import task_aligned_matcher
    cls = torch.tensor(logits, dtype=torch.float32).reshape(6, -1)
    box = torch.zeros(6, 4) if deltas is None else torch.tensor(deltas, dtype=torch.float32)
    gts = _t(gts)
    labels = torch.ones(gts.shape[0], dtype=torch.int64) if labels is None else torch.tensor(labels, dtype=torch.int64)
    return task_aligned_matcher(cls, box, TOY, gts, labels, **kw).tolist()


# ---- the rule ----------------------------------------------------------------------------------------------------------
def test_one_object_takes_the_topk_largest_metrics():
    # u = [3/11, .4, .4, .4, 3/11, -]; the logits make anchor 3 the best score, then 1, then 0: m = s * u^6
    logits = [1.0, 2.0, -3.0, 4.0, 0.0, 9.0]
    assert _match(logits, [WIDE], topk=2) == [-1, 0, -1, 0, -1, -1]
    assert _match(logits, [WIDE], topk=3) == [-1, 0, 0, 0, -1, -1]           # u^6 outweighs the score: anchor 2 (u = .4, s = .12) beats anchor 0
    assert _match(logits, [WIDE], topk=1) == [-1, -1, -1, 0, -1, -1]
    assert _match(logits, [WIDE], topk=2, alpha=1, beta=0) == [-1, 0, -1, 0, -1, -1]
    # anchor 5 has the best logit of all and is never a candidate: its centre (24) lies outside


def test_alpha_zero_ranks_by_iou_and_beta_zero_by_score():
    logits = [5.0, -2.0, -1.0, 0.0, 4.0, 9.0]
    assert _match(logits, [WIDE], topk=2, alpha=0, beta=1) == [-1, 0, 0, -1, -1, -1]       # u ties at .4: the lower anchors
    assert _match(logits, [WIDE], topk=3, alpha=0, beta=3) == [-1, 0, 0, 0, -1, -1]
    assert _match(logits, [WIDE], topk=2, alpha=1, beta=0) == [0, -1, -1, -1, 0, -1]       # the two best scores, whatever their IoU
    assert _match(logits, [WIDE], topk=2, alpha=3, beta=0) == [0, -1, -1, -1, 0, -1]
    assert _match(logits, [WIDE], topk=2, alpha=0, beta=0) == [0, 0, -1, -1, -1, -1]       # m = 1 everywhere: the lower anchors


def test_an_anchor_selected_by_two_objects_goes_to_the_larger_iou():
    tight = [8.0, 0.0, 16.0, 8.0]                                           # exactly anchor 2: u = 1 there, its only candidate
    zeros = [0.0] * 6
    assert _match(zeros, [WIDE, tight], topk=5) == [0, 0, 1, 0, 0, -1]
    assert _match(zeros, [tight, WIDE], topk=5) == [1, 1, 0, 1, 1, -1]


def test_duplicates_tie_to_the_lower_anchor_and_the_lower_row():
    zeros = [0.0] * 6
    assert _match(zeros, [WIDE, WIDE], topk=2) == [-1, 0, 0, -1, -1, -1]    # anchors 1, 2, 3 tie in m: the lower two; both rows want them: row 0
    assert _match(zeros, [WIDE, WIDE], topk=13) == [0, 0, 0, 0, 0, -1]


def test_a_centre_on_the_box_edge_is_not_a_candidate():
    zeros = [0.0] * 6
    assert _match(zeros, [[4.0, 0.0, 22.0, 8.0]], topk=13) == [-1, 0, 0, 0, 0, -1]         # anchor 0's centre x = 4 = gx1
    assert _match(zeros, [[2.0, 0.0, 20.0, 8.0]], topk=13) == [0, 0, 0, 0, -1, -1]         # anchor 4's centre x = 20 = gx2
    assert _match(zeros, [[2.0, 4.0, 22.0, 8.0]], topk=13) == [-1] * 6                     # every centre y = 4 = gy1
    assert _match(zeros, [[2.0, 0.0, 22.0, 4.0]], topk=13) == [-1] * 6                     # ... = gy2
    assert _match(zeros, [[float(np.nextafter(np.float32(4.0), np.float32(0.0))), 0.0, 22.0, 8.0]], topk=13) == [0, 0, 0, 0, 0, -1]


def test_topk_above_the_candidates_no_gt_and_rows_without_candidates():
    zeros = [0.0] * 6
    assert _match(zeros, [WIDE], topk=13) == [0, 0, 0, 0, 0, -1]
    assert _match(zeros, [], topk=13) == [-1] * 6
    assert _match(zeros, [WIDE], labels=[0]) == [-1] * 6                    # a label outside 1..K: no candidates, no error
    assert _match(zeros, [WIDE], labels=[2]) == [-1] * 6
    assert _match(zeros, [WIDE, WIDE], labels=[7, 1]) == [1, 1, 1, 1, 1, -1]
    two = [[0.0, 3.0]] * 6                                                   # K = 2: the label picks the logit column
    assert _match(two, [WIDE], labels=[2], topk=1, beta=0) == [0, -1, -1, -1, -1, -1]
    assert _match(zeros, [[2.0, 0.0, float("inf"), 8.0]]) == [-1] * 6       # a non-finite box
    assert _match(zeros, [[2.0, 0.0, float("nan"), 8.0]]) == [-1] * 6
    assert _match(zeros, [[22.0, 0.0, 2.0, 8.0]]) == [-1] * 6               # an empty one
    nan_box = [[0.0] * 4] * 2 + [[float("nan")] * 4] + [[0.0] * 4] * 3      # a NaN prediction drops its candidate, not the row
    assert _match(zeros, [WIDE], deltas=nan_box, topk=13) == [0, 0, -1, 0, 0, -1]
    # (with beta = 0 it stays: the box rule's union > 0 test fails for a NaN, so its u is 0, and u is then not a factor of m)
    assert _match(zeros, [WIDE], deltas=nan_box, topk=13, beta=0) == [0, 0, 0, 0, 0, -1]


def test_a_clipped_dw_is_the_clipped_boxs_iou():
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.box_utils import task_aligned_metric
    a = np.array([[8.0, 0.0, 16.0, 8.0]] * 2, np.float32)
    d = np.array([[0.0, 0.0, 50.0, 0.0], [0.0, 0.0, ops.BOX_XFORM_CLIP, 0.0]], np.float32)
    m, u, s = task_aligned_metric(np.zeros(2, np.float32), d, a, np.array([0.0, 0.0, 600.0, 8.0], np.float32))
    assert np.isfinite(m).all() and u[0] == u[1] > 0 and m[0] == m[1] and s[0] == s[1]


def test_the_fp32_metric_against_a_float64_evaluation_of_the_rule():
    """The bar: |m32 - m64| <= 32 * 2^-24 * m64.  The cases are chosen so that the bar follows from the rule's operation count, in
    units of 2^-24 (half an fp32 ulp, relative):
      the score -- z (<= 1 for |z| <= 2), e (0.5 + z's share), 1 + e (0.5), the quotient (0.5), e * r (0.5): s <= 4;
      set A, random deltas with the decoded box INSIDE the GT box and both around the origin (|coordinate| <= its size, so no
      cancellation: iw is the box's own width): t, exp, w: 1.5; cx +- w / 2: 0.5 each on a value <= w, the difference 0.5: iw <= 4.5,
      inter <= 9.5, the union is the GT area plus rounding noise (<= 1), the quotient 0.5: u <= 12.  m = s * u: <= 4 + 12 + 1 = 17, and
      m = s * s * u * u: <= 2 (4 + 12) = 32 -- the two exponent pairs asserted on this set;
      set B, the default exponents (1, 6) on dyadic geometry: integer anchors and boxes, deltas (j / 4, k / 4, 0, 0), so the decode,
      inter and union are exact and u is ONE rounded quotient (0.5): m <= 4 + 6 * 0.5 + 6 * 0.5 = 10."""
    from pytorch_retinanet_amd.box_utils import task_aligned_metric
    rng = np.random.default_rng(0)
    n = 4000
    bar = 32.0 * 2.0 ** -24

    def f64(logits, d, a, g, alpha, beta):
        # (valid on THIS test's domain only: reg_w = 1 and |dw|, |dh| far below the clip, so the reference has neither; what is asserted
        # is the bar on well-conditioned inputs -- it says nothing about the default exponents on boxes that cancel)
        logits, d, a, g = (v.astype(np.float64) for v in (logits, d, a, g))
        s = 1.0 / (1.0 + np.exp(-(logits + 1.0)))
        acx, acy, aw, ah = (a[:, 0] + a[:, 2]) / 2, (a[:, 1] + a[:, 3]) / 2, a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
        cx, cy, w, h = aw * d[:, 0] + acx, ah * d[:, 1] + acy, aw * np.exp(d[:, 2]), ah * np.exp(d[:, 3])
        iw = np.clip(np.minimum(cx + w / 2, g[2]) - np.maximum(cx - w / 2, g[0]), 0, None)
        ih = np.clip(np.minimum(cy + h / 2, g[3]) - np.maximum(cy - h / 2, g[1]), 0, None)
        inter = iw * ih
        u = inter / (w * h + (g[2] - g[0]) * (g[3] - g[1]) - inter)
        return s ** alpha * u ** beta

    worst = {}
    # set A
    half = rng.uniform(4.0, 8.0, size=(n, 2)).astype(np.float32)
    a = np.concatenate([-half, half], 1).astype(np.float32)                 # anchors around the origin
    d = np.concatenate([rng.uniform(-0.05, 0.05, (n, 2)), rng.uniform(-0.3, 0.3, (n, 2))], 1).astype(np.float32)
    g = np.array([-16.0, -16.0, 16.0, 16.0], np.float32)                     # contains every decoded box (half size <= 8 e^0.3 + 0.8 < 16)
    logits = rng.uniform(-3.0, 1.0, n).astype(np.float32)
    for alpha, beta in ((1, 1), (2, 2)):
        m, _, _ = task_aligned_metric(logits, d, a, g, alpha, beta)
        want = f64(logits, d, a, g, alpha, beta)
        worst[(alpha, beta)] = float(np.max(np.abs(m.astype(np.float64) - want) / want))
    # set B
    lo = rng.integers(-8, 0, size=(n, 2))
    a = np.concatenate([lo, lo + rng.integers(8, 17, size=(n, 2))], 1).astype(np.float32)
    d = np.concatenate([rng.integers(-1, 2, (n, 2)) / 4.0, np.zeros((n, 2))], 1).astype(np.float32)
    g = np.array([-6.0, -5.0, 9.0, 7.0], np.float32)
    m, u, _ = task_aligned_metric(logits, d, a, g, 1, 6)
    want = f64(logits, d, a, g, 1, 6)
    ok = want > 1e-20
    assert int(ok.sum()) > n // 2
    worst[(1, 6)] = float(np.max(np.abs(m[ok].astype(np.float64) - want[ok]) / want[ok]))
    print({k: v / 2.0 ** -24 for k, v in worst.items()})
    assert all(v <= bar for v in worst.values()), worst


# ---- the surface -------------------------------------------------------------------------------------------------------
def test_constructors_carry_the_matcher_to_the_loss():
    import pytorch_retinanet_amd as P
    from pytorch_retinanet_amd.losses import RetinaNetLosses
    crit = RetinaNetLosses(3, matcher="tal")
    assert (crit.matcher, crit.tal_topk, crit.tal_alpha, crit.tal_beta) == ("tal", 13, 1, 6)
    assert RetinaNetLosses(3).matcher == "iou"
    net = P.Retinanet(num_classes=3, backbone_kind="resnet18", pretrained=False, matcher="tal", tal_topk=9, tal_alpha=2, tal_beta=4,
                      box_decode="standard")
    crit = net.retinanet_head.losses
    assert (crit.matcher, crit.tal_topk, crit.tal_alpha, crit.tal_beta) == ("tal", 9, 2, 4) and list(crit.cells) == [9] * 5
    with pytest.raises(ValueError, match="integer"):                        # ultralytics' alpha = 0.5
        RetinaNetLosses(3, matcher="tal", tal_alpha=0.5)
    with pytest.raises(ValueError, match="integer"):
        RetinaNetLosses(3, matcher="tal", tal_beta=5.5)
    with pytest.raises(ValueError, match="0..8"):
        RetinaNetLosses(3, matcher="tal", tal_beta=9)
    with pytest.raises(ValueError, match="0..8"):
        RetinaNetLosses(3, matcher="tal", tal_alpha=-1)
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError, match="tal_topk"):
            RetinaNetLosses(3, matcher="tal", tal_topk=bad)
    with pytest.raises(ValueError):
        RetinaNetLosses(3, matcher="task")
    crit = RetinaNetLosses(3)                                               # a plain attribute: TOOD's switch between two epochs
    crit.matcher = "tal"
    with pytest.raises(ValueError, match="per-level"):
        crit([], {"cls_preds": torch.zeros(0, 6, 3), "bbox_preds": torch.zeros(0, 6, 4)}, [])


def test_hparams_reach_the_model_and_the_reference_decode_is_warned_about(caplog):
    import pytorch_retinanet_amd as P
    conf = P.load_hparams()
    conf.model.update(backbone_kind="resnet18", pretrained=False, num_classes=4, matcher="tal")
    with caplog.at_level("WARNING"):
        crit = P.Retinanet(**conf.model).retinanet_head.losses
    assert (crit.matcher, crit.tal_topk, crit.tal_alpha, crit.tal_beta) == ("tal", 13, 1, 6)
    assert any('matcher="tal"' in r.getMessage() and "box_decode" in r.getMessage() for r in caplog.records)
    caplog.clear()
    conf.model.update(box_decode="standard", tal_topk=5)
    with caplog.at_level("WARNING"):
        crit = P.Retinanet(**conf.model).retinanet_head.losses
    assert crit.tal_topk == 5 and not any('matcher="tal"' in r.getMessage() for r in caplog.records)
    conf.model.update(matcher=None, tal_topk=None)
    assert P.Retinanet(**conf.model).retinanet_head.losses.matcher == "iou"
    text = open(os.path.join(ROOT, "pytorch_retinanet_amd", "hparams.yaml")).read()
    assert "matcher: tal" in text and "tal_topk" in text and "tal_alpha" in text and "tal_beta" in text


def test_fused_matching_refuses_tal(monkeypatch):
    from pytorch_retinanet_amd import losses
    monkeypatch.setattr(losses, "FUSE_MATCH", True)
    with pytest.raises(ValueError, match="RN_FUSE_MATCH"):
        losses.RetinaNetLosses(3, matcher="tal")
    losses.RetinaNetLosses(3)                                               # the default matcher still takes the switch
    monkeypatch.setattr(losses, "FUSE_MATCH", False)
    crit = losses.RetinaNetLosses(3, matcher="tal")
    monkeypatch.setattr(losses, "FUSE_MATCH", True)                         # switched on after construction: the call refuses
    with pytest.raises(ValueError, match="RN_FUSE_MATCH"):
        crit.match_ahead([], torch.zeros(4, 4), [4])


def test_the_concatenated_path_and_packed_gt_on_the_cpu_are_refused():
    from pytorch_retinanet_amd import losses, ops
    crit = losses.RetinaNetLosses(3, matcher="tal")
    targets = [{"boxes": torch.zeros(1, 4), "labels": torch.ones(1, dtype=torch.int64)}]
    with pytest.raises(ValueError, match="per-level"):
        crit(targets, {"cls_preds": torch.zeros(1, 6, 3), "bbox_preds": torch.zeros(1, 6, 4)}, [TOY])
    with pytest.raises(ValueError, match="per-level"):
        crit.calc_loss(TOY, torch.zeros(6, 3), torch.zeros(6, 4), torch.ones(1, dtype=torch.int64), torch.zeros(1, 4))
    packed = ops.PackedGT.__new__(ops.PackedGT)
    with pytest.raises(ValueError, match="packed GT"):
        crit.forward_levels(packed, [torch.zeros(1, 6, 3)], [torch.zeros(1, 6, 4)], [TOY])
    with pytest.raises(ValueError, match="level"):
        crit._handle(targets, TOY, None)


def test_the_cpu_loss_runs_the_restatement():
    from pytorch_retinanet_amd import losses
    crit = losses.RetinaNetLosses(2, matcher="tal", cls_loss="qfl", box_loss="giou", tal_topk=2)
    cls = torch.tensor([[1.0, 0.0], [2.0, 0.0], [-3.0, 0.0], [4.0, 0.0], [0.0, 0.0], [9.0, 0.0]]).reshape(1, 6, 2).requires_grad_()
    box = torch.zeros(1, 6, 4, requires_grad=True)
    targets = [{"boxes": _t([WIDE]), "labels": torch.ones(1, dtype=torch.int64)}]
    out = crit.forward_levels(targets, [cls], [box], [TOY])
    (out["classification_loss"] + out["regression_loss"]).backward()
    assert bool(torch.isfinite(out["classification_loss"])) and float(out["regression_loss"]) > 0
    moved = (box.grad[0].abs().sum(1) > 0).tolist()
    assert moved == [False, True, False, True, False, False]                 # the two positives of the first test: anchors 1 and 3


def test_the_graph_key_names_the_matcher_and_its_three_numbers():
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
    assert key(matcher="iou") == plain and not any(isinstance(k, tuple) and k and k[0] == "matcher" for k in plain)
    assert key(matcher="tal") == plain + (("matcher", "tal", 13, 1, 6),)
    assert key(matcher="tal", tal_topk=9, tal_alpha=0, tal_beta=2) == plain + (("matcher", "tal", 9, 0, 2),)
    assert key(matcher="atss") == plain + (("matcher", "atss", 9),)


def test_header_and_binding_declare_the_entry_points():
    from pytorch_retinanet_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "retinanet_hip.h")).read()
    assert re.search(r"\bint\s+rn_tal_match\s*\(", header) and re.search(r"\bsize_t\s+rn_tal_match_workspace_bytes\s*\(", header)
    assert int(re.search(r"#define\s+RN_ABI_VERSION\s+(\d+)", header).group(1)) == 10
    for name in ("rn_tal_match", "rn_tal_match_workspace_bytes", "rn_tal_match_list_keys"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    ws = _lib.lib.rn_tal_match_workspace_bytes
    assert ws(2, 5, 3, 2, 13) == 2 * 5 * 8 + 3 * 320                        # the [B][A] table + three arrays of rows x L x topk records, 16-byte padded
    assert ws(2, 5, 3, 2, 65) == 0 and ws(2, 5, -1, 2, 13) == 0 and ws(2, 5, 3, 9, 13) == 0 and ws(0, 5, 3, 2, 13) == 0
    assert ops.tal_list_keys() >= 64 and ops.MATCHERS == ("iou", "atss", "tal")
    # the call refuses what the rule excludes, without a device (host-side checks come first)
    import ctypes as C
    null = C.c_void_p(0)
    ptrs, counts, cells = (C.c_void_p * 1)(16), (C.c_int64 * 1)(6), (C.c_int32 * 1)(1)
    rw = (C.c_float * 4)(1, 1, 1, 1)

    def call(topk=13, alpha=1, beta=6, level_w=None, K=3):
        return _lib.lib.rn_tal_match(ptrs, ptrs, counts, cells, level_w, 1, 0, 1, K, C.c_void_p(16), 0, C.c_void_p(16), C.c_void_p(16),
                                     C.c_void_p(16), topk, alpha, beta, rw, 1.0, C.c_void_p(16), null, null, 0, 0, C.c_void_p(16), 0, null)
    assert call() == -3                                                      # everything in order but the workspace: RN_EWORKSPACE
    assert call(alpha=9) == -1 and call(beta=-1) == -1 and call(topk=0) == -1 and call(K=0) == -1
    assert call(topk=65) == -4
    assert call(level_w=(C.c_int32 * 1)(4)) == -1 and call(level_w=(C.c_int32 * 1)(3)) == -3     # 6 anchors are no rows of 4 cells
