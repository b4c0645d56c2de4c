"""CPU: the ATSS matcher's restatement (``box_utils.atss_matcher``) against cases worked out by hand, and the plumbing that selects it:
the constructors, the hparams, the graph key, the refusal of ``RN_FUSE_MATCH=1`` and the header's declarations.  The HIP kernel is
compared with this restatement bit for bit in ``tests/test_atss_gpu.py``."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _t(rows):
    return torch.tensor(rows, dtype=torch.float32).reshape(-1, 4)


# ---- the rule, by hand -------------------------------------------------------------------------------------------------
# Level 0: a 2 x 2 grid of 8 x 8 anchors (one per location), level 1: one 16 x 16 anchor.  topk = 2, so k_0 = 2, k_1 = min(2, 1) = 1.
TOY = _t([[0, 0, 8, 8], [8, 0, 16, 8], [0, 8, 8, 16], [8, 8, 16, 16], [0, 0, 16, 16]])
TOY_SIZES = [4, 1]


def test_toy_grid_candidates_and_threshold_written_out():
    from pytorch_retinanet_amd.box_utils import atss_candidates, atss_matcher
    gt = _t([[0, 0, 8, 8]])                                   # centre (4, 4)
    # d2 to the level-0 centres (4,4) (12,4) (4,12) (12,12): 0, 64, 64, 128 -> anchor 0, then the tie 1 / 2 goes to the lower index
    cand = atss_candidates(TOY.numpy(), gt[0].numpy(), TOY_SIZES, 1, topk=2)
    assert cand.tolist() == [0, 1, 4]
    # IoUs of the list: 1 (the box itself), 0 (disjoint), 64 / 256 = 0.25
    mean = (1.0 + 0.0 + 0.25) / 3
    var = ((1.0 - mean) ** 2 + (0.0 - mean) ** 2 + (0.25 - mean) ** 2) / 2
    assert (1.0 - mean) ** 2 >= var and 0.25 - mean < 0       # anchor 0 passes mean + std, anchor 4 is below the mean
    assert atss_matcher(TOY, gt, TOY_SIZES, 1, topk=2).tolist() == [0, -1, -1, -1, -1]
    # the same box moved off the first cell: centre (5, 4) -> d2 1, 49, 65, 113 -> candidates 0, 1 and 4 again, IoU 56 / 72, 1 / 15, 0.25
    gt = _t([[1, 0, 9, 8]])
    assert atss_candidates(TOY.numpy(), gt[0].numpy(), TOY_SIZES, 1, topk=2).tolist() == [0, 1, 4]
    assert atss_matcher(TOY, gt, TOY_SIZES, 1, topk=2).tolist() == [0, -1, -1, -1, -1]
    # no targets: all background
    assert atss_matcher(TOY, _t([]), TOY_SIZES, 1, topk=2).tolist() == [-1] * 5


def test_ties_in_d2_go_to_the_lower_index_inside_a_location():
    from pytorch_retinanet_amd.box_utils import atss_candidates
    # three anchors per location, two locations: every anchor of a location has the same centre, so topk = 1 takes the location's three
    a = _t([[0, 0, 8, 8], [-2, 2, 10, 6], [2, -2, 6, 10], [8, 0, 16, 8], [6, 2, 18, 6], [10, -2, 14, 10]])
    assert atss_candidates(a.numpy(), np.array([9, 1, 15, 7], np.float32), [6], 3, topk=1).tolist() == [3, 4, 5]
    # the centre midway between the two locations: six equal d2, the cut at three keeps indices 0, 1, 2
    assert atss_candidates(a.numpy(), np.array([4, 0, 12, 8], np.float32), [6], 3, topk=1).tolist() == [0, 1, 2]


def test_one_candidate_has_zero_variance_and_the_centre_cut_is_strict_at_0_01():
    from pytorch_retinanet_amd.box_utils import atss_matcher
    c = np.float32(0.01)
    anchor = _t([[0.0, -4.0, float(c * np.float32(2)), 4.0]])            # centre ((0 + 0.02f) * 0.5f, 0) = (0.01f, 0) exactly
    assert (np.float32(anchor[0, 0]) + np.float32(anchor[0, 2])) * np.float32(0.5) == c
    # n == 1: mean = the IoU, dev = 0, var = 0 -> the statistics pass; what decides is the centre test
    on_the_cut = _t([[0.0, -2.0, 2.0, 2.0]])                              # acx - gx1 = 0.01f: not MORE than 0.01f
    assert atss_matcher(anchor, on_the_cut, [1], 1, topk=1).tolist() == [-1]
    just_inside = _t([[-1e-6, -2.0, 2.0, 2.0]])                           # 0.01f + 1e-6 rounds above 0.01f
    assert np.float32(c) - np.float32(-1e-6) > c
    assert atss_matcher(anchor, just_inside, [1], 1, topk=1).tolist() == [0]
    outside = _t([[1.0, -2.0, 3.0, 2.0]])
    assert atss_matcher(anchor, outside, [1], 1, topk=1).tolist() == [-1]


def test_conflicts_take_the_larger_iou_and_then_the_lower_index():
    from pytorch_retinanet_amd.box_utils import atss_matcher
    same = _t([[0, 0, 8, 8], [0, 0, 8, 8]])
    assert atss_matcher(TOY, same, TOY_SIZES, 1, topk=2).tolist() == [0, -1, -1, -1, -1]
    better_second = _t([[1, 0, 9, 8], [0, 0, 8, 8]])                       # anchor 0: IoU 56 / 72 with row 0, 1 with row 1
    assert atss_matcher(TOY, better_second, TOY_SIZES, 1, topk=2).tolist() == [1, -1, -1, -1, -1]


def test_level_sizes_must_cover_the_anchors():
    from pytorch_retinanet_amd.box_utils import atss_matcher
    with pytest.raises(ValueError):
        atss_matcher(TOY, _t([[0, 0, 8, 8]]), [4], 1)


# ---- plumbing ----------------------------------------------------------------------------------------------------------
def test_constructors_carry_the_matcher_to_the_loss():
    import pytorch_retinanet_amd as P
    from pytorch_retinanet_amd.losses import RetinaNetLosses
    net = P.Retinanet(num_classes=3, backbone_kind="resnet18", pretrained=False)
    crit = net.retinanet_head.losses
    assert (crit.matcher, crit.atss_topk) == ("iou", 9)
    net = P.Retinanet(num_classes=3, backbone_kind="resnet18", pretrained=False, matcher="atss", atss_topk=7)
    crit = net.retinanet_head.losses
    assert (crit.matcher, crit.atss_topk) == ("atss", 7) and list(crit.cells) == net.anchor_generator.num_anchors == [9] * 5
    assert RetinaNetLosses(3).matcher == "iou" and RetinaNetLosses(3, matcher="atss").cells == 9
    with pytest.raises(ValueError):
        RetinaNetLosses(3, matcher="nearest")
    with pytest.raises(ValueError):
        RetinaNetLosses(3, matcher="atss", atss_topk=0)


def test_hparams_reach_the_model():
    import pytorch_retinanet_amd as P
    conf = P.load_hparams()
    conf.model.update(backbone_kind="resnet18", pretrained=False, num_classes=4, matcher="atss")
    net = P.Retinanet(**conf.model)
    assert net.retinanet_head.losses.matcher == "atss" and net.retinanet_head.losses.atss_topk == 9
    conf.model.update(matcher=None, atss_topk=None)
    assert P.Retinanet(**conf.model).retinanet_head.losses.matcher == "iou"


def test_fused_matching_refuses_atss(monkeypatch):
    from pytorch_retinanet_amd import losses
    monkeypatch.setattr(losses, "FUSE_MATCH", True)
    with pytest.raises(ValueError, match="RN_FUSE_MATCH"):
        losses.RetinaNetLosses(3, matcher="atss")
    losses.RetinaNetLosses(3)                                  # the default matcher still takes the switch
    monkeypatch.setattr(losses, "FUSE_MATCH", False)
    crit = losses.RetinaNetLosses(3, matcher="atss")
    monkeypatch.setattr(losses, "FUSE_MATCH", True)            # switched on after construction: the call refuses
    with pytest.raises(ValueError, match="RN_FUSE_MATCH"):
        crit.match_ahead([], torch.zeros(4, 4), [4])


def test_match_ahead_needs_the_level_sizes_for_atss():
    from pytorch_retinanet_amd import losses, ops
    with pytest.raises(ValueError, match="level"):
        losses.RetinaNetLosses(3, matcher="atss").match_ahead([], torch.zeros(10, 4))
    with pytest.raises(ValueError, match="sum"):               # (the sizes themselves are checked in one place: where the matcher is launched)
        ops.atss_match(torch.zeros(10, 4), torch.zeros(0, 4), torch.zeros(1, dtype=torch.int32), 0, [4, 4], 9)


def test_the_concatenated_path_refuses_atss_instead_of_matching_by_iou():
    from pytorch_retinanet_amd import losses
    crit = losses.RetinaNetLosses(3, matcher="atss")
    targets = [{"boxes": torch.zeros(1, 4), "labels": torch.ones(1, dtype=torch.int64)}]
    with pytest.raises(ValueError, match="per-level"):
        crit(targets, {"cls_preds": torch.zeros(1, 5, 3), "bbox_preds": torch.zeros(1, 5, 4)}, [TOY])


def test_the_graph_key_names_the_matcher():
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
    assert not any(isinstance(k, tuple) and k and k[0] == "matcher" for k in plain)      # the default adds nothing to the key
    assert key(matcher="atss") == plain + (("matcher", "atss", 9),)
    assert key(matcher="atss", atss_topk=5) == plain + (("matcher", "atss", 5),)


def test_header_and_binding_declare_the_entry_points():
    from pytorch_retinanet_amd import _lib
    header = open(os.path.join(ROOT, "include", "retinanet_hip.h")).read()
    assert re.search(r"\bint\s+rn_atss_match\s*\(", header) and re.search(r"\bsize_t\s+rn_atss_match_workspace_bytes\s*\(", header)
    assert int(re.search(r"#define\s+RN_ABI_VERSION\s+(\d+)", header).group(1)) == 10
    assert "rn_atss_match" in _lib.SIGNATURES and "rn_atss_match_workspace_bytes" in _lib.SIGNATURES
    assert hasattr(_lib.lib, "rn_atss_match") and hasattr(_lib.lib, "rn_atss_match_workspace_bytes")
    # the size query refuses what the call refuses, without a device
    import ctypes as C
    off, cells = (C.c_int64 * 3)(0, 4, 5), (C.c_int32 * 2)(1, 1)
    ws = _lib.lib.rn_atss_match_workspace_bytes
    assert ws(2, 5, 3, off, cells, 2, 2) == 2 * 5 * 8 + 2 * 48            # the [B][A] table + two arrays of rows x (2 + 1) records, 16-byte padded
    assert ws(2, 6, 3, off, cells, 2, 2) == 0 and ws(2, 5, -1, off, cells, 2, 2) == 0 and ws(2, 5, 3, off, cells, 2, 0) == 0
