"""CPU: the GT capacity mode's host side (``graph.CapturedTrainStep(gt_capacity=...)``) -- the class of a batch, the accepted
settings, and the graph key that makes batches with different box counts share one captured step."""
import pytest
import torch

from pytorch_retinanet_amd import graph
from pytorch_retinanet_amd.graph import GT_CAPACITY_CLASSES, CapturedTrainStep, gt_capacity_class, gt_capacity_classes


@pytest.mark.parametrize("counts, want", [
    ([8], 8), ([9], 32), ([1, 9, 3], 32), ([32], 32), ([33], 128), ([128], 128), ([129], 512), ([512], 512),
    ([513], None), ([0, 600], None), ([0, 0], 8), ([], 8), ([1], 8),
])
def test_capacity_class_boundaries(counts, want):
    assert gt_capacity_class(counts, GT_CAPACITY_CLASSES) == want


def test_capacity_class_custom_classes():
    assert gt_capacity_class([5], (4, 16)) == 16
    assert gt_capacity_class([4, 0], (4, 16)) == 4
    assert gt_capacity_class([17], (4, 16)) is None


def test_capacity_settings():
    assert gt_capacity_classes(None) is None
    assert gt_capacity_classes("auto") == (8, 32, 128, 512)
    assert gt_capacity_classes([4, 16, 64]) == (4, 16, 64)
    assert gt_capacity_classes((1,)) == (1,)


@pytest.mark.parametrize("bad", ["yes", "", [], [8, 8], [32, 8], [0, 8], [-1], [8.0, 32], [True, 4], 8, object(), ["8"]])
def test_bad_capacity_settings_are_rejected(bad):
    with pytest.raises(ValueError):
        gt_capacity_classes(bad)
    net = torch.nn.Linear(2, 2)
    with pytest.raises(ValueError):
        CapturedTrainStep(net, torch.optim.SGD(net.parameters(), lr=0.1), gt_capacity=bad)


def _batch(counts, hw=(128, 160)):
    images = [torch.zeros(3, *hw) for _ in counts]
    targets = [{"boxes": torch.zeros(c, 4), "labels": torch.ones(c, dtype=torch.int64)} for c in counts]
    return images, targets


def _stepper(gt_capacity):
    net = torch.nn.Linear(2, 2)
    return CapturedTrainStep(net, torch.optim.SGD(net.parameters(), lr=0.1), gt_capacity=gt_capacity)


def test_signature_keys_by_capacity_class():
    s = _stepper("auto")
    a = s._signature(*_batch([3, 9]))
    assert a == s._signature(*_batch([32, 0]))                     # both in class 32
    assert a[1] == ("gt_cap", 32)
    assert a != s._signature(*_batch([3, 8]))                      # class 8
    assert a != s._signature(*_batch([3, 33]))                     # class 128
    assert a != s._signature(*_batch([3, 9], hw=(128, 192)))       # another image shape
    assert a != s._signature(*_batch([3, 9, 1]))                   # another batch size
    assert s._signature(*_batch([0, 0])) == s._signature(*_batch([8, 1]))


def test_signature_falls_back_to_exact_shapes_above_the_last_class():
    s = _stepper((4, 16))
    over = s._signature(*_batch([17, 2]))
    assert over[1] != ("gt_cap", 16) and over != s._signature(*_batch([18, 2]))
    assert over == _stepper(None)._signature(*_batch([17, 2]))


def test_capacity_off_keeps_exact_shapes():
    s = _stepper(None)
    assert s.gt_capacity is None
    assert s._signature(*_batch([3, 9])) != s._signature(*_batch([9, 3]))
    assert s._signature(*_batch([3, 9])) == s._signature(*_batch([3, 9]))


def test_packed_gt_is_refused_by_the_reference_loss_entry_points():
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.losses import RetinaNetLosses
    p = ops.PackedGT(torch.zeros(16, 4), torch.zeros(16, dtype=torch.int64), torch.zeros(3, dtype=torch.int32),
                     torch.zeros(2, dtype=torch.int32), 8)
    assert (p.rows, p.B, p.cap_per_image) == (16, 2, 8)
    with pytest.raises(TypeError):
        RetinaNetLosses(5)(p, {"cls_preds": torch.zeros(2, 10, 5), "bbox_preds": torch.zeros(2, 10, 4)}, [torch.zeros(10, 4)] * 2)
    assert graph._net_targets(p) is p
