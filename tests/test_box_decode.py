"""CPU: the standard box decode (``box_decode="standard"``) -- the numpy restatement ``box_utils.decode_boxes_reference`` against a
float64 evaluation of the numbered rule in include/retinanet_hip.h, what the feature is for (the standard decode inverts
``bbox_2_activ``, the reference decode does not), and the names at every layer: ops, box_utils, the model, the hparams, the
warning and the key of ``graph.CapturedPredict``.  (The kernels and whole predicts are in ``tests/test_box_decode_gpu.py``.)

Bars: ``rtol=1e-5, atol=1e-3`` for boxes, SURVEY 8d's bar for K4."""
import logging
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG_W = (10.0, 10.0, 5.0, 5.0)
RTOL, ATOL = 1e-5, 1e-3


def rule_f64(d, a, reg_w, clip):
    "The standard rule, steps 1-6, in float64 on the fp32 inputs' values."
    d, a = np.asarray(d, np.float64), np.asarray(a, np.float64)
    t = d / np.asarray(reg_w, np.float64)
    acx, acy = (a[..., 0] + a[..., 2]) / 2, (a[..., 1] + a[..., 3]) / 2
    aw, ah = a[..., 2] - a[..., 0], a[..., 3] - a[..., 1]
    cx, cy = aw * t[..., 0] + acx, ah * t[..., 1] + acy
    w, h = aw * np.exp(np.minimum(t[..., 2], clip)), ah * np.exp(np.minimum(t[..., 3], clip))
    return np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1)


def random_anchors(rng, n, lo=16.0, hi=512.0, span=1000.0):
    cx, cy = rng.uniform(0, span, n), rng.uniform(0, span, n)
    w, h = rng.uniform(lo, hi, n), rng.uniform(lo, hi, n)
    return np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(np.float32)


def iou_rows(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    iw = np.clip(np.minimum(a[:, 2], b[:, 2]) - np.maximum(a[:, 0], b[:, 0]), 0, None)
    ih = np.clip(np.minimum(a[:, 3], b[:, 3]) - np.maximum(a[:, 1], b[:, 1]), 0, None)
    inter = iw * ih
    return inter / ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]) + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) - inter)


def gt_near(rng, anchors, lo=0.3, hi=0.9):
    "One GT box per anchor with IoU in [lo, hi]: shifted and rescaled copies, redrawn until every row is inside the band."
    n = len(anchors)
    gt = np.zeros_like(anchors)
    todo = np.arange(n)
    while len(todo):
        a = anchors[todo].astype(np.float64)
        aw, ah = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
        cx = (a[:, 0] + a[:, 2]) / 2 + rng.uniform(-0.3, 0.3, len(todo)) * aw
        cy = (a[:, 1] + a[:, 3]) / 2 + rng.uniform(-0.3, 0.3, len(todo)) * ah
        w, h = aw * np.exp(rng.uniform(-0.6, 0.6, len(todo))), ah * np.exp(rng.uniform(-0.6, 0.6, len(todo)))
        g = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(np.float32)
        iou = iou_rows(anchors[todo], g)
        ok = (iou >= lo) & (iou <= hi)
        gt[todo[ok]] = g[ok]
        todo = todo[~ok]
    return gt


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def test_restatement_standard_against_float64():
    "2 000 random rows, reg_w = (10, 10, 5, 5); a tenth of the size deltas above the clip, so both sides of step 4 run."
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.box_utils import decode_boxes_reference
    rng = np.random.default_rng(2901)
    a = random_anchors(rng, 2000)
    d = (rng.standard_normal((2000, 4)) * np.array([3.0, 3.0, 2.5, 2.5])).astype(np.float32)
    d[::10, 2:] = rng.uniform(20.0, 60.0, (200, 2)).astype(np.float32)                      # t2, t3 in 4 .. 12: across CLIP = 4.135
    got = decode_boxes_reference(d, a, REG_W, "standard")
    assert got.dtype == np.float32 and got.shape == (2000, 4)
    want = rule_f64(d, a, REG_W, float(np.float32(ops.BOX_XFORM_CLIP)))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
    assert (d[:, 2] / 5.0 > ops.BOX_XFORM_CLIP).sum() >= 150 and (d[:, 2] / 5.0 < ops.BOX_XFORM_CLIP).sum() >= 1500
    # torch in, torch out, the same numbers; [B, A, 4] deltas broadcast over [A, 4] anchors
    t = decode_boxes_reference(torch.from_numpy(d), torch.from_numpy(a), REG_W, "standard")
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float32 and np.array_equal(t.numpy(), got)
    both = decode_boxes_reference(np.stack([d, d[::-1]]), a, REG_W, "standard")
    assert np.array_equal(both[0], got) and both.shape == (2, 2000, 4)


def test_restatement_reference_kind_and_equal_bits_rows():
    """The reference kind of the restatement is Q4 (sizes from exp(dx), exp(dy)); a row with d2 == d0, d3 == d1, equal weights and
    t <= CLIP gives the same bits under both kinds."""
    from pytorch_retinanet_amd.box_utils import decode_boxes_reference
    rng = np.random.default_rng(2902)
    a = random_anchors(rng, 500)
    d = (rng.standard_normal((500, 4)) * 0.5).astype(np.float32)
    ref = decode_boxes_reference(d, a, (2.0, 3.0, 2.0, 3.0), "reference")
    d64, a64 = d.astype(np.float64), a.astype(np.float64)
    t0, t1 = d64[:, 0] / 2.0, d64[:, 1] / 3.0
    aw, ah = a64[:, 2] - a64[:, 0], a64[:, 3] - a64[:, 1]
    cx, cy = aw * t0 + (a64[:, 0] + a64[:, 2]) / 2, ah * t1 + (a64[:, 1] + a64[:, 3]) / 2
    w, h = aw * np.exp(t0), ah * np.exp(t1)
    np.testing.assert_allclose(ref, np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1), rtol=RTOL, atol=ATOL)
    tied = d.copy()
    tied[:, 2:] = tied[:, :2]
    assert np.array_equal(decode_boxes_reference(tied, a, (2.0, 3.0, 2.0, 3.0), "standard"),
                          decode_boxes_reference(tied, a, (2.0, 3.0, 2.0, 3.0), "reference"))
    assert not np.array_equal(decode_boxes_reference(d, a, (2.0, 3.0, 2.0, 3.0), "standard"), ref)


def test_restatement_edge_cases_and_image_clip():
    "The three edge cases of the header, and the clip to the image: all of them end with a side below min_box or a NaN."
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.box_utils import decode_boxes_reference
    an = np.array([[10.0, 20.0, 50.0, 100.0]] * 6, np.float32)
    clip = np.float32(ops.BOX_XFORM_CLIP)
    d = np.zeros((6, 4), np.float32)
    d[0, 2] = np.nan
    d[1, 2] = -np.inf
    d[2, 0] = np.inf
    d[3, 2] = clip
    d[4, 2] = np.inf
    d[5, 2] = np.nextafter(clip, np.float32(-np.inf))
    out = decode_boxes_reference(d, an, (1.0, 1.0, 1.0, 1.0), "standard", image_hw=(120, 200))
    assert np.isnan(out[0, 0]) and np.isnan(out[0, 2]) and not (out[0, 2] - out[0, 0] >= 1e-2)       # a NaN box fails `>= min_box`
    assert out[1, 0] == out[1, 2] == 30.0                                                           # dw = -inf: width 0
    assert out[2, 0] == out[2, 2] == 200.0                                                          # centre +inf: both corners on one edge
    raw = decode_boxes_reference(d, an, (1.0, 1.0, 1.0, 1.0), "standard")
    assert np.array_equal(raw[3], raw[4]) and raw[5, 2] - raw[5, 0] < raw[3, 2] - raw[3, 0]          # the clip binds above CLIP only
    assert raw[3, 2] - raw[3, 0] <= 62.5 * 40.0 * (1 + 1e-6)
    per_image = decode_boxes_reference(np.stack([d, d]), an, (1.0, 1.0, 1.0, 1.0), "standard", image_hw=[(120, 200), (60, 45)])
    assert np.array_equal(per_image[0], out, equal_nan=True) and np.nanmax(per_image[1][:, [0, 2]]) <= 45.0 and np.nanmax(per_image[1][:, [1, 3]]) <= 60.0


# ---- the point of the feature ------------------------------------------------------------------------------------------------------
def test_standard_decode_inverts_the_training_targets_and_the_reference_decode_does_not():
    """deltas = bbox_2_activ(gt, anchors) * reg_w: what a perfectly trained head outputs.  The standard decode returns gt within
    the K4 bar; the reference decode, which takes the sizes from the centre deltas, misses it by more than 1 px on most rows (checked
    for this seed: 1 999 of the 2 000 rows, median miss 54.5 px; 90 % is asserted)."""
    from pytorch_retinanet_amd.box_utils import bbox_2_activ, decode_boxes_reference
    rng = np.random.default_rng(2903)
    a = random_anchors(rng, 2000)
    gt = gt_near(rng, a)
    iou = iou_rows(a, gt)
    assert iou.min() >= 0.3 and iou.max() <= 0.9
    # bbox_2_activ multiplies by config.BBOX_REG_WEIGHTS (all ones); the test's weights go on top
    d = (bbox_2_activ(torch.from_numpy(gt), torch.from_numpy(a)) * torch.tensor(REG_W)).numpy()
    std = decode_boxes_reference(d, a, REG_W, "standard")
    np.testing.assert_allclose(std, gt, rtol=RTOL, atol=ATOL)
    ref = decode_boxes_reference(d, a, REG_W, "reference")
    miss = np.abs(ref - gt).max(1) > 1.0
    print(f"reference decode misses gt by > 1 px on {miss.mean():.4f} of the rows (median miss {np.median(np.abs(ref - gt).max(1)):.1f} px)")
    assert miss.mean() >= 0.9


# ---- names ---------------------------------------------------------------------------------------------------------------------------
def _net(**kw):
    import pytorch_retinanet_amd as P
    return P.Retinanet(num_classes=5, backbone_kind="resnet18", pretrained=False, min_size=128, max_size=160, **kw)


def test_unknown_names_raise_at_every_layer():
    from pytorch_retinanet_amd import box_utils, ops
    assert ops.BOX_DECODES == ("reference", "standard")
    d, a = torch.zeros(1, 4, 4), torch.zeros(4, 4)
    c = torch.zeros(1, 4, 2)
    for bad in ("Standard", "torchvision", "", None, 1):
        with pytest.raises(ValueError, match="decode"):
            ops.decode_clip(d, a, None, decode=bad)
        with pytest.raises(ValueError, match="decode"):
            ops.detect(c, d, a, [(8, 8)], 0.05, 0.01, 0.5, 3, decode=bad)
        with pytest.raises(ValueError, match="decode"):
            ops.detect_levels([c], [d], a, [(8, 8)], 0.05, 0.01, 0.5, 3, decode=bad)
        with pytest.raises(ValueError, match="decode"):
            ops.detect_levels([c], [d], a, None, 0.05, 0.01, 0.5, 3, padded=True, decode=bad)
        with pytest.raises(ValueError, match="decode"):
            box_utils.activ_2_bbox(d[0], a, decode=bad)
        with pytest.raises(ValueError, match="decode"):
            box_utils.decode_boxes_reference(d[0], a, (1, 1, 1, 1), bad)
    for bad in ("Standard", "torchvision", "", 1):
        with pytest.raises(ValueError, match="box_decode"):
            _net(box_decode=bad)
    # a known name passes the name check and reaches the device check (there is no CPU path)
    for good in ops.BOX_DECODES:
        with pytest.raises(Exception) as e:
            ops.decode_clip(d, a, None, decode=good)
        assert "decode must be" not in str(e.value)


def test_new_entry_points_are_declared_bound_and_check_their_arguments():
    "Header <-> ``_lib.SIGNATURES`` for the two new symbols, the two kind macros, and the argument checks that need no GPU."
    import ctypes as C
    from pytorch_retinanet_amd import _lib
    header = open(os.path.join(ROOT, "include", "retinanet_hip.h")).read()
    assert re.search(r"#define\s+RN_BOX_DECODE_REFERENCE\s+0\b", header) and re.search(r"#define\s+RN_BOX_DECODE_STANDARD\s+1\b", header)
    assert len(re.findall(r"#define\s+RN_BOX_XFORM_CLIP\b", header)) == 1                     # reused, not redefined
    for name, old in (("rn_decode_clip_kind", "rn_decode_clip"), ("rn_detect_levels_kind", "rn_detect_levels")):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
        assert decl, name
        args = [x.strip() for x in decl.group(1).split(",") if x.strip()]
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
        assert len(args) == len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[old][1]) + 1, name
        assert sum(x == "int decode" for x in args) == 1
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    # rn_decode_clip_kind: the kind and the weights are refused before anything is launched (fake, aligned addresses: never read)
    fn = _lib.lib.rn_decode_clip_kind
    p = C.c_void_p(4096)
    rw = lambda *v: (C.c_float * 4)(*v)
    call = lambda w, kind: fn(p, _lib.RN_F32, 1, 4, p, 0, None, w, kind, p, None)
    assert call(rw(1, 1, 1, 1), 2) == -1 and call(rw(1, 1, 1, 1), -1) == -1                    # RN_EINVAL: an unknown kind
    for bad in (rw(1, 1, 0, 1), rw(1, 1, 1, -5), rw(float("inf"), 1, 1, 1), rw(1, float("nan"), 1, 1)):
        assert call(bad, 1) == -1                                                          # standard: every weight finite and > 0
    params = _lib.RnDetectParams(0.05, 0.01, 0.5, 3, rw(1, 1, 0, 1))
    ptrs = (C.c_void_p * 1)(4096)
    det = lambda kind: _lib.lib.rn_detect_levels_kind(ptrs, ptrs, (C.c_int64 * 1)(4), 1, _lib.RN_F32, 1, 2, p, 0, None, C.byref(params),
                                                      kind, 8, p, p, p, p, p, p, 1 << 20, None)
    assert det(1) == -1 and det(7) == -1


def test_model_attribute_default_and_hparams_route():
    import pytorch_retinanet_amd as P
    assert _net().box_decode == "reference" and _net(box_decode=None).box_decode == "reference"
    assert _net(box_decode="reference").box_decode == "reference" and _net(box_decode="standard").box_decode == "standard"
    conf = P.load_hparams()
    assert "box_decode" not in conf.model                                                  # the shipped file keeps the default
    conf.model.update(backbone_kind="resnet18", pretrained=False, num_classes=5, min_size=128, max_size=160, box_decode="standard")
    model = P.RetinaNetModel(conf)
    assert model.net.box_decode == "standard"
    text = open(os.path.join(ROOT, "pytorch_retinanet_amd", "hparams.yaml")).read().splitlines()
    at = [i for i, line in enumerate(text) if re.match(r"#\s*box_decode:\s*standard\b", line)]
    assert len(at) == 1 and any("box_loss" in text[j] for j in (at[0] - 1, at[0] - 2))       # beside box_loss


@pytest.mark.parametrize("box_loss,box_decode,warns", [("giou", None, True), ("diou", "reference", True), ("giou", "standard", False),
                                                       ("diou", "standard", False), (None, None, False), ("smooth_l1", "reference", False),
                                                       ("smooth_l1", "standard", False)])
def test_warning_for_an_iou_loss_with_the_reference_decode(caplog, box_loss, box_decode, warns):
    with caplog.at_level(logging.WARNING):
        net = _net(box_loss=box_loss, box_decode=box_decode)
    hits = [r for r in caplog.records if r.levelno == logging.WARNING and 'box_decode="standard"' in r.getMessage()]
    assert len(hits) == (1 if warns else 0), [r.getMessage() for r in caplog.records]
    assert net.box_decode == (box_decode or "reference")                                  # nothing else changes for such a model


class _FakeCuda:
    "A stand-in for a CUDA image: the key arithmetic reads shape, dtype and device only (tests/test_captured_predict.py)."
    def __init__(self, h, w):
        self.shape = torch.Size((3, h, w))
        self.dtype, self.is_cuda, self.device = torch.float32, True, torch.device("cuda", 0)

    def dim(self):
        return len(self.shape)


def test_captured_predict_key_holds_the_decode(monkeypatch):
    from pytorch_retinanet_amd import graph
    from pytorch_retinanet_amd.graph import CapturedPredict
    monkeypatch.setattr(graph, "Tensor", _FakeCuda)
    net = _net().eval()
    p = CapturedPredict(net, [(128, 160)])
    a = [_FakeCuda(120, 150), _FakeCuda(100, 125)]
    ca = p._class_of(a)
    k = p._key(a, ca, None)
    assert "reference" in k
    net.box_decode = "standard"
    k2 = p._key(a, ca, None)
    assert k2 != k and "standard" in k2 and len(k2) == len(k)
    assert [x for x, y in zip(k, k2) if x != y] == ["reference"]                          # nothing else moved
    net.box_decode = "reference"
    assert p._key(a, ca, None) == k
    assert k.index("reference") == k.index(net.nms_thres) + 1                             # next to score_thres and nms_thres
