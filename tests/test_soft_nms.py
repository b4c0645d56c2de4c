"""CPU: Soft-NMS (``nms="soft_linear" | "soft_gaussian"``) -- the numpy restatement ``box_utils.soft_nms_reference`` on cases worked out
by hand from the numbered rule next to K6 in include/retinanet_hip.h, and the names at every layer: the header, ``_lib``, ops, the
model, the hparams and the key of ``graph.CapturedPredict``.  (The kernels, the chain and whole predicts are in
``tests/test_soft_nms_gpu.py``.)

Every expected score below is written as the rule's own fp32 operations on the inputs, so the comparisons are on bits."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
METHODS = ("soft_linear", "soft_gaussian")


def ref(boxes, scores, thr, method, **kw):
    from pytorch_retinanet_amd import box_utils
    keep, sc = box_utils.soft_nms_reference(np.asarray(boxes, F), np.asarray(scores, F), thr, method, **kw)
    assert keep.dtype == np.int64 and sc.dtype == np.float32 and keep.shape == sc.shape
    return keep.tolist(), sc


def bits(x):
    return np.asarray(x, F).view(np.uint32).tolist()


def gauss(iou, sigma=0.5):
    "The Gaussian weight of the rule for an fp32 IoU."
    return F(math.exp(-(float(iou) * float(iou)) / float(F(sigma))))


# b0 is 10 x 10; b1 is its lower half (IoU 50 / (150 - 50) = 0.5); b2 overlaps b0's upper half (IoU 50 / (200 - 50) = 1/3) and only
# touches b1 (IoU 0)
THREE = [[0, 0, 10, 10], [0, 0, 10, 5], [0, 5, 10, 15]]
IOU_01, IOU_02 = F(50) / F(100), F(50) / F(150)


def test_three_boxes_linear():
    keep, sc = ref(THREE, [0.9, 0.8, 0.7], 0.4, "soft_linear")
    # pick 0; b1 (0.5 > 0.4) -> 0.8 * (1 - 0.5) = 0.4, b2 (1/3 is not > 0.4) stays 0.7; pick 2 (disjoint from 1); pick 1
    assert keep == [0, 2, 1]
    assert bits(sc) == bits([F(0.9), F(0.7), F(0.8) * (F(1) - IOU_01)])
    # a threshold below both IoUs decays both: 0.8 * 0.5 = 0.4 < 0.7 * (1 - 1/3) = 0.4667
    keep, sc = ref(THREE, [0.9, 0.8, 0.7], 0.3, "soft_linear")
    assert keep == [0, 2, 1]
    assert bits(sc) == bits([F(0.9), F(0.7) * (F(1) - IOU_02), F(0.8) * (F(1) - IOU_01)])


def test_three_boxes_gaussian():
    keep, sc = ref(THREE, [0.9, 0.8, 0.7], 0.4, "soft_gaussian", sigma=0.5)
    # no threshold: b1 -> 0.8 exp(-0.25 / 0.5) = 0.4852, b2 -> 0.7 exp(-(1/9) / 0.5) = 0.5605; pick 2, which leaves 1 alone (IoU 0)
    assert keep == [0, 2, 1]
    assert bits(sc) == bits([F(0.9), F(0.7) * gauss(IOU_02), F(0.8) * gauss(IOU_01)])
    assert abs(float(sc[1]) - 0.7 * math.exp(-2 / 9)) < 1e-6 and abs(float(sc[2]) - 0.8 * math.exp(-0.5)) < 1e-6
    # a wider sigma decays less, and the order of the last two flips: 0.8 exp(-0.25 / 2) = 0.706 > 0.7 exp(-(1/9) / 2) = 0.662
    keep, sc = ref(THREE, [0.9, 0.8, 0.7], 0.4, "soft_gaussian", sigma=2.0)
    assert keep == [0, 1, 2]
    assert bits(sc) == bits([F(0.9), F(0.8) * gauss(IOU_01, 2.0), F(0.7) * gauss(IOU_02, 2.0)])


def test_a_score_under_min_score_ends_the_segment():
    same = [[0, 0, 10, 10], [0, 0, 10, 10], [50, 50, 60, 60]]
    # the copy decays to 0.005 exp(-1 / 0.5) = 0.00068: under 1e-3, so it is never emitted; the far box (0.0005) never was above it
    keep, sc = ref(same, [0.9, 0.005, 0.0005], 0.5, "soft_gaussian")
    assert keep == [0] and bits(sc) == bits([F(0.9)])
    # with a lower floor the copy comes out with its decayed score, then the far box
    keep, sc = ref(same, [0.9, 0.005, 0.0005], 0.5, "soft_gaussian", min_score=1e-4)
    assert keep == [0, 1, 2] and bits(sc) == bits([F(0.9), F(0.005) * gauss(F(1)), F(0.0005)])
    # linear, IoU 1: the copy's score becomes 0.8 * (1 - 1) = 0, which is not > min_score
    keep, sc = ref(same, [0.9, 0.8, 0.7], 0.5, "soft_linear")
    assert keep == [0, 2] and bits(sc) == bits([F(0.9), F(0.7)])
    # the comparison is strict: a score equal to min_score is not emitted
    keep, _ = ref(same[2:], [0.25], 0.5, "soft_linear", min_score=0.25)
    assert keep == []
    assert ref(np.zeros((0, 4)), np.zeros((0,)), 0.5, "soft_linear")[0] == []


@pytest.mark.parametrize("method", METHODS)
def test_max_keep(method):
    far = [[20 * i, 0, 20 * i + 10, 10] for i in range(5)]
    scores = [0.3, 0.9, 0.5, 0.7, 0.1]
    for cap, want in ((2, [1, 3]), (1, [1]), (5, [1, 3, 2, 0, 4]), (9, [1, 3, 2, 0, 4]), (None, [1, 3, 2, 0, 4]), (0, [1, 3, 2, 0, 4])):
        keep, sc = ref(far, scores, 0.5, method, max_keep=cap)
        assert keep == want and bits(sc) == bits([scores[i] for i in want])


@pytest.mark.parametrize("method", METHODS)
def test_zero_iou_and_zero_area_pairs_leave_scores_alone(method):
    # touching edges (inter 0 -> IoU 0), far apart, and two copies of a zero-area box (0 / 0: NaN is not > 0)
    boxes = [[0, 0, 10, 10], [10, 0, 20, 10], [100, 100, 110, 110], [5, 5, 5, 5], [5, 5, 5, 5]]
    scores = [0.9, 0.8, 0.7, 0.6, 0.5]
    keep, sc = ref(boxes, scores, 0.0, method)
    assert keep == [0, 1, 2, 3, 4] and bits(sc) == bits(scores)


def test_equal_decayed_scores_come_out_lower_index_first():
    hit, miss = [0, 0, 10, 5], [50, 50, 60, 60]                     # IoU 0.5 with the first box / disjoint from everything
    half = F(0.8) * (F(1) - IOU_01)
    assert bits(half) == bits(F(0.4))                                 # the decayed 0.8 IS the other entry's 0.4, bit for bit
    for boxes, scores in (([THREE[0], miss, hit], [0.9, 0.4, 0.8]), ([THREE[0], hit, miss], [0.9, 0.8, 0.4])):
        keep, sc = ref(boxes, scores, 0.4, "soft_linear")
        assert keep == [0, 1, 2] and bits(sc) == bits([F(0.9), F(0.4), F(0.4)])
    # duplicates of box AND score: the lower index is picked, and then decays its twin
    keep, sc = ref([hit, miss, hit], [0.8, 0.9, 0.8], 0.4, "soft_gaussian")
    assert keep == [1, 0, 2] and bits(sc) == bits([F(0.9), F(0.8), F(0.8) * gauss(F(1))])


def test_linear_with_a_threshold_of_one_keeps_everything_with_its_scores():
    rng = np.random.default_rng(3)
    c = rng.uniform(0, 30, (40, 2))
    wh = rng.uniform(10, 40, (40, 2))
    boxes = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(F)
    boxes[7] = boxes[3]                                               # an exact copy: IoU 1 is not > 1
    scores = rng.uniform(0.05, 1.0, 40).astype(F)
    scores[11] = scores[5]
    for thr in (1.0, 1.5):
        keep, sc = ref(boxes, scores, thr, "soft_linear")
        want = sorted(range(40), key=lambda i: (-float(scores[i]), i))
        assert keep == want and bits(sc) == bits(scores[want])
    keep, sc = ref(boxes, scores, 0.3, "soft_linear")                 # (and below one the same boxes do decay)
    assert len(set(keep)) == len(keep) and np.all(np.diff(sc) <= 0) and np.all(sc <= scores[keep]) and np.any(sc < scores[keep])
    assert (3 in keep) != (7 in keep)                                 # the later of the two copies went to 0 * its score


def test_emitted_scores_never_increase_and_unknown_methods_raise():
    from pytorch_retinanet_amd import box_utils
    rng = np.random.default_rng(5)
    c = rng.uniform(0, 20, (60, 2))
    boxes = np.concatenate([c - 8, c + 8], 1).astype(F)
    scores = rng.uniform(0.05, 1.0, 60).astype(F)
    for method in METHODS:
        keep, sc = ref(boxes, scores, 0.5, method)
        assert len(set(keep)) == len(keep) and np.all(np.diff(sc) <= 0) and np.all(sc > F(1e-3)) and np.all(sc <= scores[keep])
    for bad in ("hard", "gaussian", "", None):
        with pytest.raises(ValueError, match="method"):
            box_utils.soft_nms_reference(boxes, scores, 0.5, bad)


# ---- the host side ------------------------------------------------------------------------------------------------------------------
def _net(**kw):
    import pytorch_retinanet_amd as P
    return P.Retinanet(num_classes=5, backbone_kind="resnet18", pretrained=False, min_size=128, max_size=160, **kw)


def test_header_and_binding_carry_the_new_symbols():
    from pytorch_retinanet_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "retinanet_hip.h")).read()
    assert re.search(r"#define\s+RN_ABI_VERSION\s+10\b", header) and _lib.lib.rn_version() == 10
    for name, value in (("RN_NMS_HARD", 0), ("RN_NMS_SOFT_LINEAR", 1), ("RN_NMS_SOFT_GAUSSIAN", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), name
    assert ops.NMS_KINDS == ("hard", "soft_linear", "soft_gaussian")
    st = re.search(r"typedef\s+struct\s+rn_nms_params\s*\{(.*?)\}\s*rn_nms_params\s*;", header, re.S)
    assert st
    body = re.sub(r"/\*.*?\*/", "", st.group(1), flags=re.S)
    assert re.sub(r"\s+", " ", body).strip() == "int32_t method; float sigma, min_score; int32_t max_keep;"
    assert [f[0] for f in _lib.RnNmsParams._fields_] == ["method", "sigma", "min_score", "max_keep"]
    assert C.sizeof(_lib.RnNmsParams) == 16
    # rn_detect_params did not move
    assert re.search(r"typedef struct rn_detect_params \{\s*float score_thr, min_box, nms_thr;\s*int32_t max_det;\s*float reg_w\[4\];\s*\} rn_detect_params;", header)
    for name, old, extra in (("rn_soft_nms_segments", "rn_nms_segments", 2), ("rn_detect_levels_nms", "rn_detect_levels_kind", 1)):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
        assert decl, name
        args = [x.strip() for x in decl.group(1).split(",") if x.strip()]
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
        assert len(args) == len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[old][1]) + extra, name
        assert sum(x == "const rn_nms_params *nms" for x in args) == 1
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]


def test_bad_nms_params_are_refused_before_anything_is_launched():
    "Fake, aligned addresses: a refused call never reads them."
    from pytorch_retinanet_amd import _lib
    p = C.c_void_p(4096)
    inf, nan = float("inf"), float("nan")
    bad = [(3, 0.5, 1e-3), (-1, 0.5, 1e-3), (2, 0.0, 1e-3), (2, -1.0, 1e-3), (2, inf, 1e-3), (2, nan, 1e-3), (2, 0.5, inf), (2, 0.5, nan),
           (1, 0.5, nan), (1, 0.5, -inf)]
    for method, sigma, floor in bad:
        q = _lib.RnNmsParams(method, sigma, floor, 0)
        assert _lib.lib.rn_soft_nms_segments(p, p, p, 1, 4, 0.5, C.byref(q), p, p, p, p, 1 << 20, None) == -1, (method, sigma, floor)
    assert _lib.lib.rn_soft_nms_segments(p, p, p, 1, 4, 0.5, C.byref(_lib.RnNmsParams(0, 0.5, 1e-3, 0)), p, p, p, p, 1 << 20, None) == -1
    assert _lib.lib.rn_soft_nms_segments(p, p, p, 1, 4, 0.5, None, p, p, p, p, 1 << 20, None) == -1
    # a valid soft kind gets past the parameter check (to the workspace check: still nothing launched)
    assert _lib.lib.rn_soft_nms_segments(p, p, p, 1, 4, 0.5, C.byref(_lib.RnNmsParams(1, nan, 1e-3, 0)), p, p, p, p, 0, None) == -3
    params = _lib.RnDetectParams(0.05, 0.01, 0.5, 3, (C.c_float * 4)(1, 1, 1, 1))
    ptrs = (C.c_void_p * 1)(4096)
    for method, sigma, floor in bad:
        q = _lib.RnNmsParams(method, sigma, floor, 0)
        rc = _lib.lib.rn_detect_levels_nms(ptrs, ptrs, (C.c_int64 * 1)(4), 1, _lib.RN_F32, 1, 2, p, 0, None, C.byref(params), 0, C.byref(q),
                                           8, p, p, p, p, p, p, 1 << 20, None)
        assert rc == -1, (method, sigma, floor)


def test_unknown_kinds_raise_at_every_layer():
    from pytorch_retinanet_amd import ops
    d, a, c = torch.zeros(1, 4, 4), torch.zeros(4, 4), torch.zeros(1, 4, 2)
    off = torch.tensor([0, 4], dtype=torch.int32)
    for bad in ("bogus", "Hard", "soft", "", None, 1):
        with pytest.raises(ValueError, match="nms"):
            ops.detect(c, d, a, [(8, 8)], 0.05, 0.01, 0.5, 3, nms=bad)
        with pytest.raises(ValueError, match="nms"):
            ops.detect_levels([c], [d], a, [(8, 8)], 0.05, 0.01, 0.5, 3, nms=bad)
        with pytest.raises(ValueError, match="nms"):
            ops.detect_levels([c], [d], a, None, 0.05, 0.01, 0.5, 3, padded=True, nms=bad)
        with pytest.raises(ValueError):
            ops.soft_nms_segments(a, torch.zeros(4), off, 0.5, bad)
    with pytest.raises(ValueError, match="nms_segments"):
        ops.soft_nms_segments(a, torch.zeros(4), off, 0.5, "hard")
    for bad in ("bogus", "Hard", "soft", "", 1):
        with pytest.raises(ValueError, match="nms"):
            _net(nms=bad)
    for good in ops.NMS_KINDS:                                         # a known name reaches the device check (there is no CPU path)
        with pytest.raises(Exception) as e:
            ops.detect(c, d, a, [(8, 8)], 0.05, 0.01, 0.5, 3, nms=good)
        assert "nms must be" not in str(e.value)


def test_model_attributes_defaults_and_hparams_route():
    import pytorch_retinanet_amd as P
    net = _net()
    assert (net.nms, net.soft_nms_sigma, net.soft_nms_min_score) == ("hard", 0.5, 1e-3)
    assert _net(nms=None).nms == "hard" and _net(nms="hard").nms == "hard"
    net = _net(nms="soft_linear", soft_nms_sigma=0.25, soft_nms_min_score=0.01)
    assert (net.nms, net.soft_nms_sigma, net.soft_nms_min_score) == ("soft_linear", 0.25, 0.01)
    assert net._nms_args() == {"nms": "soft_linear", "nms_sigma": 0.25, "nms_min_score": 0.01}
    net.nms = "soft_gaussian"                                          # read at every call
    assert net._nms_args()["nms"] == "soft_gaussian"
    conf = P.load_hparams()
    assert "nms" not in conf.model                                     # the shipped file keeps the default
    conf.model.update(backbone_kind="resnet18", pretrained=False, num_classes=5, min_size=128, max_size=160, nms="soft_gaussian")
    assert P.RetinaNetModel(conf).net.nms == "soft_gaussian"
    text = open(os.path.join(ROOT, "pytorch_retinanet_amd", "hparams.yaml")).read().splitlines()
    assert sum(bool(re.match(r"#\s*nms:\s*soft_gaussian\b", line)) for line in text) == 1


class _FakeCuda:
    "A stand-in for a CUDA image: the key arithmetic reads shape, dtype and device only (tests/test_captured_predict.py)."
    def __init__(self, h, w):
        self.shape = torch.Size((3, h, w))
        self.dtype, self.is_cuda, self.device = torch.float32, True, torch.device("cuda", 0)

    def dim(self):
        return len(self.shape)


def test_captured_predict_key_holds_the_nms_kind_and_its_constants(monkeypatch):
    from pytorch_retinanet_amd import graph
    from pytorch_retinanet_amd.graph import CapturedPredict
    monkeypatch.setattr(graph, "Tensor", _FakeCuda)
    net = _net().eval()
    p = CapturedPredict(net, [(128, 160)])
    a = [_FakeCuda(120, 150), _FakeCuda(100, 125)]
    ca = p._class_of(a)
    k = p._key(a, ca, None)
    at = k.index("hard")
    assert k[at - 1] == "reference" and k[at:at + 3] == ("hard", 0.5, 1e-3)      # behind the box decode
    keys = {k}
    for kind in ("soft_linear", "soft_gaussian"):
        net.nms = kind
        k2 = p._key(a, ca, None)
        assert len(k2) == len(k) and [(x, y) for x, y in zip(k, k2) if x != y] == [("hard", kind)]
        keys.add(k2)
    assert len(keys) == 3
    net.soft_nms_sigma = 0.3
    k3 = p._key(a, ca, None)
    assert [(x, y) for x, y in zip(k2, k3) if x != y] == [(0.5, 0.3)]
    net.soft_nms_min_score = 0.01
    assert [(x, y) for x, y in zip(k3, p._key(a, ca, None)) if x != y] == [(1e-3, 0.01)]
    net.nms, net.soft_nms_sigma, net.soft_nms_min_score = "hard", 0.5, 1e-3
    assert p._key(a, ca, None) == k
    for name in ("nms", "soft_nms_sigma", "soft_nms_min_score"):      # a model object from before the attributes existed
        delattr(net, name)
    assert p._key(a, ca, None) == k
