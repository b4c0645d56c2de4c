"""CPU: the host side of graph-replayed inference (``graph.CapturedPredict``) -- the numpy restatement of ``rn_detect_finish_var``
against ``transform.postprocess``, the result block's layout against ``rn_detect_result_bytes``, the key and class selection, the
argument checks that need no GPU, and the ``predictor`` / ``predict_image_capacity`` wiring.  (The kernel, the staged eval path and
whole captured calls are in ``tests/test_captured_predict_gpu.py``.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def _transform(min_size, max_size):
    from pytorch_retinanet_amd.transform import GeneralizedRCNNTransform
    return GeneralizedRCNNTransform(min_size, max_size, MEAN, STD)


def _padded(B, max_det, counts, seed=0):
    rng = np.random.default_rng(seed)
    boxes = (rng.random((B, max_det, 4), dtype=np.float32) * np.float32(333.0)).astype(np.float32)
    scores = rng.random((B, max_det), dtype=np.float32)
    labels = rng.integers(1, 91, (B, max_det)).astype(np.int64)
    return boxes, scores, labels, np.asarray(counts, np.int32)


# ---- the restatement and the block ----------------------------------------------------------------------------------------------
def test_finish_restatement_equals_postprocess_bit_for_bit():
    "Identity and non-identity ratios mixed: rows below the count are ``resize_boxes``' (early return included), the rest zero."
    from pytorch_retinanet_amd import ops
    in_hw = [(120, 150), (128, 160), (140, 128), (333, 500), (128, 97)]
    out_hw = [(128, 160), (128, 160), (160, 146), (106, 160), (128, 97)]                 # images 1 and 4: ratio exactly 1
    B, max_det = len(in_hw), 9
    counts = [9, 4, 0, 1, 7]
    boxes, scores, labels, count = _padded(B, max_det, counts)
    status = np.array([0, 1, 0, 0, 2], np.int32)
    block = ops.detect_finish_reference(boxes, scores, labels, count, status, in_hw, out_hw)
    assert block.dtype == np.uint8 and block.size == ops.detect_result_layout(B, max_det)["total"]
    tr = _transform(128, 160).eval()
    dets = [{"boxes": torch.from_numpy(boxes[b, :n].copy()), "scores": torch.from_numpy(scores[b, :n].copy()),
             "labels": torch.from_numpy(labels[b, :n].copy())} for b, n in enumerate(counts)]
    want = tr.postprocess(dets, out_hw, in_hw)
    got = ops.detect_result_dicts(torch.from_numpy(block), B, max_det)
    changed = 0
    for b, (g, w) in enumerate(zip(got, want)):
        assert g["boxes"].shape == (counts[b], 4) and g["labels"].dtype == torch.int64
        for k in ("boxes", "scores", "labels"):
            assert g[k].numpy().tobytes() == w[k].numpy().tobytes(), (b, k)
        changed += int(counts[b] > 0 and not np.array_equal(g["boxes"].numpy(), boxes[b, :counts[b]]))
    assert changed == 2                                                                  # images 0 and 3 moved, 1 and 4 did not
    v = ops.detect_result_views(torch.from_numpy(block), B, max_det)
    assert v["counts"].tolist() == counts and v["status"].tolist() == [0, 1, 0, 0, 2]
    for b, n in enumerate(counts):                                                       # rows past the count: zero
        assert not v["boxes"][b, n:].any() and not v["scores"][b, n:].any() and not v["labels"][b, n:].any()


@pytest.mark.parametrize("B,max_det", [(1, 1), (1, 2), (2, 1), (3, 100), (5, 7), (65, 3), (64, 300)])
def test_block_layout_matches_the_library_and_the_header(B, max_det):
    from pytorch_retinanet_amd import _lib, ops
    lay = ops.detect_result_layout(B, max_det)
    rows = B * max_det
    assert lay["total"] == _lib.lib.rn_detect_result_bytes(B, max_det)
    assert lay["counts"] == 0 and lay["status"] == 4 * B
    assert all(lay[k] % 16 == 0 for k in ("boxes", "scores", "labels", "total"))
    assert lay["boxes"] >= 8 * B and lay["scores"] == lay["boxes"] + 16 * rows and lay["labels"] >= lay["scores"] + 4 * rows
    assert lay["total"] >= lay["labels"] + 8 * rows and lay["total"] - (lay["labels"] + 8 * rows) < 16
    # the block parses: every field round-trips through the views
    block = torch.zeros(lay["total"], dtype=torch.uint8)
    v = ops.detect_result_views(block, B, max_det)
    v["counts"].copy_(torch.arange(B, dtype=torch.int32) % (max_det + 1))
    v["labels"].fill_(2 ** 40 + 3)
    v["scores"].fill_(0.5)
    v["boxes"].fill_(-1.25)
    v["status"].fill_(7)
    again = ops.detect_result_views(block, B, max_det)
    assert again["counts"].tolist() == [b % (max_det + 1) for b in range(B)] and bool((again["status"] == 7).all())
    assert bool((again["labels"] == 2 ** 40 + 3).all()) and bool((again["scores"] == 0.5).all()) and bool((again["boxes"] == -1.25).all())
    dicts = ops.detect_result_dicts(block, B, max_det)
    assert [len(d["scores"]) for d in dicts] == [b % (max_det + 1) for b in range(B)]


def test_layout_and_view_argument_errors():
    from pytorch_retinanet_amd import _lib, ops
    assert _lib.lib.rn_detect_result_bytes(0, 5) == 0 and _lib.lib.rn_detect_result_bytes(5, 0) == 0 and _lib.lib.rn_detect_result_bytes(-1, 5) == 0
    with pytest.raises(ValueError, match="max_det"):
        ops.detect_result_layout(0, 5)
    with pytest.raises(ValueError, match="max_det"):
        ops.detect_result_layout(2, 0)
    total = ops.detect_result_layout(2, 3)["total"]
    with pytest.raises(ValueError, match="result block"):
        ops.detect_result_views(torch.zeros(total + 16, dtype=torch.uint8), 2, 3)
    with pytest.raises(ValueError, match="result block"):
        ops.detect_result_views(torch.zeros(total // 4, dtype=torch.float32), 2, 3)


def test_new_entry_points_are_declared_bound_and_check_their_arguments():
    "Header <-> ``_lib.SIGNATURES`` for the two new symbols, and the argument checks of the kernel's entry point that need no GPU."
    from pytorch_retinanet_amd import _lib
    header = open(os.path.join(ROOT, "include", "retinanet_hip.h")).read()
    for name in ("rn_detect_result_bytes", "rn_detect_finish_var"):
        decl = re.search(r"^(?:size_t|int) " + name + r"\s*\(([^;]*?)\)\s*;", header, re.S | re.M)
        assert decl is not None, name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
        assert len([a for a in decl.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
    assert int(re.search(r"#define\s+RN_ABI_VERSION\s+(\d+)", header).group(1)) == 10 == _lib.lib.rn_version()
    assert "finish.o" in open(os.path.join(ROOT, "pytorch_retinanet_amd", "csrc", "Makefile")).read()
    # every argument is checked before any launch: these return without touching a device (there is none here)
    fn = _lib.lib.rn_detect_finish_var
    good = [0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 2, 3, 0x8000, _lib.lib.rn_detect_result_bytes(2, 3), None]
    for i in (0, 1, 2, 3, 4, 5, 6, 9):                                                  # a null pointer
        args = list(good); args[i] = None
        assert fn(*args) == -1, i
    for i, bad in ((7, 0), (7, -1), (8, 0), (8, -5)):                                   # B, max_det
        args = list(good); args[i] = bad
        assert fn(*args) == -1, (i, bad)
    for i, bad in ((0, 0x1008), (1, 0x2002), (2, 0x3004), (3, 0x4001), (4, 0x5002), (5, 0x6003), (6, 0x7001), (9, 0x8008)):
        args = list(good); args[i] = bad
        assert fn(*args) == -2, (i, hex(bad))                                           # RN_EALIGN
    args = list(good); args[10] = good[10] - 1
    assert fn(*args) == -3                                                              # RN_EWORKSPACE: one byte short


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from pytorch_retinanet_amd import ops
    boxes, scores, labels, count = _padded(2, 3, [1, 2])
    t = [torch.from_numpy(a) for a in (boxes, scores, labels)]
    meta = torch.zeros(2, 2, dtype=torch.int32)
    hw = torch.ones(2, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.detect_finish_var(*t, meta, hw, hw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                          # (the new arguments change no refusal)
        ops.detect_levels([torch.zeros(1, 4, 2)], [torch.zeros(1, 4, 4)], torch.zeros(4, 4), None, 0.05, 0.01, 0.5, 3,
                          image_hw_dev=torch.ones(1, 2, dtype=torch.int32), padded=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.detect_levels([torch.zeros(1, 4, 2)], [torch.zeros(1, 4, 4)], torch.zeros(4, 4), [(8, 8)], 0.05, 0.01, 0.5, 3)


# ---- the eval-mode staged transform: host arithmetic ------------------------------------------------------------------------------
def test_eval_short_side_and_bounds_are_the_list_paths():
    import math
    tr = _transform((96, 112, 128), 160).eval()
    assert tr.staged_eval_short_side() == 128 and tr.staged_short_side() is None          # eval: min_size[-1], tuple or not
    assert _transform(128.5, 160).staged_eval_short_side() is None and _transform(128, 160.5).staged_eval_short_side() is None
    with pytest.raises(ValueError, match="min_size"):
        _transform(128.5, 160).staged_eval_bounds([(120, 150)])
    sizes = [(120, 150), (140, 128), (128, 160), (1, 7), (500, 333)]
    want = []
    for h, w in sizes:
        s = tr._scale_for(h, w, 128.0)
        want.append((int(math.floor(h * s)), int(math.floor(w * s))))
    assert tr.staged_eval_bounds(sizes) == want and want[2] == (128, 160)
    # the training errors stay what tests/test_image_capacity.py pins; eval without targets on a CPU arena reaches the device refusal
    from pytorch_retinanet_amd import ops
    s = ops.new_image_arena(1, 2 ** 16, torch.device("cpu"), (160, 160))
    s.hw = [(120, 150)]
    with pytest.raises(ValueError, match="packed GT"):
        _transform(128, 160)(s, None, canvas=(160, 160))                                   # training mode: still a training input
    with pytest.raises(ValueError, match="packed GT"):
        tr(s, [{"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, dtype=torch.int64)}], canvas=(160, 160))
    with pytest.raises(ValueError, match="canvas"):
        tr(s, None)
    with pytest.raises(ValueError, match="does not contain"):
        tr(s, None, canvas=(128, 128))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr(s, None, canvas=(160, 160))


# ---- CapturedPredict: arguments, class and key selection ----------------------------------------------------------------------------
def _net():
    import pytorch_retinanet_amd as P
    return P.Retinanet(num_classes=5, backbone_kind="resnet18", pretrained=False, min_size=128, max_size=160)


def test_captured_predict_argument_errors():
    from pytorch_retinanet_amd.graph import CapturedPredict
    net = _net().eval()
    for bad in (None, "big", [], [(160,)], [(160, 160), (160, 160)], [(0, 160)], [(160.0, 160)]):
        with pytest.raises(ValueError, match="image_capacity"):
            CapturedPredict(net, bad)
    with pytest.raises(ValueError, match="size_divisible"):
        CapturedPredict(net, [(150, 160)])
    with pytest.raises(ValueError, match="amp_dtype"):
        CapturedPredict(net, "auto", amp_dtype=torch.float32)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="eager_calls"):
            CapturedPredict(net, "auto", eager_calls=bad)
    with pytest.raises(ValueError, match="max_graphs"):
        CapturedPredict(net, "auto", max_graphs=0)
    for bad in (0, -3, 2.0, True):
        with pytest.raises(ValueError, match="max_candidates"):
            CapturedPredict(net, "auto", max_candidates=bad)
    p = CapturedPredict(net, "auto")
    assert p.image_capacity == ((128, 160), (160, 128), (160, 160))
    assert p.stats == {"captures": 0, "replays": 0, "eager": 0, "fallbacks": 0, "overflows": 0, "invalidations": 0}
    with pytest.raises(ValueError, match="to"):
        p([torch.rand(3, 8, 8)], to="host")
    with pytest.raises(ValueError, match="eval"):
        _net().predict_staged(None)                                                       # a net in training mode


class _FakeCuda:
    "A stand-in for a CUDA image: the class / key arithmetic reads shape, dtype and device only."
    def __init__(self, h, w, dtype=torch.float32, shape=None):
        self.shape = torch.Size(shape or (3, h, w))
        self.dtype, self.is_cuda, self.device = dtype, True, torch.device("cuda", 0)

    def dim(self):
        return len(self.shape)


def test_class_and_key_selection(monkeypatch):
    from pytorch_retinanet_amd import graph
    from pytorch_retinanet_amd.graph import CapturedPredict
    monkeypatch.setattr(graph, "Tensor", _FakeCuda)                                      # (isinstance check of the image list)
    net = _net().eval()
    p = CapturedPredict(net, [(128, 160), (160, 192)])
    a = [_FakeCuda(120, 150), _FakeCuda(100, 125)]                                        # -> 128 x 160 both: own canvas 128 x 160
    ca = p._class_of(a)
    assert ca == ((128, 160), 2 ** 16, [(128, 160), (128, 160)])
    b = [_FakeCuda(140, 128), _FakeCuda(120, 150)]                                        # -> 140 x 128, 128 x 160: own canvas 160 x 160
    cb = p._class_of(b)
    assert cb[0] == (160, 192) and cb[2] == [(140, 128), (128, 160)]
    big = [_FakeCuda(300, 300)]                                                           # 90000 pixels: the next pixel class
    assert p._class_of(big) == ((128, 160), 2 ** 17, net.transform.staged_eval_bounds([(300, 300)]))
    # what no class holds, or the fused transform does not take, goes to net.predict
    assert CapturedPredict(net, [(128, 160)])._class_of(b) is None
    assert p._class_of([]) is None and p._class_of([_FakeCuda(8, 8, torch.uint8)]) is None
    assert p._class_of([_FakeCuda(8, 8, shape=(8, 8, 3))]) is None and p._class_of([torch.rand(3, 8, 8)]) is None
    net.train()
    assert p._class_of(a) is None
    net.eval()
    net.transform.train()
    assert p._class_of(a) is None                                                          # (predict would not rescale either)
    net.eval()
    tuple_net = _net().eval()
    tuple_net.transform.min_size = (96, 128)
    assert CapturedPredict(tuple_net, [(128, 160)])._class_of(a) == ca                      # eval: min_size[-1]
    # keys: B, canvas class, pixel class, autocast dtype, memory format
    k = p._key(a, ca, None)
    assert k == p._key([_FakeCuda(64, 80), _FakeCuda(128, 160)], p._class_of([_FakeCuda(64, 80), _FakeCuda(128, 160)]), None)
    assert k != p._key(a + a[:1], p._class_of(a + a[:1]), None)
    assert k != p._key(b, cb, None) and k != p._key(a, ca, torch.bfloat16) and p._key(big, p._class_of(big), None) != p._key(b[:1], p._class_of(b[:1]), None)
    net.to(memory_format=torch.channels_last)
    assert k != p._key(a, ca, None)
    # ... and what the pass takes by value: the transform's sizes and statistics, the detect thresholds; the modules' modes as they are
    k = p._key(a, ca, None)
    assert k == p._key(a, ca, None, p._walk()[0]) and any(isinstance(v, tuple) and len(v) == len(list(net.modules())) for v in k)
    for change, undo in ((lambda: setattr(net.transform, "max_size", 192), lambda: setattr(net.transform, "max_size", 160)),
                         (lambda: setattr(net.transform, "image_mean", [0.5, 0.5, 0.5]), lambda: setattr(net.transform, "image_mean", list(MEAN))),
                         (lambda: setattr(net, "score_thres", 0.3), lambda: setattr(net, "score_thres", 0.05)),
                         (lambda: net.fpn.train(), lambda: net.fpn.eval())):
        change()
        assert k != p._key(a, ca, None)
        undo()
        assert k == p._key(a, ca, None)
    assert p.host_seconds == 0.0 and p.host_calls == 0
    # the autocast dtype of a call: the constructor's, else the caller's state
    assert p._autocast_dtype() is None
    assert CapturedPredict(net, "auto", amp_dtype=torch.float16)._autocast_dtype() is torch.float16


def test_weights_stamp_moves_with_torch_and_raw_writes():
    from pytorch_retinanet_amd.graph import CapturedPredict
    from pytorch_retinanet_amd.norm import note_raw_write
    net = _net().eval()
    p = CapturedPredict(net, "auto")
    s0 = p._weights_stamp()
    assert p._weights_stamp() == s0
    note_raw_write()
    s1 = p._weights_stamp()
    assert s1 != s0
    with torch.no_grad():
        net.backbone.backbone.bn1.running_var.mul_(1.5)                                   # a buffer, in place
    s2 = p._weights_stamp()
    assert s2 != s1
    net.load_state_dict(net.state_dict())
    assert p._weights_stamp() != s2


# ---- wiring ---------------------------------------------------------------------------------------------------------------------------
def test_predictor_defaults_to_none_and_test_step_calls_it():
    import pytorch_retinanet_amd as P
    conf = P.load_hparams()
    conf.model.update(backbone_kind="resnet18", pretrained=False, num_classes=5, min_size=128, max_size=160)
    model = P.RetinaNetModel(conf)
    assert model.predictor is None
    seen = []

    def predictor(images):
        seen.append(len(images))
        return [{"boxes": torch.zeros(0, 4), "scores": torch.zeros(0), "labels": torch.zeros(0, dtype=torch.int64)} for _ in images]
    model.predictor = predictor
    batch = ([torch.rand(3, 8, 8)] * 2, [{"image_id": torch.tensor([3])}, {"image_id": torch.tensor([4])}], [3, 4])
    out = model.test_step(batch, 0)
    assert seen == [2] and sorted(out["detections"]) == [3, 4]


def test_trainer_resolves_predict_image_capacity():
    import pytorch_retinanet_amd as P
    conf = P.load_hparams()
    t = P.SimpleTrainer(device="cpu")
    assert t.predict_image_capacity is None and t.predictor is None and t.resolve_predict_image_capacity(conf) is None
    assert t.resolve_predict_image_capacity(None) is None
    conf["trainer"] = {"predict_image_capacity": "auto"}
    assert t.resolve_predict_image_capacity(conf) == "auto"
    conf["trainer"] = {"predict_image_capacity": [[800, 1344], [1344, 800]]}
    assert t.resolve_predict_image_capacity(conf) == [(800, 1344), (1344, 800)]
    assert P.SimpleTrainer(device="cpu", predict_image_capacity=[(160, 160)]).resolve_predict_image_capacity(conf) == [(160, 160)]
    for bad in ("big", [], [(160,)], [(160, 160), (160, 160)]):
        with pytest.raises(ValueError, match="image_capacity"):
            P.SimpleTrainer(device="cpu", predict_image_capacity=bad)
    # no gt_capacity needed (there is no GT), and training's image_capacity still needs it
    with pytest.raises(ValueError, match="gt_capacity"):
        P.SimpleTrainer(device="cpu", image_capacity="auto", predict_image_capacity="auto")
    text = open(os.path.join(os.path.dirname(P.__file__), "hparams.yaml")).read()
    assert "predict_image_capacity" in text and "trainer" not in P.load_hparams()          # mentioned in a comment only
