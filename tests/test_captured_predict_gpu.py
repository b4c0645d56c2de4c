"""GPU: graph-replayed inference for batches whose image sizes vary -- ``rn_detect_finish_var`` against its numpy restatement
(``ops.detect_finish_reference``), byte for byte over the whole result block, and ``graph.CapturedPredict`` /
``Retinanet.predict_staged`` against ``Retinanet.predict``.

Bars.  The kernel: byte equality (it runs ``transform.resize_boxes``' two roundings, built without FMA contraction and with IEEE
division).  The model: the staged path runs ``predict``'s kernels on the same values over the same canvas -- the transform kernel is
tested bit-identical in ``tests/test_image_capacity_gpu.py``, the conv stack and the detect chain are the same calls -- so eager
first calls and replays are held to ``net.predict`` bit for bit WHEN ``net.predict`` repeats itself bit for bit in one process, which
the ``repeats`` fixture checks first (``test_eager_predict_repeatability_decides_the_bars``).  On the MI355X it does not: five fp32
``predict`` calls on the fixture differ from one another by up to 1.8e-4 px in the boxes and 6e-7 in the scores (equal labels and
counts; the FPN maps by 4e-5, the class logits by 7e-6), replays of ONE graph differ from each other by as much, and under bf16 that
noise flips roundings, so whole detections near the score threshold and the top-100 cut-off come and go (56 / 58 detections for
image 0).  The conv stack accumulates in an order that is not fixed from launch to launch.  Then the bars are the ``e2e.npz`` ones:
fp32 results agree like ``test_e2e_gpu.test_predict_matches_the_reference_fp32`` asks (>= 99 % box-set agreement at IoU 0.999 with
equal labels, counts within max(1, 1 %), scores within 1e-4) -- against the reference's detections and, wherever a test says
"equals ``net.predict``", against that call's result -- and bf16 results meet the bf16 bars of
``test_e2e_gpu.test_forward_and_predict_bf16_autocast`` against the reference (>= 85 % of its confident boxes found at IoU >= 0.9
with the label and the score within 5e-3, median IoU >= 0.97).  The fp32 result meets the ``e2e.npz`` bars either way.  A
random-init net detects nothing, so every test asserts non-empty results.  Model: resnet18, K = 5, min_size 128 / max_size 160 (the ``e2e.npz`` fixture: inputs 120 x 150 and
140 x 128, own canvas 160 x 160, 53 and 100 detections)."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_e2e_gpu import DEV, E2E, _inputs, _iou, _model, box_set_agreement

pytestmark = pytest.mark.gpu
GUARD = 1024                                    # bytes before and after a guarded block (a multiple of 16: the alignment is kept)
FILL = 0xA5


# ---- 1. rn_detect_finish_var --------------------------------------------------------------------------------------------------
def _finish_case(B, max_det, counts, in_hw, out_hw, status, seed=0):
    "Random padded detect outputs (garbage past every count too) -> (device inputs, the restatement's block)."
    from pytorch_retinanet_amd import ops
    rng = np.random.default_rng(seed)
    boxes = (rng.random((B, max_det, 4), dtype=np.float32) * np.float32(640.0) - np.float32(3.0)).astype(np.float32)
    scores = rng.random((B, max_det), dtype=np.float32)
    labels = rng.integers(1, 2 ** 40, (B, max_det)).astype(np.int64)
    meta = np.stack([np.asarray(counts, np.int32), np.asarray(status, np.int32)])
    want = ops.detect_finish_reference(boxes, scores, labels, meta[0], meta[1], in_hw, out_hw)
    dev = [torch.from_numpy(a).to(DEV) for a in (boxes, scores, labels, meta, np.asarray(in_hw, np.int32), np.asarray(out_hw, np.int32))]
    return dev, want


def _run_guarded(dev, B, max_det):
    "The kernel into a buffer of EXACTLY rn_detect_result_bytes between two guards -> (the block's bytes, guards intact?)."
    from pytorch_retinanet_amd import _lib, ops
    total = int(_lib.lib.rn_detect_result_bytes(B, max_det))
    buf = torch.full((GUARD + total + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    out = ops.detect_finish_var(*dev, out=buf[GUARD:GUARD + total])
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr() + GUARD
    host = buf.cpu().numpy()
    return host[GUARD:GUARD + total], bool((host[:GUARD] == FILL).all() and (host[-GUARD:] == FILL).all())


def _sizes(B, seed):
    "Original / resized sizes with identity images (ratio exactly 1) beside others."
    rng = np.random.default_rng(seed)
    in_hw = [(int(rng.integers(60, 700)), int(rng.integers(60, 700))) for _ in range(B)]
    out_hw = [(h, w) if b % 3 == 1 else (int(rng.integers(60, 200)), int(rng.integers(60, 200))) for b, (h, w) in enumerate(in_hw)]
    return in_hw, out_hw


FINISH_CASES = {
    "smallest": (1, 1, [1]),                                     # B = 1, max_det = 1
    "smallest_empty": (1, 1, [0]),
    "two_blocks": (3, 100, [100, 0, 1]),                         # 300 rows cross a 256-thread block; counts 0, 1, max_det
    "odd_rows": (3, 5, [5, 2, 0]),                               # 15 rows: every section ends off a 16-byte boundary
    "beyond_64_images": (65, 7, [b % 8 for b in range(65)]),     # no per-64-image launch table
    "clamped_counts": (4, 6, [-3, 9, 6, 2]),                     # device data: a count outside [0, max_det] reads no row it must not
}


@pytest.mark.parametrize("case", list(FINISH_CASES))
def test_finish_kernel_equals_the_restatement_byte_for_byte(case):
    B, max_det, counts = FINISH_CASES[case]
    in_hw, out_hw = _sizes(B, seed=len(case))
    status = [(b % 4 == 2) * (b + 1) for b in range(B)]          # non-zero status: passed through
    dev, want = _finish_case(B, max_det, counts, in_hw, out_hw, status, seed=B + max_det)
    got, intact = _run_guarded(dev, B, max_det)
    assert intact, "bytes outside the block were written"
    assert got.size == want.size and got.tobytes() == want.tobytes()
    # (what the block says, once: the identity images kept their boxes, the others moved, rows past the count are zero)
    from pytorch_retinanet_amd import ops
    v = ops.detect_result_views(torch.from_numpy(got.copy()), B, max_det)
    assert v["counts"].tolist() == list(counts) and v["status"].tolist() == status
    boxes = dev[0].cpu()
    for b in range(B):
        n = min(max(counts[b], 0), max_det)
        assert not v["boxes"][b, n:].any() and not v["scores"][b, n:].any() and not v["labels"][b, n:].any()
        if n and in_hw[b] == out_hw[b]:
            assert torch.equal(v["boxes"][b, :n], boxes[b, :n])
        elif n:
            assert not torch.equal(v["boxes"][b, :n], boxes[b, :n])


def test_finish_allocates_its_block_and_postprocess_agrees():
    "Without ``out=``: a fresh block of the formula's size; its dicts are ``transform.postprocess`` of the padded rows."
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.transform import GeneralizedRCNNTransform
    B, max_det, counts = 3, 4, [4, 2, 3]
    in_hw, out_hw = [(120, 150), (128, 160), (140, 128)], [(128, 160), (128, 160), (140, 128)]
    dev, want = _finish_case(B, max_det, counts, in_hw, out_hw, [0, 0, 0], seed=5)
    block = ops.detect_finish_var(*dev)
    assert block.dtype == torch.uint8 and block.numel() == ops.detect_result_layout(B, max_det)["total"]
    assert block.cpu().numpy().tobytes() == want.tobytes()
    tr = GeneralizedRCNNTransform(128, 160, [0.5] * 3, [0.25] * 3).eval()
    dets = [{"boxes": dev[0][b, :n].clone()} for b, n in enumerate(counts)]
    for g, w in zip(ops.detect_result_dicts(block, B, max_det), tr.postprocess(dets, out_hw, in_hw)):
        assert torch.equal(g["boxes"], w["boxes"])


def test_finish_rejects_bad_arguments_before_any_launch():
    from pytorch_retinanet_amd import _lib, ops
    B, max_det = 2, 3
    dev, _ = _finish_case(B, max_det, [3, 1], [(8, 8), (9, 9)], [(8, 8), (5, 5)], [0, 0])
    boxes, scores, labels, meta, in_hw, out_hw = dev
    total = ops.detect_result_layout(B, max_det)["total"]
    out = torch.full((total,), FILL, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="out_boxes"):
        ops.detect_finish_var(boxes.half(), scores, labels, meta, in_hw, out_hw, out=out)
    with pytest.raises(ValueError, match="out_scores"):
        ops.detect_finish_var(boxes, scores[:, :2], labels, meta, in_hw, out_hw, out=out)
    with pytest.raises(ValueError, match="out_labels"):
        ops.detect_finish_var(boxes, scores, labels.int(), meta, in_hw, out_hw, out=out)
    with pytest.raises(ValueError, match="meta"):
        ops.detect_finish_var(boxes, scores, labels, meta[0], in_hw, out_hw, out=out)
    with pytest.raises(ValueError, match="in_hw"):
        ops.detect_finish_var(boxes, scores, labels, meta, in_hw.long(), out_hw, out=out)
    with pytest.raises(ValueError, match="out_hw"):
        ops.detect_finish_var(boxes, scores, labels, meta, in_hw, out_hw[:1], out=out)
    with pytest.raises(ValueError, match="bytes"):
        ops.detect_finish_var(boxes, scores, labels, meta, in_hw, out_hw, out=out[:-16])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.detect_finish_var(boxes.cpu(), scores, labels, meta, in_hw, out_hw, out=out)
    # the library's own checks, with real device pointers
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(**kw):
        a = dict(boxes=p(boxes), scores=p(scores), labels=p(labels), count=p(meta[0]), status=p(meta[1]), in_hw=p(in_hw), out_hw=p(out_hw),
                 B=B, max_det=max_det, out=p(out), nbytes=total)
        a.update(kw)
        return _lib.lib.rn_detect_finish_var(a["boxes"], a["scores"], a["labels"], a["count"], a["status"], a["in_hw"], a["out_hw"], a["B"],
                                             a["max_det"], a["out"], a["nbytes"], st)
    for name in ("boxes", "scores", "labels", "count", "status", "in_hw", "out_hw", "out"):
        assert call(**{name: None}) == -1, name
    assert call(B=0) == -1 and call(max_det=0) == -1 and call(B=-2) == -1
    assert call(nbytes=total - 1) == -3 and call(nbytes=0) == -3
    assert call(boxes=C.c_void_p(boxes.data_ptr() + 4)) == -2 and call(out=C.c_void_p(out.data_ptr() + 8)) == -2
    assert call(labels=C.c_void_p(labels.data_ptr() + 4)) == -2
    with pytest.raises(ValueError, match="max_candidates"):
        ops.detect_levels([torch.zeros(1, 4, 2, device=DEV)], [torch.zeros(1, 4, 4, device=DEV)], torch.zeros(4, 4, device=DEV), None, 0.05,
                          0.01, 0.5, 3, max_candidates="most", image_hw_dev=torch.ones(1, 2, dtype=torch.int32, device=DEV), padded=True)
    with pytest.raises(ValueError, match="image_hw_dev"):
        ops.detect_levels([torch.zeros(1, 4, 2, device=DEV)], [torch.zeros(1, 4, 4, device=DEV)], torch.zeros(4, 4, device=DEV), None, 0.05,
                          0.01, 0.5, 3, image_hw_dev=torch.ones(2, 2, dtype=torch.int32, device=DEV), padded=True)
    torch.cuda.synchronize()
    assert bool((out == FILL).all())                              # nothing ran


# ---- 2. the model ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e(golden):
    "The fixture's net in eval mode, its two images, and ``net.predict`` on them in fp32 (computed once, never changed)."
    g = golden("e2e.npz")
    net = _model(g, DEV, E2E).eval()
    images, _ = _inputs(g, DEV)
    ref = _cpu(net.predict(images))
    assert [len(d["scores"]) for d in ref] == [53, 100]
    return g, net, images, ref


def _cpu(dets):
    return [{k: v.detach().cpu().clone() for k, v in d.items()} for d in dets]


def _same(got, want):
    "Bit equality of two detection lists (boxes, scores, labels; dtypes and lengths included)."
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):
        if set(g) != {"boxes", "scores", "labels"}:
            return False
        for k in ("boxes", "scores", "labels"):
            a, b = g[k].detach().cpu(), w[k].detach().cpu()
            if a.dtype != b.dtype or a.shape != b.shape or a.numpy().tobytes() != b.numpy().tobytes():
                return False
    return True


def _np(d):
    return {k: v.detach().float().cpu().numpy() if v.dtype != torch.int64 else v.detach().cpu().numpy() for k, v in d.items()}


def _meets_fp32_bars(got, want):
    "The bars of test_predict_matches_the_reference_fp32, per image: counts, box-set agreement with equal labels, the score profile."
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):
        g, w = _np(g), _np(w)
        if g["labels"].dtype != np.int64 or g["boxes"].dtype != np.float32:
            return False
        if abs(len(g["labels"]) - len(w["labels"])) > max(1, len(w["labels"]) // 100) or box_set_agreement(g, w) < 0.99:
            return False
        n = min(len(g["scores"]), len(w["scores"]))
        if not np.allclose(g["scores"][:n], w["scores"][:n], rtol=0, atol=1e-4):
            return False
    return True


def _meets_bf16_bars(got, ref):
    "The detection bars of test_forward_and_predict_bf16_autocast against the fp32 reference's detections ``ref``."
    n_top = 0
    for g, w in zip(got, ref):
        g, w = _np(g), _np(w)
        top = w["scores"] >= 0.06
        n_top += int(top.sum())
        if top.any():
            iou = _iou(w["boxes"][top], g["boxes"])
            same = w["labels"][top][:, None] == g["labels"][None, :]
            near = np.abs(w["scores"][top][:, None] - g["scores"][None, :]) <= 5e-3
            if ((iou >= 0.9) & same & near).any(1).mean() < 0.85 or np.median(np.where(same, iou, 0.0).max(1)) < 0.97:
                return False
    return n_top > 0


def _agree(got, want, exact):
    "``got`` equals ``want``: bit for bit when predict repeats itself (``exact``), else within the fp32 bars of the module docstring."
    return _same(got, want) if exact else _meets_fp32_bars(got, want)


def _reference(g):
    return [{"boxes": torch.from_numpy(g[f"det_boxes{b}"]), "scores": torch.from_numpy(g[f"det_scores{b}"]),
             "labels": torch.from_numpy(g[f"det_labels{b}"])} for b in range(2)]


@pytest.fixture(scope="module")
def repeats(e2e):
    """Does ``net.predict`` repeat itself bit for bit in this process?  fp32, up to sixteen more calls against the fixture's, stopping at
    the first that differs.  Where the conv stack's summation order is not fixed (the MI355X: every one of five measured calls
    differed) the first call settles it; sixteen equal calls are asked for before any test demands bit equality, so a device whose
    noise shows only now and then is not taken for a repeatable one."""
    _, net, images, ref = e2e
    return all(_same(_cpu(net.predict(images)), ref) for _ in range(16))


def _nonempty(dets):
    return all(len(d["scores"]) > 0 for d in dets)


def _images(sizes, seed):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.random((3, h, w), dtype=np.float32)).to(DEV) for h, w in sizes]


def _fresh_net(golden):
    return _model(golden("e2e.npz"), DEV, E2E).eval()


def _staged_eager(net, images, canvas, dtype=None):
    "Eager ``predict_staged`` on an arena of the test's own -> the list of dicts (CPU)."
    from pytorch_retinanet_amd import graph, ops
    in_hw = [(int(im.shape[1]), int(im.shape[2])) for im in images]
    staged = ops.new_image_arena(len(images), graph.image_pixel_class(in_hw), images[0].device, canvas)
    ops.image_stage(images, staged)
    with torch.autocast("cuda", dtype=dtype, enabled=dtype is not None):
        block = net.predict_staged(staged)
    return _cpu(ops.detect_result_dicts(block, len(images), net.detections_per_img))


def test_eager_predict_repeatability_decides_the_bars(e2e, repeats):
    """The determinism check first: ``net.predict`` on one input, several times in one process.  On the MI355X the calls differ (module
    docstring: boxes by up to 1.8e-4 px, scores by 6e-7 in fp32), so ``repeats`` is False there and the tests below hold eager calls and
    replays to the ``e2e.npz`` bars; where it is True they hold them to bit equality.  Either way two calls stay within the fp32 bars."""
    g, net, images, ref = e2e
    again = _cpu(net.predict(images))
    print(f"net.predict repeats itself bit for bit: {repeats}")
    assert _nonempty(again) and _meets_fp32_bars(again, ref) and _meets_fp32_bars(ref, _reference(g))


@pytest.mark.parametrize("amp", [None, torch.bfloat16], ids=["fp32", "bf16"])
def test_same_canvas_first_call_and_replay_equal_predict(e2e, repeats, amp):
    """Class list [(160, 160)] = the fixture's own canvas: the eager first call and the replays are ``net.predict(images)`` -- bit for bit
    when predict repeats itself, else within the ``e2e.npz`` bars of the dtype (module docstring)."""
    from pytorch_retinanet_amd.graph import CapturedPredict
    g, net, images, ref = e2e
    reference = _reference(g)
    if amp is not None:
        with torch.autocast("cuda", dtype=amp):
            ref = _cpu(net.predict(images))
        assert _meets_bf16_bars(ref, reference)                            # (the yardstick itself)
    assert _nonempty(ref)

    def holds(got):
        if not (_nonempty(got) and all(set(d) == {"boxes", "scores", "labels"} and d["labels"].dtype == torch.int64 for d in got)):
            return False
        if repeats:
            return _same(got, ref)
        return _meets_fp32_bars(got, reference) and _meets_fp32_bars(got, ref) if amp is None else _meets_bf16_bars(got, reference)
    p = CapturedPredict(net, [(160, 160)], amp_dtype=amp)
    first = p(images)
    assert p.stats == dict(p.stats, captures=0, replays=0, eager=1, fallbacks=0) and all(not t.is_cuda for d in first for t in d.values())
    assert holds(first), "the eager first call differs from net.predict"
    second = p(images)
    assert p.stats == dict(p.stats, captures=1, replays=1, eager=1, fallbacks=0, invalidations=0), p.stats
    assert holds(second), "the replay differs from net.predict"
    on_dev = p(images, to="device")
    assert p.stats["replays"] == 2 and all(t.is_cuda for d in on_dev for t in d.values()) and holds(_cpu(on_dev))
    if amp is None:
        assert _meets_fp32_bars(second, reference)                         # the e2e.npz bars, whatever predict's repeatability
    else:
        # amp_dtype=None follows the caller's autocast state: the same key, the same graph's result
        q = CapturedPredict(net, [(160, 160)])
        with torch.autocast("cuda", dtype=amp):
            assert holds(q(images)) and holds(q(images))
        assert q.stats["replays"] == 1 and q._autocast_dtype() is None


# (every batch holds a portrait image, so its own canvas is 160 x 160: inside (160, 192), outside (128, 160))
BATCHES_160_192 = [[(120, 150), (140, 128)], [(100, 140), (150, 128)], [(128, 160), (100, 90)], [(150, 120), (110, 150)]]


def test_one_graph_serves_every_batch_of_a_class(e2e, repeats):
    "Four batches whose sizes differ inside the class (160, 192): one capture; each replay is eager ``predict_staged`` of that batch."
    from pytorch_retinanet_amd.graph import CapturedPredict
    _, net, _, _ = e2e
    p = CapturedPredict(net, [(128, 160), (160, 192)])
    for i, sizes in enumerate(BATCHES_160_192):
        images = _images(sizes, seed=100 + i)
        assert p._class_of(images)[0] == (160, 192)
        want = _staged_eager(net, images, (160, 192))
        got = p(images)
        assert _nonempty(want) and _agree(got, want, repeats), i
    assert p.stats == dict(p.stats, captures=1, replays=3, eager=1, fallbacks=0, invalidations=0), p.stats
    # another B, another class: each captures again
    one = _images([(140, 128)], seed=7)
    want = _staged_eager(net, one, (160, 192))
    assert _agree(p(one), want, repeats) and _agree(p(one), want, repeats) and _nonempty(want)
    assert p.stats["captures"] == 2 and p.stats["replays"] == 4
    wide = _images([(120, 150), (100, 125)], seed=8)                        # own canvas 128 x 160: the first class
    want = _staged_eager(net, wide, (128, 160))
    assert _agree(p(wide), want, repeats) and _agree(p(wide), want, repeats) and _nonempty(want)
    assert p.stats["captures"] == 3 and p.stats["replays"] == 5 and p.stats["fallbacks"] == 0
    assert _agree(want, _cpu(net.predict(wide)), repeats)                   # (its own canvas: predict itself)
    # a batch no class holds falls back to net.predict
    q = CapturedPredict(net, [(128, 160)])
    tall = _images(BATCHES_160_192[0], seed=100)                            # own canvas 160 x 160
    want = _cpu(net.predict(tall))
    assert _agree(q(tall), want, repeats) and _agree(q(tall), want, repeats) and _nonempty(want)
    assert q.stats == dict(q.stats, captures=0, replays=0, eager=0, fallbacks=2)


def _perturbed(state, scale):
    return {k: (v * scale if v.is_floating_point() and "running_var" not in k and "anchor" not in k else v) for k, v in state.items()}


def test_changed_weights_drop_the_graphs(golden, repeats):
    """After a replay the weights change three ways -- load_state_dict, one MasterSGD step through the library's kernels, the EMA swap --
    and each time the next call is a fresh eager ``net.predict`` on the new weights, not the old graph's: every change moves the
    detections OUT of the bars against every earlier result, so a graph that survived it would fail here."""
    from pytorch_retinanet_amd.graph import CapturedPredict
    from pytorch_retinanet_amd.optim import MasterSGD, WeightEMA
    g = golden("e2e.npz")
    net = _fresh_net(golden)
    images, targets = _inputs(g, DEV)
    p = CapturedPredict(net, [(160, 160)])
    seen = []

    def check(what, invalidations):
        want = _cpu(net.predict(images))
        assert _nonempty(want), what
        assert all(not _meets_fp32_bars(old, want) for old in seen), f"{what}: the weights did not move the detections out of the bars (the test would show nothing)"
        seen.append(want)
        assert _agree(p(images), want, repeats), f"{what}: the call after the change is not net.predict on the new weights"
        assert p.stats["invalidations"] == invalidations, (what, p.stats)
        assert _agree(p(images), want, repeats) and p.stats["replays"] == invalidations + 1, (what, p.stats)      # ... and replays again

    check("initial", 0)
    net.load_state_dict(_perturbed(net.state_dict(), 1.01))
    check("load_state_dict", 1)
    opt = MasterSGD(net.parameters(), lr=1e-4, momentum=0.9)
    ema = opt.weight_ema = WeightEMA(0.5)

    def train_step():
        net.train()
        opt.zero_grad(set_to_none=True)
        out = net(images, [dict(t) for t in targets])
        (out["classification_loss"] + out["regression_loss"]).backward()
        opt.step()
        net.eval()
    train_step()
    check("MasterSGD.step", 2)
    train_step()                                                            # (the average now differs from the weights)
    check("a second step", 3)
    with ema.swapped(net.parameters()):
        check("WeightEMA.swapped", 4)
    assert _agree(p(images), seen[-2], repeats) and p.stats["invalidations"] == 5    # swapped back: the weights of the second step again


def test_candidate_overflow_reruns_eagerly_and_reports_it(e2e, repeats):
    from pytorch_retinanet_amd.graph import CapturedPredict
    _, net, images, ref = e2e
    p = CapturedPredict(net, [(160, 160)], max_candidates=8)
    for i in range(3):                                                      # eager, capture + replay, replay: all overflow
        assert _agree(p(images), ref, repeats), i
    assert p.stats["overflows"] == 3 and p.stats["fallbacks"] == 3 and p.stats["replays"] == 2 and p.stats["captures"] == 1, p.stats


def test_trainer_test_through_the_predictor_equals_the_default(golden, repeats):
    "``SimpleTrainer(predict_image_capacity=[(160, 160)]).test`` -> the detections and the 12 COCO statistics of the default ``test()``."
    import pytorch_retinanet_amd as P
    net = _fresh_net(golden)
    conf = P.load_hparams()
    conf.model.update(E2E)
    conf.dataloader.test_bs = 2
    conf.dataloader.args.pin_memory = False
    model = P.RetinaNetModel(conf)
    model.net = net
    sizes = [(120, 150), (140, 128), (150, 120), (128, 140)]                # every batch of two: own canvas 160 x 160
    images = [im.cpu() for im in _images(sizes, seed=55)]
    first = _cpu(net.predict([im.to(DEV) for im in images[:2]]) + net.predict([im.to(DEV) for im in images[2:]]))
    assert all(len(d["labels"]) >= 6 for d in first)

    class DS(torch.utils.data.Dataset):
        def __len__(self): return 4
        def __getitem__(self, i):
            d = first[i]
            boxes = torch.cat([d["boxes"][[0, 3, 5]], torch.tensor([[2.0, 2.0, 9.0, 9.0]])])
            labels = torch.cat([d["labels"][[0, 3, 5]], torch.tensor([1])])
            return images[i], {"boxes": boxes, "labels": labels, "image_id": torch.tensor([10 + i])}, 10 + i
    model.test_ds = DS()

    def run(trainer):
        res, outs = trainer.test(model)
        dets = {k: v for o in outs for k, v in o["detections"].items()}
        return res, [dets[10 + i] for i in range(4)], np.asarray(model.test_evaluator.coco_eval["bbox"].stats, dtype=np.float64)
    res0, dets0, stats0 = run(P.SimpleTrainer(device=DEV, precision="32"))
    trainer = P.SimpleTrainer(device=DEV, precision="32", predict_image_capacity=[(160, 160)])
    res1, dets1, stats1 = run(trainer)
    assert _agree(dets0, first, repeats) and _agree(dets1, dets0, repeats) and _nonempty(dets1)
    # The 12 COCO statistics are EQUAL, whether or not predict repeats itself bit for bit.  They are step functions of the detections:
    # a statistic moves only when a detection changes sides of an IoU threshold (0.5 .. 0.95) or of an area range (32^2, 96^2 px^2)
    # or two detections of a category swap score ranks across a true positive.  Every true positive here is a copy of a GT box
    # (IoU 1 - 1e-6 with it), and the run-to-run noise is 2e-4 px in the boxes and 6e-7 in the scores against score gaps of ~1e-3:
    # it moves an IoU by ~1e-5 and an area by ~1e-2 px^2, which crosses none of those steps.
    print("COCO statistics, default test():", stats0.tolist(), "through the predictor:", stats1.tolist())
    assert stats1.shape == (12,) and stats0[0] > 0
    assert np.array_equal(stats0, stats1) and float(res0["AP"]) == float(res1["AP"]) == stats1[0]
    assert trainer.predictor.stats == dict(trainer.predictor.stats, captures=1, replays=1, eager=1, fallbacks=0)
    assert model.predictor is None                                          # removed again: a later default test() is the default


def test_replays_outlive_the_caches_their_graphs_point_into(e2e, repeats):
    """A captured pass holds the ADDRESS of the anchors, which ``AnchorGenerator._cache`` owns and clears once it holds more than 16
    feature-map shapes -- every ``net.predict`` on a canvas of its own adds one, the predictor's own fallback included.  Between two
    replays the cache is driven past that limit the way ``predict`` drives it (``anchor_generator(images, feature_maps)``; this model's
    min_size 128 / max_size 160 admits only eleven canvases, so the seventeen shapes are fed to the generator directly, after three
    real fallback calls), and the allocator is made to hand the freed blocks out again, filled with garbage.  The replay after it is
    the replay before it: the entry keeps what its graph points at alive."""
    from pytorch_retinanet_amd.graph import CapturedPredict
    from pytorch_retinanet_amd.transform import ImageList
    _, net, images, ref = e2e
    p = CapturedPredict(net, [(160, 160)])
    assert _agree(p(images), ref, repeats) and _agree(p(images), ref, repeats) and p.stats["replays"] == 1
    gen = net.anchor_generator
    held, sizes = [t.data_ptr() for t in gen._cache.values()], sorted({t.numel() for t in gen._cache.values()})
    assert held
    q = CapturedPredict(net, [(32, 32)])                                     # no class holds anything: every call is a fallback
    for i, size in enumerate([(128, 70), (70, 128), (128, 40)]):             # own canvases 160 x 96, 96 x 160, 160 x 64
        assert len(q(_images([size], seed=200 + i))) == 1
    assert q.stats["fallbacks"] == 3 and q.stats["replays"] == 0
    one = ImageList(torch.empty(1, 3, 8, 8, device=DEV), [(8, 8)])
    for i in range(17):                                                       # seventeen more feature-map shapes: the cache clears itself
        gen(one, [torch.empty(1, 1, 3 + i, 5 + j, device=DEV) for j in range(len(gen.strides))])
    assert not set(held) & {t.data_ptr() for t in gen._cache.values()}, "the cache still owns the anchors: the test would show nothing"
    junk = [torch.full((n,), float("nan"), device=DEV) for n in sizes for _ in range(32)]     # (whatever was freed is handed out again)
    torch.cuda.synchronize()
    assert _agree(p(images), ref, repeats) and p.stats["replays"] == 2 and p.stats["invalidations"] == 0
    del junk
