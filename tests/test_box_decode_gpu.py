"""GPU: the standard box decode (``decode="standard"`` / ``Retinanet(box_decode="standard")``) -- ``decode_clip_kernel`` and
``seg_count_kernel``'s standard instantiations against the numpy restatement (``box_utils.decode_boxes_reference``), the detect
chain against the UNCHANGED CPU oracle, and the model, ``predict_staged`` and ``graph.CapturedPredict`` with the switch.

The oracle route.  The oracle knows the reference decode (Q4) only.  Fed ZERO deltas and per-image anchors [B, A, 4] equal to the
restatement's clipped standard boxes, its decode gives cx = aw * 0 + acx, w = aw * exp(0): the anchors back to within a rounding,
and the rest of its chain (clip, remove_small_boxes, NMS, top-k) runs on the standard boxes.

Bars: boxes ``rtol=1e-5, atol=1e-3`` (SURVEY 8d's K4 bar), scores ``rtol=1e-6, atol=1e-7``, labels equal; ``torch.equal`` wherever two
runs of the same kernels on the same values are compared; the ``e2e.npz`` fp32 bars for whole predicts (the conv stack is not
repeatable bit for bit on the MI355X, tests/test_captured_predict_gpu.py)."""
import numpy as np
import pytest
import torch

import synth
from test_e2e_gpu import DEV, E2E, _inputs, _model, box_set_agreement

pytestmark = pytest.mark.gpu

REG_W = (10.0, 10.0, 5.0, 5.0)
RTOL, ATOL = 1e-5, 1e-3
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from pytorch_retinanet_amd import ops as _ops
    return _ops


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def rounded(a, dtype):
    return a if dtype == torch.float32 else (synth.round_f16(a) if dtype == torch.float16 else synth.round_bf16(a))


def restate(d, a, reg_w, decode="standard", hw=None):
    from pytorch_retinanet_amd.box_utils import decode_boxes_reference
    return decode_boxes_reference(d, a, reg_w, decode, image_hw=hw)


def random_anchors(rng, n, lo=16.0, hi=512.0, span=1000.0):
    cx, cy = rng.uniform(0, span, n), rng.uniform(0, span, n)
    w, h = rng.uniform(lo, hi, n), rng.uniform(lo, hi, n)
    return np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(np.float32)


def random_deltas(rng, shape):
    "t = d / REG_W ~ N(0, 0.3) in the centres, N(0, 0.5) in the sizes; every 16th row has size deltas above the clip."
    d = (rng.standard_normal(shape + (4,)) * np.array([3.0, 3.0, 2.5, 2.5])).astype(np.float32)
    flat = d.reshape(-1, 4)
    flat[::16, 2:] = rng.uniform(21.0, 60.0, (len(flat[::16]), 2)).astype(np.float32)
    return d


# ---- the decode kernel against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("clip_to", [None, [(600, 800), (333, 500)]], ids=["noclip", "hw"])
def test_decode_clip_standard_equals_the_restatement(ops, dtype, clip_to):
    rng = np.random.default_rng(3001)
    B, A = 2, 1000
    a = random_anchors(rng, A)
    d = rounded(random_deltas(rng, (B, A)), dtype)
    hw = None if clip_to is None else dev(np.asarray(clip_to, np.int32))
    got = ops.decode_clip(dev(d, dtype), dev(a), hw, REG_W, decode="standard").cpu().numpy()
    want = restate(d, a, REG_W, hw=clip_to)
    assert got.shape == (B, A, 4) and got.dtype == np.float32
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
    # reg_w[2] and reg_w[3] are really read: with unit size weights the widths differ
    other = ops.decode_clip(dev(d, dtype), dev(a), hw, (10.0, 10.0, 1.0, 1.0), decode="standard").cpu().numpy()
    assert np.abs(other - got).max() > 1.0
    # [A, 4] deltas: the squeezed form
    one = ops.decode_clip(dev(d[0], dtype), dev(a), None, REG_W, decode="standard").cpu().numpy()
    np.testing.assert_allclose(one, restate(d[0], a, REG_W), rtol=RTOL, atol=ATOL)


def test_decode_clip_standard_past_one_grid_pass(ops):
    "B = 1, A = 4096 * 256 + 300 rows: the 4 096-block grid walks its stride loop a second time."
    rng = np.random.default_rng(3002)
    A = 4096 * 256 + 300
    a = random_anchors(rng, A)
    d = random_deltas(rng, (1, A))
    got = ops.decode_clip(dev(d), dev(a), dev(np.asarray([[700, 900]], np.int32)), REG_W, decode="standard").cpu().numpy()
    np.testing.assert_allclose(got, restate(d, a, REG_W, hw=[(700, 900)]), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_equal_bits_when_the_size_deltas_repeat_the_centre_deltas(ops, dtype):
    "d[..., 2:] = d[..., :2], equal weights, |t| < CLIP: the standard kind runs the reference kind's operations on the same operands."
    rng = np.random.default_rng(3003)
    B, A = 2, 1000
    a = random_anchors(rng, A)
    d = rounded(np.clip(rng.standard_normal((B, A, 4)) * 8.0, -20.0, 20.0).astype(np.float32), dtype)      # |t| <= 4 < CLIP = 4.135
    d[..., 2:] = d[..., :2]
    rw = (10.0, 5.0, 10.0, 5.0)
    assert np.abs(d / np.asarray(rw, np.float32)).max() < ops.BOX_XFORM_CLIP
    hw = dev(np.asarray([(600, 800), (333, 500)], np.int32))
    for h in (None, hw):
        s = ops.decode_clip(dev(d, dtype), dev(a), h, rw, decode="standard")
        r = ops.decode_clip(dev(d, dtype), dev(a), h, rw, decode="reference")
        assert torch.equal(s, r) and torch.equal(r, ops.decode_clip(dev(d, dtype), dev(a), h, rw))


def test_the_clip_and_the_edge_cases(ops):
    """t2 in {CLIP, nextafter(CLIP, inf), 10, 88.8, +inf}: the bits of the t2 == CLIP row; just below CLIP a smaller width; t2 = -inf
    a zero width; t2 = NaN a NaN box, which ``detect`` does not return (neither the zero-width one)."""
    clip = np.float32(ops.BOX_XFORM_CLIP)
    t2 = np.array([clip, np.nextafter(clip, np.float32(np.inf)), 10.0, 88.8, np.inf, np.nextafter(clip, np.float32(-np.inf)), -np.inf, np.nan],
                  np.float32)
    n = len(t2)
    an = np.array([[10.0, 20.0, 18.0, 30.0]] * n, np.float32)
    d = np.zeros((n, 4), np.float32)
    d[:, 0], d[:, 1], d[:, 2], d[:, 3] = 0.25, -0.125, t2, 0.5
    out = ops.decode_clip(dev(d), dev(an), None, decode="standard").cpu().numpy()
    for r in range(1, 5):
        assert out[r].tobytes() == out[0].tobytes(), r
    assert out[5, 2] - out[5, 0] < out[0, 2] - out[0, 0]
    assert out[6, 0] == out[6, 2] and np.isfinite(out[6]).all()
    assert np.isnan(out[7, 0]) and np.isnan(out[7, 2]) and np.isfinite(out[7, [1, 3]]).all()
    np.testing.assert_allclose(out[:7], restate(d, an, (1.0, 1.0, 1.0, 1.0))[:7], rtol=RTOL, atol=ATOL)
    # the chain: one class, every row a confident candidate on an anchor of its own, 1 000 px apart (nothing for NMS to remove)
    an2 = an + (np.arange(n, dtype=np.float32) * 1000.0)[:, None] * np.array([1.0, 0.0, 1.0, 0.0], np.float32)
    d2 = d.copy()
    d2[:, 2] = np.where(t2 > 1.0, np.float32(1.0), t2)                               # (widths of 8 e px for the rows that live; -inf and NaN stay)
    cls = np.full((1, n, 1), 3.0, np.float32) + np.arange(n, dtype=np.float32)[None, :, None] * 0.01
    dets = ops.detect(dev(cls), dev(d2[None]), dev(an2), [(4000, 10000)], 0.05, 1e-2, 0.5, 100, decode="standard")
    boxes = dets[0]["boxes"].cpu().numpy()
    assert len(boxes) == n - 2 and np.isfinite(boxes).all()
    assert sorted(int(x // 1000) for x in boxes[:, 0]) == list(range(n - 2))          # rows 6 (width 0) and 7 (NaN) are absent


def test_round_trip_on_the_device(ops):
    "decode_clip(bbox_2_activ(gt, anchors) * reg_w, anchors, decode='standard') returns gt."
    from pytorch_retinanet_amd.box_utils import bbox_2_activ
    from test_box_decode import gt_near
    rng = np.random.default_rng(3004)
    a = random_anchors(rng, 2000)
    gt = gt_near(rng, a)
    d = bbox_2_activ(dev(gt), dev(a)) * torch.tensor(REG_W, device=DEV)
    got = ops.decode_clip(d, dev(a), None, REG_W, decode="standard").cpu().numpy()
    np.testing.assert_allclose(got, gt, rtol=RTOL, atol=ATOL)
    ref = ops.decode_clip(d, dev(a), None, REG_W, decode="reference").cpu().numpy()
    assert (np.abs(ref - gt).max(1) > 1.0).mean() >= 0.9


# ---- the detect chain against the oracle -------------------------------------------------------------------------------------------
def cmp_dets(got, ref):
    "As tests/test_hip_parity.py compares detections: labels equal, scores rtol 1e-6 / atol 1e-7, boxes rtol 1e-5 / atol 1e-3."
    assert len(got) == len(ref)
    for b, (g_, r_) in enumerate(zip(got, ref)):
        gl, gs, gb = (g_[k].cpu().numpy() for k in ("labels", "scores", "boxes"))
        assert gl.shape == r_["labels"].shape, (b, gl.shape, r_["labels"].shape)
        assert np.array_equal(gl, r_["labels"]), b
        np.testing.assert_allclose(gs, r_["scores"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(gb, r_["boxes"], rtol=RTOL, atol=ATOL)


def same_dets(x, y):
    return len(x) == len(y) and all(torch.equal(a_[k], b_[k]) for a_, b_ in zip(x, y) for k in ("boxes", "scores", "labels"))


def oracle_route(oracle_lib, cls, box, anc, hw, reg_w):
    std = restate(box, anc, reg_w, hw=hw)                                          # [B, A, 4], clipped to each image
    return oracle_lib.detect(cls, np.zeros_like(box), np.ascontiguousarray(std), hw)


def split_levels(t, counts):
    outs, o = [], 0
    for n in counts:
        outs.append(t[:, o:o + n].contiguous())
        o += n
    return outs


CHAIN_HW = [(224, 160), (200, 150)]
CHAIN_RW = (1.0, 1.0, 2.0, 2.0)                                                    # (size weights that are not the centre weights)


@pytest.fixture(scope="module")
def chain(ops, oracle_lib):
    "The chain's inputs in fp32, computed once and never changed: 224 x 160 levels (A = 6 759), K = 5, B = 2."
    rng = np.random.default_rng(3005)
    levels = synth.levels_for(224, 160)
    counts = [h * w * 9 for h, w, _ in levels]
    A, K, B = sum(counts), 5, 2
    assert A == 6759
    cls, box = synth.head_outputs(rng, B, A, K, cls_mean=-3.0, cls_std=1.3)           # dw, dh drawn independently of dx, dy
    box[..., 2:] *= np.float32(2.0)                                                # t2, t3 ~ N(0, 0.1) under CHAIN_RW
    cells = [oracle_lib.cell_anchors(s, synth.ANCHOR_RATIOS) for s in synth.ANCHOR_SIZES]
    anc = ops.anchors_emit(levels, [dev(c) for c in cells], 0.0)
    return dict(cls=cls, box=box, anc=anc, anc_np=anc.cpu().numpy(), counts=counts, A=A, K=K, B=B)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_detect_standard_vs_oracle_route_and_levels(ops, oracle_lib, chain, dtype):
    cls, box = rounded(chain["cls"], dtype), rounded(chain["box"], dtype)
    dc, db, anc = dev(cls, dtype), dev(box, dtype), chain["anc"]
    args = (anc, CHAIN_HW, 0.05, 1e-2, 0.5, 100, CHAIN_RW)
    whole = ops.detect(dc, db, *args, decode="standard")
    lev = ops.detect_levels(split_levels(dc, chain["counts"]), split_levels(db, chain["counts"]), *args, decode="standard")
    assert same_dets(whole, lev)
    ref = oracle_route(oracle_lib, cls, box, chain["anc_np"], CHAIN_HW, CHAIN_RW)
    assert all(len(r["labels"]) > 20 for r in ref)
    cmp_dets(whole, ref)
    cmp_dets(lev, ref)
    # the overflow retry (1 000 candidates per image are too few) gives the same result
    assert same_dets(ops.detect(dc, db, *args, max_candidates=1000, decode="standard"), whole)
    # padded outputs, sizes read on the device: the same rows
    hw_dev = dev(np.asarray(CHAIN_HW, np.int32))
    ob, osc, ol, meta = ops.detect_levels(split_levels(dc, chain["counts"]), split_levels(db, chain["counts"]), anc, None, 0.05, 1e-2, 0.5,
                                          100, CHAIN_RW, max_candidates="all", image_hw_dev=hw_dev, padded=True, decode="standard")
    meta = meta.cpu()
    assert not bool(meta[1].any())
    padded = [{"boxes": ob[b, :n], "scores": osc[b, :n], "labels": ol[b, :n]} for b, n in enumerate(meta[0].tolist())]
    assert same_dets(padded, whole)
    # the enqueue-only form (what a graph capture records) runs the same chain
    handle = []
    assert ops.detect_levels([dc], [db], anc, CHAIN_HW, 0.05, 1e-2, 0.5, 100, CHAIN_RW, max_candidates="all", enqueue_only=handle,
                             decode="standard") == []
    handle[0]()
    eb, es, el, em = handle[1][:4]
    em = em.cpu()
    assert same_dets([{"boxes": eb[b, :n], "scores": es[b, :n], "labels": el[b, :n]} for b, n in enumerate(em[0].tolist())], whole)


def test_reference_decode_differs_on_the_same_inputs_and_is_what_it_was(ops, oracle_lib, chain, golden):
    """The test that cannot pass without the feature: on inputs whose (dw, dh) are not (dx, dy) the two decodes return boxes more
    than 1 px apart; the reference kind is still the oracle's own detect, and the default argument is the reference kind."""
    dc, db, anc = dev(chain["cls"]), dev(chain["box"]), chain["anc"]
    args = (anc, CHAIN_HW, 0.05, 1e-2, 0.5, 100, CHAIN_RW)
    std = ops.detect(dc, db, *args, decode="standard")
    ref = ops.detect(dc, db, *args, decode="reference")
    assert same_dets(ref, ops.detect(dc, db, *args))
    params = oracle_lib.default_detect_params(reg_w=CHAIN_RW)
    cmp_dets(ref, oracle_lib.detect(chain["cls"], chain["box"], chain["anc_np"], CHAIN_HW, params))
    worst = 0.0
    for s, r in zip(std, ref):
        sb, rb = s["boxes"].cpu().numpy(), r["boxes"].cpu().numpy()
        if sb.shape != rb.shape:
            worst = np.inf
        else:
            worst = max(worst, float(np.abs(sb - rb).max()))
    print(f"standard against reference decode, same inputs: detection boxes up to {worst:.1f} px apart")
    assert worst > 1.0
    # an existing golden case: decode="reference" and no argument give identical tensors
    g = golden("detect.npz")
    hw = [tuple(int(x) for x in r) for r in g["toy_hw"]]
    toy = (dev(g["toy_cls"]), dev(g["toy_box"]), dev(g["toy_anchors"]), hw, 0.05, 1e-2, 0.5, 100)
    plain, named = ops.detect(*toy), ops.detect(*toy, decode="reference")
    assert same_dets(plain, named) and sum(len(d["labels"]) for d in plain) > 0
    cmp_dets(named, [{k: g[f"toy_{k}{b}"] for k in ("boxes", "scores", "labels")} for b in range(2)])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_detect_standard_exploding_head_outputs(ops, oracle_lib, dtype):
    """The inputs of test_hip_parity's test_detect_exploding_head_outputs_vs_oracle (logits x 1000, deltas x 500, the overflow retry's
    one-list form): the clip keeps w <= 62.5 aw, so the clipped standard boxes are finite and the oracle route applies; every
    returned box is finite, inside its image and at least min_box wide and high."""
    rng = np.random.default_rng(77)
    levels = synth.levels_for(224, 160)
    A, K, B = sum(h * w * 9 for h, w, _ in levels), 5, 2
    cls = (rng.standard_normal((B, A, K)) * 1000.0).astype(np.float32)
    box = (rng.standard_normal((B, A, 4)) * 500.0).astype(np.float32)
    cls, box = rounded(cls, dtype), rounded(box, dtype)
    cells = [oracle_lib.cell_anchors(s, synth.ANCHOR_RATIOS) for s in synth.ANCHOR_SIZES]
    anc = ops.anchors_emit(levels, [dev(c) for c in cells], 0.0)
    got = ops.detect(dev(cls, dtype), dev(box, dtype), anc, CHAIN_HW, 0.05, 1e-2, 0.5, 100, max_candidates=4096, decode="standard")
    assert np.isfinite(restate(box, anc.cpu().numpy(), (1.0, 1.0, 1.0, 1.0), hw=CHAIN_HW)).all()
    ref = oracle_route(oracle_lib, cls, box, anc.cpu().numpy(), CHAIN_HW, (1.0, 1.0, 1.0, 1.0))
    cmp_dets(got, ref)
    assert all(len(r["labels"]) > 0 for r in ref)
    for d, (h, w) in zip(got, CHAIN_HW):
        b = d["boxes"].cpu().numpy()
        assert np.isfinite(b).all() and b.min() >= 0.0 and b[:, [0, 2]].max() <= w and b[:, [1, 3]].max() <= h
        assert (b[:, 2] - b[:, 0] >= np.float32(1e-2)).all() and (b[:, 3] - b[:, 1] >= np.float32(1e-2)).all()


# ---- the model -------------------------------------------------------------------------------------------------------------------------
def _cpu(dets):
    return [{k: v.detach().cpu().clone() for k, v in d.items()} for d in dets]


def meets_fp32_bars(got, want):
    "The ``e2e.npz`` fp32 bars per image: counts within max(1, 1 %), >= 99 % box-set agreement at IoU 0.999 with equal labels, scores 1e-4."
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):
        g, w = ({k: v.detach().cpu().numpy() for k, v in x.items()} for x in (g, w))
        if abs(len(g["labels"]) - len(w["labels"])) > max(1, len(w["labels"]) // 100) or box_set_agreement(g, w) < 0.99:
            return False
        n = min(len(g["scores"]), len(w["scores"]))
        if not np.allclose(g["scores"][:n], w["scores"][:n], rtol=0, atol=1e-4):
            return False
    return True


@pytest.fixture(scope="module")
def e2e_net(golden):
    g = golden("e2e.npz")
    net = _model(g, DEV, E2E).eval()
    images, _ = _inputs(g, DEV)
    return net, images


def head_outputs_of(net, images):
    "predict's pipeline up to the head, once: the two decodes are then compared on the SAME head outputs."
    with torch.no_grad():
        il, _ = net.transform(images, None, **net._batch_layout())
        fmaps = net.fpn(net.backbone(il.tensors))
        anchors = net.anchor_generator(il, fmaps)
        return il, anchors, net.retinanet_head.forward_levels(fmaps)


def test_predict_with_the_standard_decode(ops, e2e_net):
    from pytorch_retinanet_amd.config import BBOX_REG_WEIGHTS, MIN_BOX_SIZE
    net, images = e2e_net
    assert net.box_decode == "reference"
    original = [(int(im.shape[-2]), int(im.shape[-1])) for im in images]
    il, anchors, out = head_outputs_of(net, images)
    try:
        by_kind = {}
        for kind in ("reference", "standard"):
            net.box_decode = kind
            model = net.transform.postprocess(net.process_detections_levels(out, anchors, il.image_sizes), il.image_sizes, original)
            direct = ops.detect_levels(out["cls_levels"], out["bbox_levels"], anchors, il.image_sizes, net.score_thres, MIN_BOX_SIZE,
                                       net.nms_thres, net.detections_per_img, reg_w=BBOX_REG_WEIGHTS, decode=kind)
            direct = net.transform.postprocess(direct, il.image_sizes, original)
            assert same_dets(model, direct), kind                                   # the model passes its attribute on
            by_kind[kind] = _cpu(model)
            assert all(len(d["scores"]) > 0 for d in model)
            assert meets_fp32_bars(_cpu(net.predict(images)), by_kind[kind]), kind   # predict itself, up to the conv stack's noise
        assert not same_dets(by_kind["standard"], by_kind["reference"])
        assert not meets_fp32_bars(by_kind["standard"], by_kind["reference"])       # ... by more than that noise
        # process_detections (concatenated outputs) passes it on too
        net.box_decode = "standard"
        cat = {"cls_preds": torch.cat([c[..., :net.num_classes] for c in out["cls_levels"]], 1).contiguous(),
               "bbox_preds": torch.cat(list(out["bbox_levels"]), 1).contiguous()}
        whole = net.transform.postprocess(net.process_detections(cat, anchors, il.image_sizes), il.image_sizes, original)
        assert same_dets(_cpu(whole), by_kind["standard"])
    finally:
        net.box_decode = "reference"


def test_captured_predict_follows_the_attribute(e2e_net):
    "Replays match eager predict within the ``e2e.npz`` bars; flipping ``net.box_decode`` captures a new graph, never replays a stale one."
    from pytorch_retinanet_amd.graph import CapturedPredict
    net, images = e2e_net
    try:
        want = {}
        for kind in ("reference", "standard"):
            net.box_decode = kind
            want[kind] = _cpu(net.predict(images))
        assert not meets_fp32_bars(want["standard"], want["reference"])             # (the two are told apart by the bars used below)
        net.box_decode = "standard"
        p = CapturedPredict(net, [(160, 160)])
        first, second = p(images), p(images)                                      # eager, then capture + replay
        assert p.stats["captures"] == 1 and p.stats["replays"] == 1 and p.stats["fallbacks"] == 0, p.stats
        assert meets_fp32_bars(first, want["standard"]) and meets_fp32_bars(second, want["standard"])
        assert meets_fp32_bars(p(images), want["standard"]) and p.stats["replays"] == 2
        net.box_decode = "reference"                                              # flipped between calls
        third, fourth = p(images), p(images)
        assert p.stats["captures"] == 2 and p.stats["replays"] == 3 and p.stats["fallbacks"] == 0 and p.stats["invalidations"] == 0, p.stats
        assert meets_fp32_bars(third, want["reference"]) and meets_fp32_bars(fourth, want["reference"])
        assert not meets_fp32_bars(fourth, want["standard"])
        net.box_decode = "standard"                                               # back: the first graph is still the standard decode's
        fifth = p(images)
        assert p.stats["captures"] == 2 and p.stats["replays"] == 4, p.stats
        assert meets_fp32_bars(fifth, want["standard"]) and not meets_fp32_bars(fifth, want["reference"])
    finally:
        net.box_decode = "reference"
