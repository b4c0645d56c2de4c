"""GPU: Soft-NMS (csrc/softnms.hip) -- ``rn_soft_nms_segments`` against the numpy restatement ``box_utils.soft_nms_reference`` at every
length class of the kernels, the detect chain with a soft kind against the restatement applied to the chain's own candidates, the
hard path against ``rn_detect_levels_kind``, and the model and ``graph.CapturedPredict`` with the switch.

Bars.  Linear: bit equality (every step of the rule is one fp32 operation on both sides).  Gaussian: equal indices and counts, scores
within ``rtol = 4 * R * 2**-24`` for a segment of R rounds -- each decay multiplies by a weight that may differ by one fp32 unit between
two correct double ``exp`` implementations, and the product is rounded once more per round.  That such a difference cannot change a
pick is asserted on the restatement alone (``soft_nms_cases.Margin``): at every round the runner-up is further below the pick than
the bound, or is an exact copy of its box and score.  The seeds below were chosen on the CPU for that.

One op call takes ONE ``max_keep``, so the ten lengths run in one call capped at 48 (the long segments stay within seconds), and the
lengths up to 257 run again in a second call without a cap."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import soft_nms_cases as cases
import synth
from test_e2e_gpu import DEV, E2E, _inputs, _model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ("soft_linear", "soft_gaussian")
SEED, SEED_DUP = 92, 1051


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from pytorch_retinanet_amd import ops as _ops
    return _ops


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def word_bits(t):
    return t.contiguous().view(torch.int32)


# ---- the op ---------------------------------------------------------------------------------------------------------------------------
OP_CASES = {"all-capped": (SEED, cases.LENGTHS, cases.CAP, False), "short-uncapped": (SEED, cases.SHORT, None, False),
            "duplicates-capped": (SEED_DUP, cases.LENGTHS, cases.CAP, True), "duplicates-uncapped": (SEED_DUP, cases.SHORT, None, True)}


@pytest.fixture(scope="module")
def op_inputs():
    "Inputs and expected outputs per case and method, computed once and never changed."
    out = {}
    for name, (seed, lengths, cap, dup) in OP_CASES.items():
        boxes, scores, off = cases.segments(seed, lengths, dup)
        out[name] = dict(boxes=boxes, scores=scores, off=off, cap=cap,
                         want={m: cases.expected(boxes, scores, off, m, cap) for m in METHODS})
    return out


def run_op(ops, case, method):
    return ops.soft_nms_segments(dev(case["boxes"]), dev(case["scores"]), dev(case["off"]), cases.IOU_THR, method, max_keep=case["cap"])


@pytest.mark.parametrize("name", list(OP_CASES))
def test_linear_equals_the_restatement_bit_for_bit(ops, op_inputs, name):
    case = op_inputs[name]
    keep, ks, cnt = run_op(ops, case, "soft_linear")
    wk, ws, wc, _ = case["want"]["soft_linear"]
    assert cnt.dtype == torch.int32 and keep.dtype == torch.int64 and ks.dtype == torch.float32
    assert torch.equal(cnt.cpu(), torch.from_numpy(wc))
    assert int(wc.max()) >= 14 and (case["cap"] is None or int(wc.max()) == case["cap"])
    off = case["off"]
    live = np.zeros(len(case["scores"]), bool)                          # keep is defined up to each segment's count
    for s, c in enumerate(wc):
        live[off[s]:off[s] + c] = True
    live = torch.from_numpy(live)
    assert torch.equal(keep.cpu()[live], torch.from_numpy(wk)[live])
    assert torch.equal(word_bits(ks.cpu()), word_bits(torch.from_numpy(ws)))       # (zeros past the count on both sides)
    # the same bits on a second call
    keep2, ks2, cnt2 = run_op(ops, case, "soft_linear")
    assert torch.equal(cnt2, cnt) and torch.equal(keep2.cpu()[live], keep.cpu()[live]) and torch.equal(word_bits(ks2), word_bits(ks))


@pytest.mark.parametrize("name", list(OP_CASES))
def test_gaussian_equals_the_restatement_within_the_exp_bound(ops, op_inputs, name):
    case = op_inputs[name]
    wk, ws, wc, gaps = case["want"]["soft_gaussian"]
    for s, (gap, c) in enumerate(zip(gaps, wc)):                        # the condition, on the restatement alone
        assert gap > cases.gaussian_bound(c), f"segment {s}: a pick {gap:.3e} above its runner-up, bound {cases.gaussian_bound(c):.3e}"
    keep, ks, cnt = run_op(ops, case, "soft_gaussian")
    assert torch.equal(cnt.cpu(), torch.from_numpy(wc))
    keep_h, ks_h, off = keep.cpu().numpy(), ks.cpu().numpy(), case["off"]
    differ = 0
    for s, c in enumerate(wc):
        lo, hi = int(off[s]), int(off[s]) + int(c)
        assert np.array_equal(keep_h[lo:hi], wk[lo:hi]), s
        np.testing.assert_allclose(ks_h[lo:hi], ws[lo:hi], rtol=cases.gaussian_bound(c), atol=0)
        assert not ks_h[hi:int(off[s + 1])].any()
        differ += int((ks_h[lo:hi].view(np.uint32) != ws[lo:hi].view(np.uint32)).sum())
    print(f"{name}: {differ} of {int(wc.sum())} Gaussian score words differ in bits from the restatement")
    keep2, ks2, cnt2 = run_op(ops, case, "soft_gaussian")
    assert torch.equal(cnt2, cnt) and torch.equal(word_bits(ks2), word_bits(ks))
    for s, c in enumerate(wc):
        assert torch.equal(keep2[int(off[s]):int(off[s]) + int(c)], keep[int(off[s]):int(off[s]) + int(c)])


def test_kernels_stay_inside_their_operands():
    "As tests/test_guard_gpu.py: every operand at the end of its own device mapping, lengths 65 and 2049, in a child process."
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "guard_probe.py"), "softnms"], capture_output=True, text=True, env=env,
                       timeout=600, cwd=ROOT)
    tail = (r.stdout + r.stderr)[-1500:]
    assert r.returncode == 0, f"probe softnms died (GPU memory access fault?):\n{tail}"
    assert "ok softnms" in r.stdout, tail


# ---- the chain ----------------------------------------------------------------------------------------------------------------------
CHAIN_HW = [(128, 128), (120, 112)]
CHAIN_RW = (1.0, 1.0, 1.0, 1.0)
PLANT = [[300, 150, 70], [40, 260, 100]]              # candidates per (image, class): both kernels, one class under 64
MAX_DET, THR, SCORE_THR, MIN_BOX = 100, 0.5, 0.05, 1e-2
CHAIN_SEED = 18
DTYPES = [torch.float32, torch.bfloat16]


def chain_inputs(seed):
    """B = 2, K = 3 on the 128 x 128 pyramid (A = 3 069).  Every logit is -8 (never a candidate) except the planted ones, which are
    DISTINCT bf16 values in [-2.5, 3) away from zero, so that the scores are distinct in both dtypes; deltas are bf16 values too."""
    rng = np.random.default_rng(seed)
    levels = synth.levels_for(128, 128)
    counts = [h * w * 9 for h, w, _ in levels]
    A, K, B = sum(counts), 3, 2
    vals = (np.arange(1 << 16, dtype=np.uint32) << 16).view(np.float32)
    vals = vals[np.isfinite(vals) & (vals >= -2.5) & (vals < 3.0) & (np.abs(vals) >= 1.0 / 64)]
    cls = np.full((B, A, K), -8.0, np.float32)
    for b in range(B):
        chosen = rng.choice(vals, sum(PLANT[b]), replace=False)
        at = 0
        for k, n in enumerate(PLANT[b]):
            cls[b, rng.choice(A, n, replace=False), k] = chosen[at:at + n]
            at += n
    box = synth.round_bf16((rng.standard_normal((B, A, 4)) * 0.1).astype(np.float32))
    return dict(cls=cls, box=box, counts=counts, levels=levels, A=A, K=K, B=B)


def split_levels(t, counts):
    outs, o = [], 0
    for n in counts:
        outs.append(t[:, o:o + n].contiguous())
        o += n
    return outs


def expected_chain(dump, method):
    """Per image: the restatement per class on the dumped candidates (score order, so index order = score order), then the top MAX_DET
    by (score descending, class, position).  -> rows per image, and the conditions' figures."""
    from pytorch_retinanet_amd.box_utils import soft_nms_reference
    out = []
    for d in dump:
        sc, lb, bx = d["scores"].cpu().numpy(), d["labels"].cpu().numpy(), d["boxes"].cpu().numpy()
        rows, rounds, margin_ok = [], 1, True
        for k in range(int(lb.max())):
            idx = np.nonzero(lb == k + 1)[0]
            m = cases.Margin(bx[idx])
            keep, ks = soft_nms_reference(bx[idx], sc[idx], THR, method, 0.5, 1e-3, MAX_DET, on_pick=m)
            rounds = max(rounds, len(keep))
            margin_ok &= m.gap > (cases.gaussian_bound(len(keep)) if method == "soft_gaussian" else 0.0)
            rows += [(float(ks[j]), k, j, int(idx[keep[j]])) for j in range(len(keep))]
        rows.sort(key=lambda r: (-r[0], r[1], r[2]))
        allsc = np.asarray([r[0] for r in rows], np.float64)
        rel_gap = float(np.min((allsc[:-1] - allsc[1:]) / allsc[:-1]))
        rows = rows[:MAX_DET]
        src = np.asarray([r[3] for r in rows])
        out.append(dict(scores=np.asarray([r[0] for r in rows], np.float32), labels=np.asarray([r[1] + 1 for r in rows], np.int64),
                        boxes=bx[src], rounds=rounds, margin_ok=bool(margin_ok), rel_gap=rel_gap))
    return out


@pytest.fixture(scope="module")
def chain(ops):
    from pytorch_retinanet_amd.anchors import AnchorGenerator
    case = chain_inputs(CHAIN_SEED)
    case["anc"] = ops.anchors_emit(case["levels"], list(AnchorGenerator().to(DEV).cell_anchors), 0.0)
    assert case["anc"].shape[0] == case["A"] == 3069
    return case


def rows_match(got, want, method):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g["labels"].shape[0] == len(w["labels"])
        assert torch.equal(g["labels"].cpu(), torch.from_numpy(w["labels"]))
        assert torch.equal(g["boxes"].cpu(), torch.from_numpy(w["boxes"]))
        if method == "soft_linear":
            assert torch.equal(word_bits(g["scores"].cpu()), word_bits(torch.from_numpy(w["scores"])))
        else:
            np.testing.assert_allclose(g["scores"].cpu().numpy(), w["scores"], rtol=cases.gaussian_bound(w["rounds"]), atol=0)


def same_dets(x, y):
    return len(x) == len(y) and all(torch.equal(a_[k], b_[k]) for a_, b_ in zip(x, y) for k in ("boxes", "scores", "labels"))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_chain_equals_the_restatement_on_its_own_candidates(ops, chain, dtype, method):
    dc, db, anc, counts = dev(chain["cls"], dtype), dev(chain["box"], dtype), chain["anc"], chain["counts"]
    cl, bl = split_levels(dc, counts), split_levels(db, counts)
    # every candidate's score, label and box: the hard chain with a threshold no IoU exceeds
    dump = ops.detect_levels(cl, bl, anc, CHAIN_HW, SCORE_THR, MIN_BOX, 1.0, 1024, CHAIN_RW)
    assert [len(d["scores"]) for d in dump] == [sum(p) for p in PLANT]
    for d, p in zip(dump, PLANT):
        assert [int((d["labels"] == k + 1).sum()) for k in range(3)] == p
    want = expected_chain(dump, method)
    for w in want:                                                       # the conditions, on the expected output alone
        assert w["rel_gap"] > (cases.gaussian_bound(w["rounds"]) if method == "soft_gaussian" else 0.0), "two rows tie in final score"
        assert w["margin_ok"], "a pick too close to its runner-up: choose another CHAIN_SEED"
        assert len(w["scores"]) == MAX_DET and len(set(w["labels"].tolist())) == 3
    kind = dict(nms=method)
    args = (anc, CHAIN_HW, SCORE_THR, MIN_BOX, THR, MAX_DET, CHAIN_RW)
    lev = ops.detect_levels(cl, bl, *args, **kind)
    rows_match(lev, want, method)
    whole = ops.detect(dc, db, *args, **kind)
    assert same_dets(whole, lev)
    assert same_dets(ops.detect_levels(cl, bl, *args, **kind), lev)                        # the same bits on a second call
    # the overflow retry (64 candidates per image are too few) gives the same result
    assert same_dets(ops.detect(dc, db, *args, max_candidates=64, **kind), lev)
    # padded outputs, sizes read on the device: the same rows
    hw_dev = dev(np.asarray(CHAIN_HW, np.int32))
    ob, osc, ol, meta = ops.detect_levels(cl, bl, anc, None, SCORE_THR, MIN_BOX, THR, MAX_DET, CHAIN_RW, max_candidates="all",
                                          image_hw_dev=hw_dev, padded=True, **kind)
    meta = meta.cpu()
    assert not bool(meta[1].any())
    assert same_dets([{"boxes": ob[b, :n], "scores": osc[b, :n], "labels": ol[b, :n]} for b, n in enumerate(meta[0].tolist())], lev)
    # the enqueue-only form (what a graph capture records) runs the same chain
    handle = []
    assert ops.detect_levels([dc], [db], *args, max_candidates="all", enqueue_only=handle, **kind) == []
    handle[0]()
    eb, es, el, em = handle[1][:4]
    em = em.cpu()
    assert same_dets([{"boxes": eb[b, :n], "scores": es[b, :n], "labels": el[b, :n]} for b, n in enumerate(em[0].tolist())], lev)


def raw_chain(ops, name, cl, bl, anc, hw, nms):
    "One raw call of ``rn_detect_levels_kind`` (``nms`` = ...) or ``rn_detect_levels_nms`` (``nms`` = None for NULL, or RnNmsParams)."
    from pytorch_retinanet_amd import _lib
    L, (B, _, K) = len(cl), cl[0].shape
    counts = [int(c.shape[1]) for c in cl]
    A = sum(counts)
    cap = A * K
    params = _lib.RnDetectParams(SCORE_THR, MIN_BOX, THR, MAX_DET, (C.c_float * 4)(*CHAIN_RW))
    out = (torch.empty((B, MAX_DET, 4), device=DEV), torch.empty((B, MAX_DET), device=DEV),
           torch.empty((B, MAX_DET), dtype=torch.int64, device=DEV), torch.empty((2, B), dtype=torch.int32, device=DEV))
    need = _lib.lib.rn_detect_workspace_bytes(B, A, K, cap)
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    arr = lambda ts: (C.c_void_p * L)(*[t.data_ptr() for t in ts])
    head = (arr(cl), arr(bl), (C.c_int64 * L)(*counts), L, ops._dtype_code(cl[0]), B, K, anc.data_ptr(), 0, hw.data_ptr(), C.byref(params), 0)
    tail = (cap, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3][0].data_ptr(), out[3][1].data_ptr(), ws.data_ptr(), need,
            torch.cuda.current_stream().cuda_stream)
    with torch.cuda.device(DEV):
        if name == "rn_detect_levels_kind":
            rc = _lib.lib.rn_detect_levels_kind(*head, *tail)
        else:
            rc = _lib.lib.rn_detect_levels_nms(*head, None if nms is None else C.byref(nms), *tail)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_hard_path_is_untouched(ops, chain, dtype, golden):
    from pytorch_retinanet_amd import _lib
    dc, db, anc, counts = dev(chain["cls"], dtype), dev(chain["box"], dtype), chain["anc"], chain["counts"]
    cl, bl = split_levels(dc, counts), split_levels(db, counts)
    hw = dev(np.asarray(CHAIN_HW, np.int32))
    base = raw_chain(ops, "rn_detect_levels_kind", cl, bl, anc, hw, None)
    n = base[3][0].tolist()
    assert min(n) > 20 and not bool(base[3][1].any())
    for nms in (None, _lib.RnNmsParams(0, 0.5, 1e-3, 0), _lib.RnNmsParams(0, float("nan"), float("inf"), 7)):   # (a hard kind reads nothing else)
        got = raw_chain(ops, "rn_detect_levels_nms", cl, bl, anc, hw, nms)
        assert all(torch.equal(g, b) for g, b in zip(got, base))
    args = (anc, CHAIN_HW, SCORE_THR, MIN_BOX, THR, MAX_DET, CHAIN_RW)
    base_d = [{"boxes": base[0][b, :c], "scores": base[1][b, :c], "labels": base[2][b, :c]} for b, c in enumerate(n)]
    assert same_dets(ops.detect_levels(cl, bl, *args, nms="hard"), base_d)
    assert same_dets(ops.detect_levels(cl, bl, *args), base_d)
    assert same_dets(ops.detect(dc, db, *args, nms="hard", nms_sigma=3.0, nms_min_score=0.5), base_d)
    if dtype == torch.float32:
        # a golden case recorded long before the kinds existed: the default and nms="hard" are what they were
        g = golden("detect.npz")
        toy_hw = [tuple(int(x) for x in r) for r in g["toy_hw"]]
        toy = (dev(g["toy_cls"]), dev(g["toy_box"]), dev(g["toy_anchors"]), toy_hw, 0.05, 1e-2, 0.5, 100)
        plain, named = ops.detect(*toy), ops.detect(*toy, nms="hard")
        assert same_dets(plain, named) and sum(len(d["labels"]) for d in plain) > 0
        for b, d in enumerate(named):
            assert np.array_equal(d["labels"].cpu().numpy(), g[f"toy_labels{b}"])
            np.testing.assert_allclose(d["scores"].cpu().numpy(), g[f"toy_scores{b}"], rtol=1e-6, atol=1e-7)
            np.testing.assert_allclose(d["boxes"].cpu().numpy(), g[f"toy_boxes{b}"], rtol=1e-5, atol=1e-3)


# ---- the model ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e_net(golden):
    g = golden("e2e.npz")
    net = _model(g, DEV, E2E).eval()
    images, _ = _inputs(g, DEV)
    return net, images


def _cpu(dets):
    return [{k: v.detach().cpu().clone() for k, v in d.items()} for d in dets]


def test_predict_with_soft_gaussian(ops, e2e_net):
    """On the SAME head outputs (the conv stack does not repeat bit for bit): at least as many rows as hard NMS, non-increasing scores,
    and every hard-kept detection present with an equal or lower score."""
    from pytorch_retinanet_amd.config import BBOX_REG_WEIGHTS, MIN_BOX_SIZE
    net, images = e2e_net
    assert net.nms == "hard"
    with torch.no_grad():
        il, _ = net.transform(images, None, **net._batch_layout())
        fmaps = net.fpn(net.backbone(il.tensors))
        anchors = net.anchor_generator(il, fmaps)
        out = net.retinanet_head.forward_levels(fmaps)
    per_img, floor, score_thr = net.detections_per_img, net.soft_nms_min_score, net.score_thres
    try:
        # "every hard-kept detection appears" is what the rule gives when nothing cuts the soft list short.  Two things can: a
        # low-scoring hard-kept box under many overlapping picks decays below min_score, and past max_det rows (at most 1024 in the
        # chain) decayed rows fall off the end -- one fixture image has more than 1000 candidates at the default threshold.  So here
        # the floor is 0 (every candidate is emitted), the rows are 1000, and the score threshold is raised to the 901st best score
        # of the fullest image, which keeps every soft list under 1000 rows.
        with torch.no_grad():
            every = torch.cat([c[..., :net.num_classes] for c in out["cls_levels"]], 1).float().sigmoid().flatten(1)
            net.score_thres = max(score_thr, float(every.topk(901, dim=1).values[:, -1].max()))
        net.detections_per_img, net.soft_nms_min_score = 1000, 0.0
        hard = _cpu(net.process_detections_levels(out, anchors, il.image_sizes))
        net.nms = "soft_gaussian"
        soft = _cpu(net.process_detections_levels(out, anchors, il.image_sizes))
        print(f"score threshold {net.score_thres:.4f}; rows per image, hard / soft:", [len(h["scores"]) for h in hard], [len(x["scores"]) for x in soft])
        assert all(len(x["scores"]) < 1000 for x in soft)
        direct = ops.detect_levels(out["cls_levels"], out["bbox_levels"], anchors, il.image_sizes, net.score_thres, MIN_BOX_SIZE,
                                   net.nms_thres, net.detections_per_img, reg_w=BBOX_REG_WEIGHTS, nms="soft_gaussian",
                                   nms_sigma=net.soft_nms_sigma, nms_min_score=net.soft_nms_min_score)
        assert same_dets(soft, _cpu(direct))                                 # the model passes its attributes on
        cat = {"cls_preds": torch.cat([c[..., :net.num_classes] for c in out["cls_levels"]], 1).contiguous(),
               "bbox_preds": torch.cat(list(out["bbox_levels"]), 1).contiguous()}
        assert same_dets(_cpu(net.process_detections(cat, anchors, il.image_sizes)), soft)
        overlapping = 0
        for h, s in zip(hard, soft):
            assert len(s["scores"]) >= len(h["scores"]) > 0
            assert bool((s["scores"][1:] <= s["scores"][:-1]).all())
            overlapping += len(s["scores"]) > len(h["scores"])
            for b, lab, sc in zip(h["boxes"], h["labels"], h["scores"]):
                hit = (s["boxes"] == b).all(1) & (s["labels"] == lab)
                assert int(hit.sum()) >= 1 and float(s["scores"][hit].max()) <= float(sc)
        assert overlapping > 0, "no image with overlapping detections: the comparison is vacuous"
        # predict itself, with the model's defaults
        net.detections_per_img, net.soft_nms_min_score = per_img, floor
        hard = [{k: v[:per_img] for k, v in h.items()} for h in hard]      # (hard NMS at 100 rows is the head of its list at 1000)
        pred = net.predict(images)
        assert len(pred) == len(images)
        for p, h in zip(pred, hard):
            assert len(p["scores"]) >= len(h["scores"]) - max(1, len(h["scores"]) // 100)      # (the e2e bar on counts between two conv passes)
            assert bool((p["scores"][1:] <= p["scores"][:-1]).all())
    finally:
        net.nms, net.detections_per_img, net.soft_nms_min_score, net.score_thres = "hard", per_img, floor, score_thr


def test_captured_predict_follows_the_nms_kind(e2e_net):
    "Flipping ``net.nms`` on a live ``CapturedPredict`` captures a new graph and returns that kind's result; flipping back replays the first."
    from pytorch_retinanet_amd.graph import CapturedPredict
    from test_box_decode_gpu import meets_fp32_bars
    net, images = e2e_net
    try:
        want = {}
        for kind in ("hard", "soft_gaussian"):
            net.nms = kind
            want[kind] = _cpu(net.predict(images))
        assert sum(len(d["scores"]) for d in want["soft_gaussian"]) > sum(len(d["scores"]) for d in want["hard"])
        assert not meets_fp32_bars(want["soft_gaussian"], want["hard"])
        net.nms = "hard"
        p = CapturedPredict(net, [(160, 160)])
        first, second = p(images), p(images)                                      # eager, then capture + replay
        assert p.stats["captures"] == 1 and p.stats["replays"] == 1 and p.stats["fallbacks"] == 0, p.stats
        assert meets_fp32_bars(first, want["hard"]) and meets_fp32_bars(second, want["hard"])
        net.nms = "soft_gaussian"                                                 # flipped between calls
        third, fourth = p(images), p(images)
        assert p.stats["captures"] == 2 and p.stats["replays"] == 2 and p.stats["fallbacks"] == 0 and p.stats["invalidations"] == 0, p.stats
        assert meets_fp32_bars(third, want["soft_gaussian"]) and meets_fp32_bars(fourth, want["soft_gaussian"])
        assert not meets_fp32_bars(fourth, want["hard"])
        net.nms = "hard"                                                          # back: the first graph is still the hard kind's
        fifth = p(images)
        assert p.stats["captures"] == 2 and p.stats["replays"] == 3, p.stats
        assert meets_fp32_bars(fifth, want["hard"]) and not meets_fp32_bars(fifth, want["soft_gaussian"])
    finally:
        net.nms = "hard"
