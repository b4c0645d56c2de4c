"""GPU: COCO bbox AP on the device -- ``rn_eval_match`` against ``BBoxEval._evaluate_img`` and ``rn_eval_accumulate`` against the numpy
lines of ``BBoxEval.evaluate``, both exact on every bit; ``DeviceBBoxEval`` / ``CocoEvaluator(device=...)`` against ``BBoxEval`` on the
hand-computed protocol fixtures and on seeded scenes with ties, crowds and a pair above 64 ground-truth rows (``np.array_equal`` on
``precision`` and ``recall``); the evaluator flow; and ``SimpleTrainer(device_eval=True).test``.

Equality is the bar everywhere: every floating-point step of ``BBoxEval`` is one double operation on values that started as fp32, and
``csrc/eval.hip`` (built without FMA contraction) does the same operations in the same order."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import eval_scenes as S
from test_device_eval import EV_CHUNK, _cases, case_predictions

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64                                               # elements of tail behind every guarded operand


def _guard(t, fill):
    "``t`` on the device as the leading slice of a larger allocation whose tail is ``fill`` (NaN for floats)."
    t = t.contiguous()
    buf = torch.full((t.numel() + PAD,), fill, dtype=t.dtype, device=DEV)
    buf[:t.numel()] = t.reshape(-1).to(DEV)
    return buf, buf[:t.numel()].view(t.shape)


def _consts():
    from pytorch_retinanet_amd.coco_eval import BBoxEval
    return torch.tensor(BBoxEval.iou_thrs, device=DEV), torch.tensor(np.array(BBoxEval.area_rng), device=DEV)


def _run_match(pair_list):
    """``rn_eval_match`` itself on the pairs of ``pair_list`` ([(rows, xyxy detections sorted)]), every input the leading slice of a
    NaN-tailed allocation and every output inside a sentinel-tailed one -> per pair (matched, ignored, gt_ignored) as numpy."""
    from pytorch_retinanet_amd._lib import check, lib
    xyxy = np.concatenate([d for _, d in pair_list]).reshape(-1, 4).astype(np.float32)
    rows = [r for rs, _ in pair_list for r in rs]
    table, d0, g0 = [], 0, 0
    for rs, d in pair_list:
        table.append([d0, d0 + len(d), g0, g0 + len(rs)])
        d0, g0 = d0 + len(d), g0 + len(rs)
    D, G = d0, g0
    nan = float("nan")
    _, boxes = _guard(torch.from_numpy(xyxy), nan)
    _, gx = _guard(torch.tensor([r[:4] for r in rows], dtype=torch.float64).reshape(-1, 4), nan)
    _, ga = _guard(torch.tensor([r[2] * r[3] for r in rows], dtype=torch.float64), nan)
    _, gc = _guard(torch.tensor([r[4] for r in rows], dtype=torch.uint8), 1)
    _, pairs = _guard(torch.tensor(table, dtype=torch.int32).reshape(-1, 4), 2 ** 30)
    thrs, rng = _consts()
    mbuf, m = _guard(torch.full((D,), -3, dtype=torch.int64), -3)
    ibuf, i = _guard(torch.full((D,), -3, dtype=torch.int64), -3)
    gbuf, gi = _guard(torch.full((G,), 0xEE, dtype=torch.uint8), 0xEE)
    sbuf, st = _guard(torch.full((G,), -1, dtype=torch.int64), -1)                # the scratch starts dirty: it needs no initialisation
    p = lambda t: C.c_void_p(t.data_ptr() if t.numel() else 0)
    check(lib.rn_eval_match(p(boxes), D, p(gx), p(ga), p(gc), G, p(pairs), len(table), p(thrs), 10, p(rng), 4, 100, p(m), p(i), p(gi), p(st),
                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "rn_eval_match")
    torch.cuda.synchronize()
    for buf, n, fill in ((mbuf, D, -3), (ibuf, D, -3), (gbuf, G, 0xEE), (sbuf, G, -1)):
        assert bool((buf[n:] == fill).all()), "a store went past an output"
    m, i, gi = m.cpu().numpy().view(np.uint64), i.cpu().numpy().view(np.uint64), gi.cpu().numpy()
    return [(m[a:b], i[a:b], gi[c:d]) for a, b, c, d in table]


@pytest.fixture(scope="module")
def cases():
    "The hand-made pairs and their reference masks (``BBoxEval._evaluate_img``), computed once."
    out = []
    for name, rows, dets in S.match_cases():
        xyxy, m, i, g = S.match_reference(rows, dets)
        out.append((name, rows, xyxy, m, i, g))
    names = " | ".join(c[0] for c in out)
    for want in ("no ground truth", "no detections", "one ground truth", "63 ", "64 ", "65 ", "130 ", "100 det", "103 det", "identical", "equal scores",
                 "crowd region", "out-of-range", "lower IoU", "exactly 0.5", "zero areas"):
        assert want in names, want
    return out


def test_match_equals_evaluate_img_on_every_case_alone(cases):
    for name, rows, xyxy, m, i, g in cases:
        (gm, gi, gg), = _run_match([(rows, xyxy)])
        assert np.array_equal(gm, m) and np.array_equal(gi, i) and np.array_equal(gg, g), name
    # what two of the cases are there for, read off the reference masks: IoU exactly 0.5 counts at the first threshold only (bit 0 of
    # every area range that holds the detection), and the fourth detection of 103 equal rows past the cut carries nothing
    name, rows, xyxy, m, i, g = [c for c in cases if "exactly 0.5" in c[0]][0]
    assert int(m[0]) & 0x3FF == 1
    name, rows, xyxy, m, i, g = [c for c in cases if c[0] == "103 detections"][0]
    assert len(m) == 103 and not m[100:].any() and not i[100:].any() and m[:100].any()


def test_match_on_all_cases_as_pairs_of_one_launch_twice(cases):
    "Many pairs per launch (several workgroups, a last one with idle waves), empty ranges among them; a second call gives the same bits."
    pair_list = [(rows, xyxy) for _, rows, xyxy, _, _, _ in reversed(cases)]
    first, second = _run_match(pair_list), _run_match(pair_list)
    for (name, _, _, m, i, g), a, b in zip(reversed(cases), first, second):
        assert np.array_equal(a[0], m) and np.array_equal(a[1], i) and np.array_equal(a[2], g), name
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), name


# ---- the accumulation -------------------------------------------------------------------------------------------------------------------
def _accumulate_reference(dtm, dt_ig, npig, ev):
    "The numpy lines of ``BBoxEval.evaluate`` for one (category, area range, maxDets): dtm / dt_ig bool [T, n] in list order."
    T, R = len(ev.iou_thrs), len(ev.rec_thrs)
    precision, recall = -np.ones((T, R)), -np.ones(T)
    eps = np.spacing(1)
    if npig == 0:
        return precision, recall
    tps = np.cumsum(dtm & ~dt_ig, axis=1).astype(np.float64)
    fps = np.cumsum(~dtm & ~dt_ig, axis=1).astype(np.float64)
    for ti in range(T):
        tp, fp = tps[ti], fps[ti]
        nd = len(tp)
        rc = tp / npig
        pr = tp / (fp + tp + eps)
        recall[ti] = rc[-1] if nd else 0.0
        for i in range(nd - 1, 0, -1):
            if pr[i] > pr[i - 1]:
                pr[i - 1] = pr[i]
        q = np.zeros(R)
        inds = np.searchsorted(rc, ev.rec_thrs, side="left")
        ok = inds < nd
        q[ok] = pr[inds[ok]]
        precision[ti] = q
    return precision, recall


def test_accumulate_equals_the_numpy_lines_of_evaluate():
    """Synthetic masks; one category per list length 0, 1, C - 1, C, C + 1, 3 C + 5 for the chunk length C; scores in runs of equal
    values sorted by torch as the evaluator sorts them; a (category, range) with npig == 0; npig above the true positives (a recall
    that never reaches 1) and equal to them (one that does)."""
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.coco_eval import BBoxEval
    ev = BBoxEval([])
    T, A, M = len(ev.iou_thrs), len(ev.area_rng), len(ev.max_dets)
    lengths = [0, 1, EV_CHUNK - 1, EV_CHUNK, EV_CHUNK + 1, 3 * EV_CHUNK + 5]
    K = len(lengths)
    rng = np.random.default_rng(11)
    base = []                                            # per category, in the base order: (score, rank, matched, ignored)
    for n in lengths:
        score = (rng.integers(1, 6, n) / 8.0).astype(np.float32)                 # five values: long runs of equal scores
        rank = rng.integers(0, 100, n).astype(np.int32)
        rank[rng.random(n) < 0.3] = 0
        m = rng.integers(0, 2 ** 40, n, dtype=np.uint64) & rng.integers(0, 2 ** 40, n, dtype=np.uint64)
        i = rng.integers(0, 2 ** 40, n, dtype=np.uint64) & rng.integers(0, 2 ** 40, n, dtype=np.uint64) & rng.integers(0, 2 ** 40, n, dtype=np.uint64)
        base.append((score, rank, m, i))
    # the evaluator's sort: stable, descending, on the device
    order = [torch.sort(torch.from_numpy(b[0]).to(DEV), descending=True, stable=True).indices.cpu().numpy() for b in base]
    for b, o in zip(base, order):
        assert np.array_equal(o, np.argsort(-b[0].astype(np.float64), kind="mergesort"))
    cat = lambda j, dt: np.concatenate([b[j][o] for b, o in zip(base, order)]).astype(dt)
    rank, m, i = cat(1, np.int32), cat(2, np.uint64), cat(3, np.uint64)
    cat_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    bit = lambda v, a, t: ((v >> np.uint64(a * T + t)) & np.uint64(1)).astype(bool)
    npig = np.zeros((K, A), np.int64)
    for k in range(K):
        for a in range(A):
            sl = slice(cat_off[k], cat_off[k + 1])
            tp = max(int((bit(m[sl], a, t) & ~bit(i[sl], a, t)).sum()) for t in range(T))
            npig[k, a] = max(tp, 1) + (3 if (k + a) % 2 else 0)
    npig[2, 1] = npig[5, 3] = 0
    _, dm = _guard(torch.from_numpy(m.view(np.int64)), -1)
    _, di = _guard(torch.from_numpy(i.view(np.int64)), -1)
    _, dr = _guard(torch.from_numpy(rank), 0)
    dev = lambda x: torch.from_numpy(x).to(DEV)
    args = (dm, di, dr, dev(cat_off), dev(npig), dev(ev.rec_thrs), torch.tensor(ev.max_dets, dtype=torch.int32, device=DEV), T)
    precision, recall = (x.cpu().numpy() for x in ops.eval_accumulate(*args))
    again = [x.cpu().numpy() for x in ops.eval_accumulate(*args)]
    assert precision.shape == (T, len(ev.rec_thrs), K, A, M) and recall.shape == (T, K, A, M)
    assert np.array_equal(again[0], precision) and np.array_equal(again[1], recall)
    reached, short = False, False
    for k in range(K):
        sl = slice(cat_off[k], cat_off[k + 1])
        for a in range(A):
            for mi, md in enumerate(ev.max_dets):
                keep = rank[sl] < md
                dtm = np.stack([bit(m[sl], a, t)[keep] for t in range(T)])
                dig = np.stack([bit(i[sl], a, t)[keep] for t in range(T)])
                p, r = _accumulate_reference(dtm, dig, int(npig[k, a]), ev)
                assert np.array_equal(precision[:, :, k, a, mi], p) and np.array_equal(recall[:, k, a, mi], r), (lengths[k], a, md)
                reached |= bool((r == 1.0).any())
                short |= bool(((r > 0) & (r < 1)).any())
    assert reached and short and (recall[:, 2, 1] == -1).all() and (precision[:, :, 5, 3] == -1).all() and (recall[:, 0, 0] == 0).all()


# ---- the evaluators ---------------------------------------------------------------------------------------------------------------------
def _device_evaluator(gt, preds, to=DEV, batches=3):
    from pytorch_retinanet_amd.coco_eval import CocoEvaluator, DeviceBBoxEval
    ev = CocoEvaluator(copy.deepcopy(gt), ["bbox"], device=DEV)
    assert isinstance(ev.coco_eval["bbox"], DeviceBBoxEval)
    S.feed(ev, preds, batches, to=to)
    ev.synchronize_between_processes()
    ev.accumulate()
    ev.summarize(verbose=False)
    return ev


def test_protocol_fixtures():
    from pytorch_retinanet_amd.coco_eval import BBoxEval
    for case in _cases():
        want = BBoxEval(copy.deepcopy(case["gt"]), copy.deepcopy(case["dt"])).evaluate().summarize(verbose=False)
        got = _device_evaluator(case["gt"], case_predictions(case), batches=1).coco_eval["bbox"].stats
        assert np.array_equal(got, want), (case["name"], got, want)
        np.testing.assert_allclose(got, case["stats"], atol=1e-9, err_msg=case["name"])


@pytest.fixture(scope="module")
def scenes():
    "Per seed: (gt, predictions, the host evaluator after summarize) -- computed once, never changed."
    out = {}
    for seed in S.SCENE_SEEDS:
        gt, preds = S.random_scene(seed)
        out[seed] = (gt, preds, S.host_evaluator(gt, preds))
    return out


@pytest.mark.parametrize("seed", S.SCENE_SEEDS)
def test_random_scenes_give_the_hosts_bits(scenes, seed):
    gt, preds, host = scenes[seed]
    h, d = host.coco_eval["bbox"], _device_evaluator(gt, preds).coco_eval["bbox"]
    assert h.eval["precision"].shape == d.eval["precision"].shape
    assert np.array_equal(d.eval["precision"], h.eval["precision"]) and np.array_equal(d.eval["recall"], h.eval["recall"])
    assert np.array_equal(d.stats, h.stats) and (h.eval["recall"] == -1).any() and h.stats[0] > 0


def test_evaluator_flow(scenes):
    from pytorch_retinanet_amd.coco_eval import BBoxEval, prepare_for_coco_detection
    gt, preds, host = scenes[S.SCENE_SEEDS[0]]
    want = host.coco_eval["bbox"]
    on_dev, on_cpu = _device_evaluator(gt, preds, to=DEV), _device_evaluator(gt, preds, to=None)
    for ev in (on_dev, on_cpu):
        assert all(k[0].device.type == "cuda" for k in ev.kept) and not ev.results
        assert np.array_equal(ev.coco_eval["bbox"].stats, want.stats)
    # the rows a multi-rank run would gather are the host path's rows
    assert on_cpu._kept_rows() == host.results
    # a second accumulate(): the same bits
    first = {k: v.copy() for k, v in on_dev.coco_eval["bbox"].eval.items()}
    on_dev.accumulate()
    assert all(np.array_equal(first[k], on_dev.coco_eval["bbox"].eval[k]) for k in first)
    # img_ids that leave an image out are honoured
    left_out = S.IMG_IDS[3]
    on_dev.img_ids = [i for i in on_dev.img_ids if i != left_out]
    on_dev.accumulate()
    on_dev.summarize(verbose=False)
    ref = BBoxEval(copy.deepcopy(gt), prepare_for_coco_detection(preds), img_ids=sorted(set(on_dev.img_ids))).evaluate()
    ref.summarize(verbose=False)
    got = on_dev.coco_eval["bbox"]
    assert np.array_equal(got.eval["precision"], ref.eval["precision"]) and np.array_equal(got.stats, ref.stats)
    assert not np.array_equal(got.eval["precision"], want.eval["precision"])
    # no detections at all: every row with ground truth is 0, the rest -1
    from pytorch_retinanet_amd.coco_eval import CocoEvaluator
    empty = CocoEvaluator(copy.deepcopy(gt), ["bbox"], device=DEV)
    empty.update({S.IMG_IDS[0]: {"boxes": torch.zeros((0, 4)), "scores": torch.zeros((0,)), "labels": torch.zeros((0,), dtype=torch.int64)}})
    empty.accumulate()
    empty.summarize(verbose=False)
    ref = BBoxEval(copy.deepcopy(gt), [], img_ids=[S.IMG_IDS[0]]).evaluate()
    assert np.array_equal(empty.coco_eval["bbox"].eval["precision"], ref.eval["precision"])


# ---- the model --------------------------------------------------------------------------------------------------------------------------
def test_trainer_test_with_device_eval(golden):
    """``SimpleTrainer().test`` with the host evaluator; its stored detections through a device evaluator give the same statistics (a
    second ``test()`` could not be compared exactly: ``net.predict`` does not repeat bit for bit).  Then
    ``SimpleTrainer(device_eval=True).test`` runs, and the model's evaluator is the device one."""
    import pytorch_retinanet_amd as P
    from pytorch_retinanet_amd.coco_eval import BBoxEval, CocoEvaluator, DeviceBBoxEval, gt_from_dataset
    from test_captured_predict_gpu import E2E, _fresh_net
    conf = P.load_hparams()
    conf.model.update(E2E)
    conf.dataset.kind = "synthetic"
    conf.dataset.length, conf.dataset.height, conf.dataset.width = 4, 128, 160
    conf.dataloader.test_bs = 2
    conf.dataloader.args.pin_memory = False
    model = P.RetinaNetModel(conf)
    model.net = _fresh_net(golden)                       # the fixture's weights: the predictions are not empty
    model.prepare_data()
    res, outs = P.SimpleTrainer(device=DEV, precision="32").test(model)
    host = model.test_evaluator
    assert type(host.coco_eval["bbox"]) is BBoxEval and sum(len(d["scores"]) for o in outs for d in o["detections"].values()) > 0
    dev = CocoEvaluator(gt_from_dataset(model.test_ds), ["bbox"], device=DEV)
    for o in outs:
        dev.update(o["detections"])
    dev.accumulate()
    dev.summarize(verbose=False)
    assert np.array_equal(dev.coco_eval["bbox"].stats, host.coco_eval["bbox"].stats)
    assert np.array_equal(dev.coco_eval["bbox"].eval["precision"], host.coco_eval["bbox"].eval["precision"])
    res2, _ = P.SimpleTrainer(device=DEV, precision="32", device_eval=True).test(model)
    assert isinstance(model.test_evaluator.coco_eval["bbox"], DeviceBBoxEval) and model.test_evaluator.device.type == "cuda"
    ap = float(res2["AP"])
    assert ap == -1.0 or 0.0 <= ap <= 1.0
    assert ap == float(model.test_evaluator.coco_eval["bbox"].stats[0])
