"""CPU: the device evaluator's host side -- the two entry points in the ABI table, the argument checks of their wrappers, the
evaluator with ``device=None`` / ``"cpu"`` (today's host path), the ``device_eval`` plumbing of ``SimpleTrainer`` / the hparams, and
the grouping helpers (pair table, base order, per-category lists) against the dict-of-lists grouping of ``BBoxEval.evaluate``.
The kernels themselves are in ``test_device_eval_gpu.py``."""
import copy
import json
import os
import re
from collections import defaultdict

import numpy as np
import pytest
import torch

import eval_scenes as S
from pytorch_retinanet_amd.coco_eval import BBoxEval, CocoEvaluator, DeviceBBoxEval, category_lists, group_pairs, prepare_for_coco_detection

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EV_CHUNK = 64                                          # include/retinanet_hip.h, rn_eval_accumulate: the chunk of the scans


def test_entry_points_are_in_the_abi_table_with_the_headers_arity():
    from pytorch_retinanet_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "retinanet_hip.h")).read(), flags=re.S)
    for name, n in (("rn_eval_match", 18), ("rn_eval_accumulate", 16)):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert decl, name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
        args = [a for a in decl.group(1).split(",") if a.strip()]
        assert len(args) == n == len(_lib.SIGNATURES[name][1]), name
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.lib.rn_version() == 10
    assert "chunks of %d entries" % EV_CHUNK in open(os.path.join(ROOT, "include", "retinanet_hip.h")).read()


def test_entry_points_refuse_bad_arguments_before_any_gpu_call():
    from pytorch_retinanet_amd._lib import lib
    EINVAL, EALIGN = -1, -2
    p = 4096                                            # an aligned non-null "pointer": never dereferenced on these paths
    ok = lambda **kw: lib.rn_eval_match(*[kw.get(k, v) for k, v in (("b", p), ("D", 4), ("x", p), ("ar", p), ("c", p), ("G", 4), ("pairs", p), ("P", 1),
                                                                    ("thr", p), ("T", 10), ("rng", p), ("A", 4), ("md", 100), ("m", p), ("i", p), ("gi", p),
                                                                    ("st", p), ("s", 0))])
    assert ok(T=0) == EINVAL and ok(T=33) == EINVAL and ok(A=9) == EINVAL and ok(T=17, A=4) == EINVAL and ok(md=0) == EINVAL
    assert ok(b=0) == EINVAL and ok(st=0) == EINVAL and ok(pairs=0) == EINVAL and ok(D=-1) == EINVAL and ok(G=2 ** 31) == EINVAL
    assert ok(b=p + 8) == EALIGN and ok(m=p + 4) == EALIGN and ok(pairs=p + 2) == EALIGN
    assert ok(P=0, pairs=0) == 0                        # nothing to do: no launch
    acc = lambda **kw: lib.rn_eval_accumulate(*[kw.get(k, v) for k, v in (("m", p), ("i", p), ("r", p), ("N", 8), ("off", p), ("np", p), ("rec", p), ("R", 101),
                                                                          ("md", p), ("M", 3), ("T", 10), ("K", 2), ("A", 4), ("pr", p), ("rc", p), ("s", 0))])
    assert acc(R=0) == EINVAL and acc(R=1025) == EINVAL and acc(M=0) == EINVAL and acc(K=-1) == EINVAL and acc(N=-1) == EINVAL
    assert acc(m=0) == EINVAL and acc(pr=0) == EINVAL and acc(off=0) == EINVAL and acc(K=2 ** 30) == EINVAL
    assert acc(r=p + 2) == EALIGN and acc(pr=p + 4) == EALIGN
    assert acc(K=0, off=0, np=0, pr=0, rc=0) == 0       # no category: nothing is written


def test_ops_wrappers_check_their_arguments():
    "Wrong dtypes, non-contiguous tensors and mismatched lengths are refused; well-formed CPU tensors reach the no-CPU-fallback error."
    from pytorch_retinanet_amd import ops
    ev = BBoxEval([])
    good = dict(dt_boxes=torch.zeros(3, 4), gt_xywh=torch.zeros(2, 4, dtype=torch.float64), gt_area=torch.zeros(2, dtype=torch.float64),
                gt_crowd=torch.zeros(2, dtype=torch.uint8), pairs=torch.tensor([[0, 3, 0, 2]], dtype=torch.int32),
                iou_thrs=torch.tensor(ev.iou_thrs), area_rng=torch.tensor(np.array(ev.area_rng)))
    for key, bad in (("dt_boxes", torch.zeros(3, 4, dtype=torch.float64)), ("dt_boxes", torch.zeros(4, 3).t()), ("dt_boxes", torch.zeros(3, 5)),
                     ("gt_xywh", torch.zeros(2, 4)), ("gt_xywh", torch.zeros(3, 4, dtype=torch.float64)), ("gt_area", torch.zeros(2)),
                     ("gt_crowd", torch.zeros(2, dtype=torch.bool)), ("gt_crowd", torch.zeros(3, dtype=torch.uint8)),
                     ("pairs", torch.zeros(1, 4, dtype=torch.int64)), ("pairs", torch.zeros(4, 2, dtype=torch.int32).t()),
                     ("iou_thrs", torch.tensor(ev.iou_thrs, dtype=torch.float32)), ("iou_thrs", torch.zeros(33, dtype=torch.float64)),
                     ("area_rng", torch.zeros(9, 2, dtype=torch.float64)), ("area_rng", torch.zeros(4, dtype=torch.float64))):
        with pytest.raises(ValueError):
            ops.eval_match(**{**good, key: bad})
    with pytest.raises(ValueError):
        ops.eval_match(**good, max_det=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.eval_match(**good)
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64)
    good = dict(matched=i64(5), ignored=i64(5), rank=torch.zeros(5, dtype=torch.int32), cat_off=torch.tensor([0, 2, 5]), npig=i64(2, 4),
                rec_thrs=torch.tensor(ev.rec_thrs), max_dets=torch.tensor(ev.max_dets, dtype=torch.int32), T=10)
    for key, bad in (("matched", torch.zeros(5, dtype=torch.int32)), ("ignored", i64(4)), ("ignored", i64(10)[::2]), ("rank", i64(5)),
                     ("cat_off", torch.tensor([0, 2, 5], dtype=torch.int32)), ("npig", i64(3, 4)), ("npig", i64(2, 9)), ("npig", i64(8)),
                     ("rec_thrs", torch.tensor(ev.rec_thrs, dtype=torch.float32)), ("rec_thrs", torch.zeros(1025, dtype=torch.float64)),
                     ("max_dets", torch.tensor(ev.max_dets)), ("T", 17), ("T", 0)):
        with pytest.raises(ValueError):
            ops.eval_accumulate(**{**good, key: bad})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.eval_accumulate(**good)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DeviceBBoxEval([], "cpu")


def _cases():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "coco_protocol_cases.json")))["cases"]


def case_predictions(case):
    """A fixture case's detection rows as ``update``'s input: per image xyxy fp32 boxes whose ``convert_to_xywh`` gives the rows'
    ``bbox`` back exactly (asserted), scores, labels."""
    by_img = defaultdict(list)
    for d in case["dt"]:
        by_img[d["image_id"]].append(d)
    preds = {}
    for img, rows in by_img.items():
        b = torch.tensor([[r["bbox"][0], r["bbox"][1], r["bbox"][0] + r["bbox"][2], r["bbox"][1] + r["bbox"][3]] for r in rows], dtype=torch.float32)
        preds[img] = {"boxes": b, "scores": torch.tensor([r["score"] for r in rows], dtype=torch.float32),
                      "labels": torch.tensor([r["category_id"] for r in rows], dtype=torch.int64)}
    back = prepare_for_coco_detection(preds)
    want = [r for rows in by_img.values() for r in rows]
    assert [r["bbox"] for r in back] == [[float(v) for v in r["bbox"]] for r in want], case["name"]
    return preds


@pytest.mark.parametrize("device", [None, "cpu", torch.device("cpu")])
def test_host_devices_give_bboxevals_stats_on_the_fixture_cases(device):
    for case in _cases():
        want = BBoxEval(copy.deepcopy(case["gt"]), copy.deepcopy(case["dt"])).evaluate().summarize(verbose=False)
        ev = CocoEvaluator(copy.deepcopy(case["gt"]), ["bbox"], device=device)
        assert type(ev.coco_eval["bbox"]) is BBoxEval and ev.device is None
        ev.update(case_predictions(case))
        ev.synchronize_between_processes()
        ev.accumulate()
        ev.summarize(verbose=False)
        got = ev.coco_eval["bbox"].stats
        # the scores went through fp32 here: their ORDER is the rows', so the statistics are the rows' (and the file's)
        assert np.array_equal(got, want), case["name"]
        np.testing.assert_allclose(got, case["stats"], atol=1e-9, err_msg=case["name"])
    with pytest.raises(ValueError):
        CocoEvaluator([], ["segm"], device=device)


def test_trainer_and_hparams_plumbing():
    import pytorch_retinanet_amd as P
    conf = P.load_hparams()
    assert "device_eval" not in (conf.get("trainer") or {})                   # the shipped hparams leave it off
    assert P.SimpleTrainer(device="cpu").device_eval is False and P.SimpleTrainer(device="cpu").resolve_device_eval(conf) is False
    assert P.SimpleTrainer(device="cpu", device_eval=True).resolve_device_eval(conf) is True
    conf2 = copy.deepcopy(conf)
    conf2["trainer"] = dict(conf2.get("trainer") or {}, device_eval=True)
    assert P.SimpleTrainer(device="cpu").resolve_device_eval(conf2) is True
    assert P.SimpleTrainer(device="cpu").resolve_device_eval(None) is False
    # the model: off by default, and on a CPU net the host evaluator whatever the switch says
    conf.model.pretrained = False
    conf.model.backbone_kind = "resnet18"
    conf.dataset.kind = "synthetic"
    conf.dataset.length, conf.dataset.height, conf.dataset.width = 2, 64, 96
    m = P.RetinaNetModel(conf)
    assert m.device_eval is False
    m.prepare_data()
    m.test_dataloader()
    assert type(m.test_evaluator.coco_eval["bbox"]) is BBoxEval and m.test_evaluator.device is None
    m.device_eval = True
    m.test_dataloader()
    assert type(m.test_evaluator.coco_eval["bbox"]) is BBoxEval and m.test_evaluator.device is None


def _rows(preds):
    "(image id, category, score, serial) per detection in ``update`` order, and the same as flat tensors."
    rows = [(img, int(l), float(s)) for img, p in preds.items() for l, s in zip(p["labels"].tolist(), p["scores"].tolist())]
    return rows, (torch.tensor([r[0] for r in rows]), torch.tensor([r[1] for r in rows]), torch.tensor([r[2] for r in rows], dtype=torch.float32))


@pytest.mark.parametrize("drop", [None, S.IMG_IDS[3]])
def test_grouping_helpers_equal_the_dict_of_lists_grouping(drop):
    """Shuffled image ids, an image without detections, one without ground truth, a category that only detections name -- and, with
    ``drop``, an image left out of the evaluated set."""
    gt, preds = S.random_scene(1)
    assert S.IMG_IDS != sorted(S.IMG_IDS) and S.IMG_IDS[1] not in preds and S.IMG_IDS[2] not in {g["image_id"] for g in gt}
    rows, (dimg, dcat, dscore) = _rows(preds)
    assert S.DET_ONLY_CAT in {r[1] for r in rows} and S.DET_ONLY_CAT not in {g["category_id"] for g in gt}
    imgs = sorted(i for i in S.IMG_IDS if i != drop)
    cats = sorted({g["category_id"] for g in gt} | {r[1] for r in rows})
    # the host's grouping (BBoxEval.evaluate), by serial number
    gts, dts = defaultdict(list), defaultdict(list)
    for n, g in enumerate(gt):
        if g["image_id"] in imgs:
            gts[g["image_id"], g["category_id"]].append(n)
    for n, r in enumerate(rows):
        if r[0] in imgs:
            dts[r[0], r[1]].append(n)
    for key in dts:
        dts[key] = sorted(dts[key], key=lambda n: -rows[n][2])                # stable, like ``sorted(d, key=-score)``
    assert any(len({rows[n][2] for n in v}) < len(v) for v in dts.values()), "no equal scores inside a pair: the stable order is untested"
    g = group_pairs(torch.tensor([x["image_id"] for x in gt]), torch.tensor([x["category_id"] for x in gt]), dimg, dcat, dscore,
                    torch.tensor(imgs), torch.tensor(cats))
    want_keys = sorted({(cats.index(c), imgs.index(i)) for i, c in list(gts) + list(dts)})
    assert g.pair_key.tolist() == [k * len(imgs) + i for k, i in want_keys] and g.n_img == len(imgs)
    assert g.pairs.dtype == torch.int32 and g.pairs.shape == (len(want_keys), 4)
    for (k, i), (d0, d1, g0, g1) in zip(want_keys, g.pairs.tolist()):
        key = (imgs[i], cats[k])
        assert g.dt_order[d0:d1].tolist() == dts.get(key, []) and g.gt_order[g0:g1].tolist() == gts.get(key, [])
        assert g.dt_rank[d0:d1].tolist() == list(range(d1 - d0))
    assert g.dt_order.numel() == sum(len(v) for v in dts.values()) and g.gt_order.numel() == sum(len(v) for v in gts.values())
    # the per-category lists: np.argsort(-scores, kind="mergesort") over "image ascending, then rank", for each maxDets
    for cut in (100, 10, 1):
        order, cat_off = category_lists(g, dscore[g.dt_order], len(cats), cut)
        for k, c in enumerate(cats):
            base = [n for i in imgs for n in dts.get((i, c), [])[:cut]]
            sc = np.array([rows[n][2] for n in base])
            want = [base[j] for j in np.argsort(-sc, kind="mergesort")]
            assert g.dt_order[order[cat_off[k]:cat_off[k + 1]]].tolist() == want, (cut, c)
        assert int(cat_off[-1]) == order.numel()
    # a smaller maxDets is the sub-list of the list for 100 (what the kernel relies on)
    order, cat_off = category_lists(g, dscore[g.dt_order], len(cats), 100)
    o10, _ = category_lists(g, dscore[g.dt_order], len(cats), 10)
    assert order[g.dt_rank[order] < 10].tolist() == o10.tolist()


@pytest.mark.parametrize("seed", S.SCENE_SEEDS)
def test_the_random_scenes_exercise_the_hard_branches(seed):
    "Confirmed with ``BBoxEval`` alone, where there is no GPU: the scenes the GPU test compares hold ties, ignored matches and -1 rows."
    props = S.scene_properties(*S.random_scene(seed))
    assert all(props.values()), props
