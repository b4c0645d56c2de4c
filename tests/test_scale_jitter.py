"""CPU: multi-scale training drawn on the device -- the draw's Python restatement (``augment.RandomShortSide.draw``, what
``rn_short_side_draw`` computes) against an independent numpy version and against ``transform.resize``, the PyTorch path of
``GeneralizedRCNNTransform`` with a jitter installed, and everything that must NOT change when none is."""
import logging
import math

import numpy as np
import pytest
import torch

from pytorch_retinanet_amd.augment import RandomHorizontalFlip, RandomShortSide
from pytorch_retinanet_amd.transform import GeneralizedRCNNTransform

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]

# what the GPU tests (tests/test_scale_jitter_gpu.py) draw from: max_size = 64 caps every draw of the 21 x 90 image and the 48 draw of
# the 37 x 53 one; 64 x 40 and 40 x 64 at 40 and 48 x 48 at 48 keep their size (the transform kernel's one-tap branch)
SHAPES = [(37, 53), (64, 40), (48, 48), (21, 90), (40, 64)]
SIZES, MAX_SIZE, SEED = (24, 32, 40, 48), 64, 2


# ---- 1. the draw ------------------------------------------------------------------------------------------------------
def _numpy_draw(seed, counter, b, h, w, sizes, max_size):
    "rn_short_side_draw for one image: the hash in wrapping uint64, the choice in fp32, the size in float64.  -> (short, nh, nw, rh, rw)"
    with np.errstate(over="ignore"):
        u64 = np.uint64
        z = (u64(seed) ^ u64(0x5CA1E5CA1E5CA1E5)) ^ (u64(counter) * u64(0x9E3779B97F4A7C15)) ^ (u64(b + 1) * u64(0xD1B54A32D192ED03))
        z = (z ^ (z >> u64(30))) * u64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u64(27))) * u64(0x94D049BB133111EB)
        z ^= z >> u64(31)
    u = np.float32(int(z >> u64(40))) * np.float32(2.0 ** -24)
    n = len(sizes)
    idx = min(int(u * np.float32(n)), n - 1)
    short = np.float64(sizes[idx])
    lo, hi = np.float64(min(h, w)), np.float64(max(h, w))
    scale = short / lo
    capped = bool(hi * scale > np.float64(max_size))
    if capped:
        scale = np.float64(max_size) / hi
    ph, pw = np.float64(h) * scale, np.float64(w) * scale
    nh, nw = int(np.floor(ph)), int(np.floor(pw))
    near = any(abs(p - np.rint(p)) <= np.spacing(np.rint(p)) for p in (ph, pw))        # a product within 1 ulp of an integer
    below = any(np.rint(p) - p > 0 and np.rint(p) - p <= np.spacing(np.rint(p)) for p in (ph, pw))
    return (int(short), nh, nw, float(np.float32(nh) / np.float32(h)), float(np.float32(nw) / np.float32(w))), capped, near, below


_DRAW_SHAPES = [(37, 53), (64, 40), (48, 48), (21, 90), (40, 64), (49, 131), (300, 500), (375, 500), (480, 640), (427, 640), (1, 7), (97, 23)]
_DRAW_CASES = [((24, 32, 40, 48), 64), ((480, 512, 544, 576, 608, 640, 672, 704, 736, 768, 800), 1333), ((7,), 9),
               (tuple(range(33, 49)), 50)]


def test_draw_equals_an_independent_numpy_restatement():
    from pytorch_retinanet_amd.transform import _ratios
    cases = capped = near = below = 0
    for sizes, max_size in _DRAW_CASES:
        for seed in (0, 1, SEED, 2 ** 64 - 1, 0x1234_5678_9ABC_DEF0):
            j = RandomShortSide(sizes, seed=seed)
            for counter in (0, 1, 5, 2 ** 33):
                shorts = j.draw_short(counter, len(_DRAW_SHAPES))
                got = j.draw(counter, _DRAW_SHAPES, max_size)
                ratios = j.ratios(_DRAW_SHAPES, got)
                for b, (h, w) in enumerate(_DRAW_SHAPES):
                    want, c, n, bl = _numpy_draw(seed, counter, b, h, w, sizes, max_size)
                    assert (shorts[b], *got[b], *ratios[b]) == want, (sizes, seed, counter, b, h, w)
                    assert ratios[b] == _ratios((h, w), got[b])
                    cases, capped, near, below = cases + 1, capped + c, near + n, below + bl
    # the set holds what it must: a few hundred cases, the max_size cap binding, products within 1 ulp of an integer (some BELOW it, where
    # the floor gives one pixel less than the short side asked for: torchvision's behaviour, which the device must repeat)
    assert cases >= 300 and capped >= 30 and cases - capped >= 30 and near >= 30 and below >= 5, (cases, capped, near, below)


def test_every_drawn_size_is_what_resize_produces():
    seen = set()
    for sizes, max_size in _DRAW_CASES[:1] + _DRAW_CASES[2:]:               # (small images: the interpolation itself runs)
        j = RandomShortSide(sizes, seed=SEED)
        for counter in range(6):
            shorts = j.draw_short(counter, len(_DRAW_SHAPES))
            got = j.draw(counter, _DRAW_SHAPES, max_size)
            for (h, w), s, hw in zip(_DRAW_SHAPES, shorts, got):
                if h * w > 64 * 90 or (h, w, s, max_size) in seen:
                    continue
                seen.add((h, w, s, max_size))
                t = GeneralizedRCNNTransform((s,), max_size, MEAN, STD).train()
                out, _ = t.resize(torch.zeros(3, h, w), None)
                assert tuple(out.shape[-2:]) == hw, (h, w, s, max_size)
    # the 800-class sizes: torch's own output size for the scale factor (what resize's interpolate call computes), without the pixels
    sizes, max_size = _DRAW_CASES[1]
    j = RandomShortSide(sizes, seed=SEED)
    t = GeneralizedRCNNTransform(sizes, max_size, MEAN, STD)
    for counter in range(4):
        for (h, w), s, hw in zip(_DRAW_SHAPES, j.draw_short(counter, len(_DRAW_SHAPES)), j.draw(counter, _DRAW_SHAPES, max_size)):
            scale = t._scale_for(h, w, float(s))
            assert hw == (int(math.floor(h * scale)), int(math.floor(w * scale)))
    assert len(seen) >= 40


def test_the_gpu_tests_seed_gives_varied_draws_and_an_identity_size():
    """A condition on SEED.  "The same size at all 4 counters" is read on the short side drawn: every draw of the 21 x 90 image is cut
    by max_size to 14 x 64 (that is what the image is there for), so its size after the resize cannot vary; the other four must."""
    j = RandomShortSide(SIZES, seed=SEED)
    shorts = [j.draw_short(c, len(SHAPES)) for c in range(4)]
    sizes = [j.draw(c, SHAPES, MAX_SIZE) for c in range(4)]
    assert len({s for row in shorts for s in row}) >= 3, shorts
    for b, hw in enumerate(SHAPES):
        assert len({shorts[c][b] for c in range(4)}) > 1, (b, shorts)
        if hw != (21, 90):
            assert len({sizes[c][b] for c in range(4)}) > 1, (b, sizes)
    assert {sizes[c][3] for c in range(4)} == {(14, 64)}                       # the cap binds
    assert any(sizes[c][b] == SHAPES[b] for c in range(4) for b in range(len(SHAPES))), sizes      # an identity size
    assert len({tuple(row) for row in sizes}) == 4                             # no two steps alike


def test_the_salt_separates_the_jitter_from_a_flip_with_the_same_seed():
    from pytorch_retinanet_amd.augment import hflip_u
    j = RandomShortSide((1, 2), seed=5)
    # without the salt the short side of image b would be 1 exactly where u < 0.5, i.e. where a p = 0.5 flip with seed 5 flips
    tied = [[1 if hflip_u(5, c, b) < 0.5 else 2 for b in range(64)] for c in range(4)]
    assert [j.draw_short(c, 64) for c in range(4)] != tied
    a, b = RandomShortSide(SIZES, seed=0), RandomShortSide(SIZES, seed=1)
    assert a.draw_short(0, 64) != b.draw_short(0, 64) and a.draw_short(0, 64) != a.draw_short(1, 64)
    ranks = [RandomShortSide(SIZES, seed=10) for _ in range(4)]
    for r, f in enumerate(ranks):
        f.set_rank(r)
        assert f.seed == 10 + r and f.base_seed == 10
    assert len({tuple(f.draw_short(0, 64)) for f in ranks}) == 4
    ranks[2].set_rank(2)                                                        # idempotent: base + rank
    assert ranks[2].seed == 12


def test_state_dict_round_trip_and_the_sizes_setter():
    j = RandomShortSide(SIZES, seed=9)
    for _ in range(3):
        j.next_sizes(SHAPES, MAX_SIZE, "cpu")
    sd = j.state_dict()
    assert sd == {"seed": 9, "counter": 3, "sizes": list(SIZES)}
    k = RandomShortSide((48,))
    k.load_state_dict(sd)
    assert k.state_dict() == sd
    got, ratios = k.next_sizes(SHAPES, MAX_SIZE, torch.device("cpu"))
    assert got.dtype == torch.int32 and [tuple(r) for r in got.tolist()] == j.draw(3, SHAPES, MAX_SIZE) and k.sizes_drawn is got
    assert ratios.dtype == torch.float32 and ratios.tolist() == [v for r in j.ratios(SHAPES, j.draw(3, SHAPES, MAX_SIZE)) for v in r]
    j.sizes = (24, 48)                                                          # a smaller set, the same maximum: fine
    j.sizes = (32, 40)                                                          # a smaller maximum: fine, the canvas bound stays
    assert j.sizes == (32, 40) and j.canvas_short == 48 and j.bound(48, 48, MAX_SIZE) == (48, 48)
    with pytest.raises(ValueError, match="canvas"):
        j.sizes = (32, 56)                                                      # a larger maximum: the canvas would change
    assert j.sizes == (32, 40)
    for bad in ((), tuple(range(1, 18)), (0, 8), (8.5,), (True,)):
        with pytest.raises(ValueError):
            RandomShortSide(bad)


# ---- 2. the PyTorch path ----------------------------------------------------------------------------------------------
def _images_and_targets(seed, shapes=SHAPES):
    g = torch.Generator().manual_seed(seed)
    images = [torch.rand((3, h, w), generator=g) for h, w in shapes]
    targets = []
    for n, (h, w) in enumerate(shapes):
        k = 0 if n == 2 else 3                                                  # one image without boxes
        xy = torch.rand(k, 2, generator=g) * torch.tensor([w * 0.5, h * 0.5])
        wh = 2 + torch.rand(k, 2, generator=g) * torch.tensor([w * 0.4, h * 0.4])
        targets.append({"boxes": torch.cat([xy, xy + wh], 1), "labels": torch.arange(1, k + 1)})
    return images, targets


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "with-flip"])
def test_fallback_with_a_jitter_equals_the_per_image_resize_on_the_fixed_canvas(flip):
    images, targets = _images_and_targets(1)
    t = GeneralizedRCNNTransform(SIZES, MAX_SIZE, MEAN, STD).train()
    t.scale_jitter = RandomShortSide(SIZES, seed=SEED)
    if flip:
        t.hflip = RandomHorizontalFlip(0.5, seed=3)
    for counter in range(3):
        shorts = t.scale_jitter.draw_short(counter, len(images))
        want_hw = t.scale_jitter.draw(counter, SHAPES, MAX_SIZE)
        flags = t.hflip.draw(counter, len(images)) if flip else [False] * len(images)
        il, tg = t(images, [dict(x) for x in targets])
        assert t.scale_jitter.counter == counter + 1
        assert [tuple(r) for r in t.scale_jitter.sizes_drawn.tolist()] == want_hw
        # the canvas: every image at the largest short side, rounded up to 32 -- whatever was drawn
        assert tuple(il.tensors.shape) == (len(images), 3, 64, 64)
        assert il.image_sizes == [t.scale_jitter.bound(h, w, MAX_SIZE) for h, w in SHAPES] == [(44, 64), (64, 40), (48, 48), (14, 64), (40, 64)]
        for b, (im, x, s, (nh, nw), f) in enumerate(zip(images, targets, shorts, want_hw, flags)):
            one = GeneralizedRCNNTransform((s,), MAX_SIZE, MEAN, STD).train()     # the ordinary transform of this image at its short side
            if flip:
                one.hflip = RandomHorizontalFlip(1.0 if f else 0.0)
            ref, rt = one([im], [dict(x)])
            assert ref.image_sizes == [(nh, nw)]
            assert torch.equal(il.tensors[b, :, :nh, :nw], ref.tensors[0, :, :nh, :nw])
            assert not il.tensors[b, :, nh:, :].any() and not il.tensors[b, :, :, nw:].any()
            assert torch.equal(tg[b]["boxes"], rt[0]["boxes"]) and torch.equal(tg[b]["labels"], x["labels"])


def test_the_host_side_tuple_draw_is_not_consulted_while_a_jitter_is_installed(monkeypatch):
    images, targets = _images_and_targets(2)
    t = GeneralizedRCNNTransform(SIZES, MAX_SIZE, MEAN, STD).train()
    t.scale_jitter = RandomShortSide(SIZES, seed=SEED)
    monkeypatch.setattr(t, "_target_short_side", lambda: pytest.fail("the host draw was consulted"))
    t(images, [dict(x) for x in targets])
    assert t.scale_jitter.counter == 1


# ---- 3. no side effects -----------------------------------------------------------------------------------------------
def test_eval_mode_and_missing_targets_leave_the_counter_alone():
    images, targets = _images_and_targets(3)
    plain = GeneralizedRCNNTransform(48, MAX_SIZE, MEAN, STD)
    t = GeneralizedRCNNTransform(48, MAX_SIZE, MEAN, STD)
    assert t.scale_jitter is None
    t.scale_jitter = RandomShortSide(SIZES, seed=SEED)
    t.eval(); plain.eval()
    a, ta = t(images, [dict(x) for x in targets])
    b, tb = plain(images, [dict(x) for x in targets])
    assert torch.equal(a.tensors, b.tensors) and a.image_sizes == b.image_sizes
    assert all(torch.equal(x["boxes"], y["boxes"]) for x, y in zip(ta, tb))
    t.train(); plain.train()
    a, _ = t(images, None)
    b, _ = plain(images, None)
    assert torch.equal(a.tensors, b.tensors) and a.image_sizes == b.image_sizes
    assert t.scale_jitter.counter == 0 and t.scale_jitter.sizes_drawn is None


def test_scale_jitter_adds_no_state_dict_key():
    import pytorch_retinanet_amd as P
    net = P.Retinanet(num_classes=5, backbone_kind="resnet18", pretrained=False, min_size=64, max_size=96)
    keys = list(net.state_dict())
    assert net.transform.scale_jitter is None
    net.transform.scale_jitter = RandomShortSide((48, 64))
    assert list(net.state_dict()) == keys


def test_graph_key_is_unchanged_without_a_jitter_and_holds_the_object_with_one():
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from pytorch_retinanet_amd.optim import MasterSGD

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = torch.nn.Conv2d(3, 4, 1)
            self.transform = GeneralizedRCNNTransform(SIZES, MAX_SIZE, MEAN, STD)

    net = Net()
    opt = MasterSGD(net.parameters(), lr=1e-2, momentum=0.9)
    step = CapturedTrainStep(net, opt, amp_dtype=None, enabled=False)
    images = [torch.zeros(3, 16, 16)]
    targets = [{"boxes": torch.zeros(2, 4), "labels": torch.zeros(2, dtype=torch.int64)}]
    none = step._signature(images, targets)
    assert len(none) == 8 and none[-2:] == (None, None)                 # (..., amp dtype, hflip, clip): the key of the parent commit
    a, b = RandomShortSide(SIZES), RandomShortSide(SIZES)
    net.transform.scale_jitter = a
    with_a = step._signature(images, targets)
    assert with_a[:-1] == none and with_a[-1] == ("scale_jitter", a) and with_a[-1][1] is a
    a.sizes = (24, 32)                                                  # the candidates are no part of the key
    a.reseed(7)
    assert step._signature(images, targets) == with_a
    net.transform.scale_jitter = b
    assert step._signature(images, targets) != with_a
    net.transform.scale_jitter = None
    assert step._signature(images, targets) == none


def test_trainer_resolves_the_argument_and_the_hparams_key(caplog):
    import os
    import pytorch_retinanet_amd as P
    conf = P.load_hparams()
    assert "trainer" not in conf                                          # the shipped file keeps the reference's key set
    t = P.SimpleTrainer(device="cpu")
    assert t.device_scale_jitter is False and t.scale_jitter_seed == 0 and t.scale_jitter is None
    assert t.resolve_device_scale_jitter(conf) is False
    assert P.SimpleTrainer(device="cpu", device_scale_jitter=True).resolve_device_scale_jitter(conf) is True
    conf.trainer = {"device_scale_jitter": True}
    assert t.resolve_device_scale_jitter(conf) is True
    conf.trainer = {"gradient_clip_val": 0.5}
    assert t.resolve_device_scale_jitter(conf) is False
    assert "device_scale_jitter" in open(os.path.join(os.path.dirname(P.__file__), "hparams.yaml")).read()

    class Model:
        pass
    model = Model()
    model.conf = {}
    model.net = torch.nn.Module()
    model.net.transform = GeneralizedRCNNTransform(SIZES, MAX_SIZE, MEAN, STD)
    t._install_scale_jitter(model)                                        # off: nothing is installed
    assert model.net.transform.scale_jitter is None and t.scale_jitter is None
    on = P.SimpleTrainer(device="cpu", device_scale_jitter=True, scale_jitter_seed=5)
    on._install_scale_jitter(model)
    model.net.transform.set_rank(3)                                       # (what fit() does as rank 3 of a process group)
    sj = model.net.transform.scale_jitter
    assert isinstance(sj, RandomShortSide) and on.scale_jitter is sj and sj.sizes == SIZES and sj.base_seed == 5 and sj.seed == 8
    model.conf = {"trainer": {"device_scale_jitter": True}}
    model.net.transform = GeneralizedRCNNTransform(48, MAX_SIZE, MEAN, STD)
    with caplog.at_level(logging.INFO, logger="lightning"):
        t._install_scale_jitter(model)                                    # a single-entry min_size: one log line, nothing installed
    assert model.net.transform.scale_jitter is None and t.scale_jitter is None
    assert sum("single entry" in r.getMessage() for r in caplog.records) == 1


def test_new_entry_points_reject_bad_arguments_before_any_gpu_call():
    import ctypes as C
    from pytorch_retinanet_amd._lib import RN_F32, SIGNATURES, lib
    for name in ("rn_short_side_draw", "rn_transform_batch_dev", "rn_gt_flip_scale_many_dev", "rn_gt_flip_scale_packed_dev"):
        assert name in SIGNATURES and getattr(lib, name).argtypes == SIGNATURES[name][1]
    EINVAL, EALIGN = -1, -2
    p = 4096
    hw = lambda *v: (C.c_int32 * len(v))(*v)
    f3 = (C.c_float * 3)(0.5, 0.5, 0.5)
    assert lib.rn_short_side_draw(0, hw(8, 8), 8, 1, p, p, 0) == EINVAL                      # no block
    assert lib.rn_short_side_draw(p, None, 8, 1, p, p, 0) == EINVAL and lib.rn_short_side_draw(p, hw(8, 8), 8, 1, 0, p, 0) == EINVAL
    assert lib.rn_short_side_draw(p, hw(8, 8), 8, 1, p, 0, 0) == EINVAL and lib.rn_short_side_draw(p, hw(8, 8), 8, 0, p, p, 0) == EINVAL
    assert lib.rn_short_side_draw(p, hw(8, 8), 0, 1, p, p, 0) == EINVAL and lib.rn_short_side_draw(p, hw(8, 0), 8, 1, p, p, 0) == EINVAL
    assert lib.rn_short_side_draw(p + 4, hw(8, 8), 8, 1, p, p, 0) == EALIGN and lib.rn_short_side_draw(p, hw(8, 8), 8, 1, p + 2, p, 0) == EALIGN
    one = (C.c_void_p * 1)(p)
    args = lambda out_hw, flags=0: (one, hw(8, 8), 1, f3, f3, 32, 32, p, RN_F32, 0, out_hw, flags, 0)
    assert lib.rn_transform_batch_dev(*args(0)) == EINVAL                                   # no device sizes
    assert lib.rn_transform_batch_dev(*args(p + 2)) == EALIGN
    n1 = (C.c_int64 * 1)(2)
    w1 = (C.c_float * 1)(8.0)
    assert lib.rn_gt_flip_scale_many_dev(one, n1, 1, w1, 0, 0, p, 2, 0) == EINVAL            # no device ratios
    assert lib.rn_gt_flip_scale_many_dev(one, n1, 1, w1, p + 2, 0, p, 2, 0) == EALIGN
    assert lib.rn_gt_flip_scale_many_dev(one, n1, 1, w1, p, 0, p, 1, 0) == EINVAL            # more boxes than rows
    assert lib.rn_gt_flip_scale_packed_dev(p, p + 64, p, w1, 0, 0, 1, 4, 4, 0) == EINVAL
    assert lib.rn_gt_flip_scale_packed_dev(p, p, p, w1, p, 0, 1, 4, 4, 0) == EINVAL          # in place
    assert lib.rn_gt_flip_scale_packed_dev(p, p + 64, p, w1, p + 2, 0, 1, 4, 4, 0) == EALIGN
    assert lib.rn_gt_flip_scale_packed_dev(0, 0, p, w1, p, 0, 1, 0, 4, 0) == 0               # no rows: nothing to do, no launch
    # the host-ratio forms still insist on their flags and ratios
    r2 = (C.c_float * 2)(1.0, 1.0)
    assert lib.rn_gt_flip_scale_many(one, n1, 1, w1, r2, 0, p, 2, 0) == EINVAL
    assert lib.rn_gt_flip_scale_packed(p, p + 64, p, w1, r2, 0, 1, 4, 4, 0) == EINVAL
