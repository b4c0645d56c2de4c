"""CPU: the colour jitter's host side -- exports and argument checks of the new entry points, ``augment.ColorJitter``'s ranges, draws
and state, the hparams mapping, and the PyTorch fallback of ``net.transform`` against the restatement below.

The restatement (``restate_*``) is torchvision 0.8's tensor ColorJitter (``transforms.functional_tensor``) written out here in torch
fp32 on the CPU with tensor operands, independent of the package; ``tests/test_color_jitter_gpu.py`` compares the kernels with it."""
import ctypes as C
import itertools
import logging

import numpy as np
import pytest
import torch

OPS = ("brightness", "contrast", "saturation", "hue")
SKIP = 0xF
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


# ---- the restatement ----------------------------------------------------------------------------------------------------
def _t(v):
    return torch.tensor(float(v), dtype=torch.float32)


def restate_gray(x):
    r, g, b = x.unbind(0)
    return _t(0.2989) * r + _t(0.587) * g + _t(0.114) * b


def _clamp(x):
    return torch.minimum(torch.maximum(x, _t(0.0)), _t(1.0))


def restate_mean64(x):
    "The fp64 mean of the fp32 gray values."
    return float(restate_gray(x).to(torch.float64).sum()) / float(x.shape[1] * x.shape[2])


def restate_hue(x, f):
    r, g, b = x.unbind(0)
    one = _t(1.0)
    maxc = torch.maximum(torch.maximum(r, g), b)
    minc = torch.minimum(torch.minimum(r, g), b)
    eq = maxc == minc
    cr = maxc - minc
    s = cr / torch.where(eq, one, maxc)
    d = torch.where(eq, one, cr)
    rc, gc, bc = (maxc - r) / d, (maxc - g) / d, (maxc - b) / d
    h0 = torch.where(maxc == r, bc - gc, torch.where(maxc == g, _t(2.0) + rc - bc, _t(4.0) + gc - rc))
    h = torch.fmod(h0 / _t(6.0) + one, one)
    v = maxc
    h = h + _t(f)
    h = h - torch.floor(h)
    h6 = h * _t(6.0)
    i = torch.floor(h6)
    ff = h6 - i
    i = i.to(torch.int64) % 6
    p = _clamp(v * (one - s))
    q = _clamp(v * (one - s * ff))
    t = _clamp(v * (one - s * (one - ff)))
    table = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)]
    out = torch.zeros_like(x)
    for k, rgb in enumerate(table):
        for c in range(3):
            out[c] = torch.where(i == k, rgb[c], out[c])
    return out


def restate_pre(x, factors, order):
    "The image as it is when the contrast's turn comes (the operations before it), or None when ``order`` holds no contrast."
    for k in range(4):
        op = (order >> (4 * k)) & 0xF
        if op == 1:
            return x
        x = restate_op(x, op, factors, None)
    return None


def restate_op(x, op, factors, mean):
    if op == SKIP:
        return x
    f = _t(factors[op])
    if op == 0:
        return _clamp(x * f)
    if op == 1:
        return _clamp(f * x + (_t(1.0) - f) * _t(mean))
    if op == 2:
        return _clamp(f * x + (_t(1.0) - f) * restate_gray(x)[None])
    return restate_hue(x, factors[3])


def restate(x, factors, order, mean=None):
    """The jittered image.  ``mean``: the contrast's mean when given, else fp32(the fp64 mean of the fp32 gray values of the image
    as it is then)."""
    for k in range(4):
        op = (order >> (4 * k)) & 0xF
        m = mean
        if op == 1 and m is None:
            m = float(np.float32(restate_mean64(x)))
        x = restate_op(x, op, factors, m)
    return x


def order_of(ops):
    "Operation ids in application order -> the nibbles (missing slots 0xF)."
    ops = list(ops) + [SKIP] * (4 - len(ops))
    return sum(op << (4 * k) for k, op in enumerate(ops))


def special_image(h, w, seed=0):
    "Random RGB in [0, 1] with the special pixels first: exact 0 and 1, a gray pixel, saturated primaries."
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((3, h, w), generator=g)
    flat = x.reshape(3, -1)
    special = [(0, 0, 0), (1, 1, 1), (0.5, 0.5, 0.5), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0.25, 0.25, 0.75)]
    for k, px in enumerate(special[:flat.shape[1]]):
        flat[:, k] = torch.tensor(px)
    return x


# ---- 1. the C ABI ---------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_reject_bad_arguments_before_any_launch():
    from pytorch_retinanet_amd import _lib
    lib = _lib.lib
    for name in ("rn_color_jitter_draw", "rn_color_mean_workspace_bytes", "rn_color_mean", "rn_transform_batch_color"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    EINVAL, EALIGN = -1, -2
    assert b"alignment" in lib.rn_status_string(EALIGN)
    buf = (C.c_double * 64)()                      # host memory standing in for device pointers: every check precedes the launch
    p = C.addressof(buf)
    assert lib.rn_color_jitter_draw(None, 1, p, None) == EINVAL
    assert lib.rn_color_jitter_draw(p, 1, None, None) == EINVAL
    assert lib.rn_color_jitter_draw(p, 0, p, None) == EINVAL
    assert lib.rn_color_jitter_draw(p + 4, 1, p, None) == EALIGN
    assert lib.rn_color_mean_workspace_bytes(0) == 0 and lib.rn_color_mean_workspace_bytes(3) == 3 * lib.rn_color_mean_workspace_bytes(1) > 0
    need = lib.rn_color_mean_workspace_bytes(1)
    ptrs, hw = (C.c_void_p * 1)(p), (C.c_int32 * 2)(2, 2)
    assert lib.rn_color_mean(None, None, None, 0, None, 1, p, p, need, None) == EINVAL          # no images at all
    assert lib.rn_color_mean(ptrs, hw, None, 0, None, 0, p, p, need, None) == EINVAL            # B <= 0
    assert lib.rn_color_mean(ptrs, hw, None, 0, None, 1, None, p, need, None) == EINVAL         # no coef
    assert lib.rn_color_mean(ptrs, hw, None, 0, None, 1, p, None, need, None) == EINVAL         # no workspace
    assert lib.rn_color_mean(ptrs, hw, None, 0, None, 1, p, p, need - 1, None) == EINVAL        # one byte short
    assert lib.rn_color_mean(ptrs, hw, p, 64, p, 1, p, p, need, None) == EINVAL                 # both input forms
    assert lib.rn_color_mean(ptrs, hw, None, 0, None, 1, p, p + 4, need, None) == EALIGN
    assert lib.rn_color_mean(None, None, p + 4, 64, p, 1, p, p, need, None) == EALIGN
    mean, std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    args = dict(images=ptrs, in_hw=hw, arena=None, slot=0, in_hw_dev=None, out_hw=hw, out_hw_dev=None, B=1, mean=mean, std=std, Hp=4, Wp=4,
                out=p, dt=0, cl=0, flags=None, coef=p, stream=None)

    def call(**kw):
        return lib.rn_transform_batch_color(*{**args, **kw}.values())
    assert call(coef=None) == EINVAL
    assert call(B=0) == EINVAL
    assert call(out=None) == EINVAL
    assert call(out_hw=None) == EINVAL                                                           # neither host nor device sizes
    assert call(out_hw_dev=p) == EINVAL                                                          # both
    assert call(images=None) == EINVAL
    assert call(images=None, in_hw=None, arena=p, slot=64, in_hw_dev=p) == EINVAL                # staged input needs device sizes
    assert call(coef=p + 2) == EALIGN
    assert call(out=p + 4) == EALIGN


# ---- 2. the object ----------------------------------------------------------------------------------------------------------
def test_constructor_ranges_and_refusals():
    from pytorch_retinanet_amd.augment import ColorJitter
    f32 = lambda v: float(np.float32(v))
    cj = ColorJitter(brightness=0.4, contrast=(0.5, 1.5), saturation=2.0, hue=0.1)
    assert cj.brightness == (f32(0.6), f32(1.4)) and cj.contrast == (0.5, 1.5) and cj.saturation == (0.0, 3.0)
    assert cj.hue == (f32(-0.1), f32(0.1)) and cj.p == 1.0 and cj.enabled_mask == 0xF
    cj = ColorJitter(hue=(-0.5, 0.25))
    assert cj.hue == (-0.5, 0.25) and cj.brightness is None and cj.enabled_mask == 0b1000
    assert ColorJitter().enabled_mask == 0 and ColorJitter(brightness=None, contrast=0, saturation=(1, 1), hue=(0, 0)).enabled_mask == 0
    for kw in ({"brightness": -0.1}, {"hue": 0.6}, {"hue": (-0.6, 0.1)}, {"contrast": (1.5, 0.5)}, {"saturation": (-0.1, 1.0)},
               {"brightness": (1.0,)}, {"p": 1.5}, {"hue": -0.1}):
        with pytest.raises(ValueError):
            ColorJitter(**kw)
    import pytorch_retinanet_amd as P
    t = P.transform.GeneralizedRCNNTransform(32, 64, MEAN, STD)
    keys = set(t.state_dict())
    t.color_jitter = ColorJitter(0.2)
    assert set(t.state_dict()) == keys and not isinstance(t.color_jitter, torch.nn.Module)


def test_draw_is_deterministic_and_differs_by_counter_image_and_seed():
    from pytorch_retinanet_amd.augment import ColorJitter
    a, b = ColorJitter(0.4, 0.4, 0.4, 0.1, seed=5), ColorJitter(0.4, 0.4, 0.4, 0.1, seed=5)
    assert a.draw(3, 6) == b.draw(3, 6) == a.draw(3, 6)
    assert a.draw(3, 6)[:4] == a.draw(3, 4)                                    # image b's draw does not depend on B
    assert a.draw(3, 6) != a.draw(4, 6)
    assert len({d for d in a.draw(3, 6)}) == 6                                 # the images differ
    assert a.draw(3, 6) != ColorJitter(0.4, 0.4, 0.4, 0.1, seed=6).draw(3, 6)
    for fac, order in a.draw(0, 64):
        assert all(float(np.float32(f)) == f for f in fac)                     # fp32 values
        assert np.float32(0.6) <= fac[0] <= np.float32(1.4) and np.float32(-0.1) <= fac[3] <= np.float32(0.1)
        assert sorted((order >> (4 * k)) & 0xF for k in range(4)) == [0, 1, 2, 3] and order >> 16 == 0


def test_p_zero_never_applies_p_one_always_and_all_24_orders_occur():
    from pytorch_retinanet_amd.augment import ColorJitter
    assert all(order == 0xFFFF for k in range(8) for _, order in ColorJitter(0.4, 0.4, 0.4, 0.1, p=0.0, seed=1).draw(k, 64))
    orders = [order for k in range(40) for _, order in ColorJitter(0.4, 0.4, 0.4, 0.1, p=1.0, seed=1).draw(k, 64)]
    want = {order_of(perm) for perm in itertools.permutations(range(4))}
    assert 0xFFFF not in orders and set(orders) == want and len(want) == 24
    counts = np.array([orders.count(o) for o in sorted(want)])
    assert counts.min() > 0.6 * len(orders) / 24 and counts.max() < 1.4 * len(orders) / 24
    half = [order for k in range(40) for _, order in ColorJitter(0.4, p=0.5, seed=2).draw(k, 64)]
    assert 0.4 < sum(o == 0xFFFF for o in half) / len(half) < 0.6
    # the order index is the lexicographic rank
    from pytorch_retinanet_amd.augment import color_order
    assert [color_order(i) for i in range(24)] == [order_of(perm) for perm in sorted(itertools.permutations(range(4)))]


def test_disabled_operations_never_appear_in_the_order():
    from pytorch_retinanet_amd.augment import ColorJitter
    cj = ColorJitter(brightness=0.3, hue=0.2, seed=3)
    seen = set()
    for k in range(20):
        for fac, order in cj.draw(k, 32):
            nib = [(order >> (4 * j)) & 0xF for j in range(4)]
            assert sorted(nib) == [0, 3, SKIP, SKIP]
            assert fac[1] == 1.0 and fac[2] == 1.0                             # a disabled operation's factor is its identity
            seen.add(tuple(n for n in nib if n != SKIP))
    assert seen == {(0, 3), (3, 0)}


def test_state_dict_round_trip_and_host_counter():
    from pytorch_retinanet_amd.augment import ColorJitter
    a = ColorJitter(0.4, (0.8, 1.1), 0, 0.05, p=0.75, seed=11)
    for k in range(3):
        assert a.next_draw(4) == a.draw(k, 4) and a.counter == k + 1
    state = a.state_dict()
    assert state["counter"] == 3 and state["seed"] == 11 and state["p"] == 0.75 and state["saturation"] is None
    b = ColorJitter(seed=1)
    b.load_state_dict(state)
    assert b.state_dict() == state and b.next_draw(5) == a.next_draw(5)
    b.set_rank(2)
    assert b.seed == 3 and b.counter == 4                                      # the constructor's seed + rank, the counter kept
    b.contrast = 0                                                             # without a device block any range may change
    b.saturation = 0.5
    assert b.enabled_mask == 0b1101
    with pytest.raises(RuntimeError, match="GPU"):
        a.next_coef([torch.zeros(3, 2, 2)])


# ---- 3. hparams -------------------------------------------------------------------------------------------------------------
def test_hparams_mapping_and_defaults():
    from pytorch_retinanet_amd.augment import ColorJitter, color_jitter_from_transforms, from_transforms
    f32 = lambda v: float(np.float32(v))
    cj = color_jitter_from_transforms([{"class_name": "albumentations.ColorJitter"}], seed=4)
    assert isinstance(cj, ColorJitter) and cj.p == 0.5 and cj.seed == 4
    assert cj.brightness == cj.contrast == cj.saturation == (f32(0.8), f32(1.2)) and cj.hue == (f32(-0.2), f32(0.2))
    cj = color_jitter_from_transforms([{"class_name": "albumentations.ColorJitter", "params": {"brightness": 0.4, "hue": 0, "always_apply": True}}])
    assert cj.p == 1.0 and cj.brightness == (f32(0.6), f32(1.4)) and cj.hue is None
    for name in ("torchvision.transforms.ColorJitter", "ColorJitter"):
        cj = color_jitter_from_transforms([{"class_name": name, "params": {"contrast": [0.5, 1.5]}}])
        assert cj.p == 1.0 and cj.contrast == (0.5, 1.5) and cj.enabled_mask == 0b0010
    assert color_jitter_from_transforms([{"class_name": "albumentations.HorizontalFlip"}]) is None
    assert color_jitter_from_transforms(None) is None
    assert from_transforms([{"class_name": "albumentations.ColorJitter"}]) is None                # the flip mapping keeps its return value


def test_prepare_data_installs_the_jitter_and_still_warns_about_brightness_contrast(tmp_path, caplog):
    from pytorch_retinanet_amd.augment import ColorJitter
    from test_hflip import _model, _png_csv
    path = _png_csv(tmp_path)
    with caplog.at_level(logging.WARNING):
        model = _model("csv", path, [{"class_name": "albumentations.RandomBrightnessContrast", "params": {"p": 0.2}},
                                     {"class_name": "albumentations.ColorJitter", "params": {"p": 0.3}},
                                     {"class_name": "albumentations.HorizontalFlip", "params": {"p": 0.5}}])
    msgs = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert sum("albumentations.RandomBrightnessContrast" in m for m in msgs) == 1, msgs
    assert not any("albumentations.ColorJitter" in m for m in msgs), msgs      # the jitter's own entry is not warned about
    assert isinstance(model.net.transform.color_jitter, ColorJitter) and model.net.transform.color_jitter.p == float(np.float32(0.3))
    assert model.net.transform.hflip is not None
    assert _model("csv", path).net.transform.color_jitter is None                # the shipped hparams: no colour jitter
    assert _model("synthetic").net.transform.color_jitter is None


# ---- 4. the PyTorch path ----------------------------------------------------------------------------------------------------
def test_package_torch_ops_equal_the_restatement_bit_for_bit():
    from pytorch_retinanet_amd.augment import apply_color_ops
    x = special_image(7, 5, seed=2)
    factors = (1.3, 0.7, 1.6, -0.2)
    for perm in itertools.permutations(range(4)):
        order = order_of(perm)
        assert torch.equal(apply_color_ops(x, factors, order).view(torch.int32), restate(x, factors, order).view(torch.int32)), perm
    for hue in (-0.5, 0.5, -1e-7, 0.0):
        assert torch.equal(apply_color_ops(x, (1, 1, 1, hue), order_of([3])).view(torch.int32),
                           restate(x, (1, 1, 1, hue), order_of([3])).view(torch.int32)), hue
    assert torch.equal(apply_color_ops(x, factors, 0xFFFF), x)
    assert torch.equal(apply_color_ops(x, factors, order_of([1]), mean=0.25), restate(x, factors, order_of([1]), mean=0.25))


def test_fallback_through_the_transform_equals_the_restatement_bit_for_bit():
    from pytorch_retinanet_amd.augment import ColorJitter, RandomHorizontalFlip
    from pytorch_retinanet_amd.transform import GeneralizedRCNNTransform
    shapes = [(24, 40), (33, 21), (40, 40)]
    images = [special_image(h, w, seed=k) for k, (h, w) in enumerate(shapes)]
    targets = [{"boxes": torch.tensor([[2.0, 3.0, 15.0, 17.0]]), "labels": torch.tensor([1])} for _ in shapes]
    t = GeneralizedRCNNTransform(32, 64, MEAN, STD).train()
    t.color_jitter = ColorJitter(0.4, 0.4, 0.4, 0.1, p=0.8, seed=9)
    t.hflip = RandomHorizontalFlip(0.5, seed=9)
    plain = GeneralizedRCNNTransform(32, 64, MEAN, STD).train()
    plain.hflip = RandomHorizontalFlip(0.5, seed=9)
    seen = set()
    for k in range(4):
        got, _ = t(images, [dict(x) for x in targets])
        draws = ColorJitter(0.4, 0.4, 0.4, 0.1, p=0.8, seed=9).draw(k, 3)
        seen |= {order for _, order in draws}
        want, _ = plain([restate(im, fac, order) for im, (fac, order) in zip(images, draws)], [dict(x) for x in targets])
        assert torch.equal(got.tensors.view(torch.int32), want.tensors.view(torch.int32)), k
        assert t.color_jitter.counter == k + 1 and t.color_jitter.drawn == draws
    assert 0xFFFF in seen and len(seen) >= 6
    # eval mode and targets=None: the image and the counter are left alone
    t.hflip = plain.hflip = None
    for train, tg in ((False, targets), (False, None), (True, None)):
        t.train(train), plain.train(train)
        got, _ = t(images, None if tg is None else [dict(x) for x in tg])
        want, _ = plain(images, None)
        assert torch.equal(got.tensors, want.tensors) and t.color_jitter.counter == 4, (train, tg is None)
