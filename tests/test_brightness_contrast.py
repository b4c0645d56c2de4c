"""CPU: the host side of ``augment.RandomBrightnessContrast`` -- the draw's restatement against a numpy fp32 one written out here, the
limits and the state, the new ``draw_state`` layout, ``apply_brightness_contrast`` against float64, the PyTorch path of
``net.transform``, and the opt-in hparams mapping."""
import logging

import numpy as np
import pytest
import torch

from pytorch_retinanet_amd import augment, draw_state
from pytorch_retinanet_amd.augment import ColorJitter, RandomBrightnessContrast, apply_brightness_contrast, apply_color_ops, hflip_u

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
F32 = np.float32


def _u(seed, salt, counter, b):
    return F32(hflip_u((seed ^ salt) & (2 ** 64 - 1), counter, b))


def _restate_draw(seed, counter, B, p, brightness, contrast):
    "Steps 1 and 2 in numpy fp32, one rounding per operation, in the written order."
    out = []
    for b in range(B):
        applied = bool(_u(seed, augment.BC_SALT_APPLY, counter, b) < F32(p))
        t = _u(seed, augment.BC_SALT_CONTRAST, counter, b) * F32(F32(contrast[1]) - F32(contrast[0]))
        alpha = F32(F32(1.0) + F32(F32(contrast[0]) + F32(t)))
        t = _u(seed, augment.BC_SALT_BRIGHTNESS, counter, b) * F32(F32(brightness[1]) - F32(brightness[0]))
        beta = F32(F32(brightness[0]) + F32(t))
        out.append((applied, float(alpha), float(beta)))
    return out


# ---- 1. the draw --------------------------------------------------------------------------------------------------------
def test_draw_is_a_pure_function_of_seed_counter_and_image():
    bc = RandomBrightnessContrast(0.3, (-0.1, 0.4), p=0.5, seed=11)
    assert bc.draw(3, 64) == bc.draw(3, 64) == RandomBrightnessContrast(0.3, (-0.1, 0.4), p=0.5, seed=11).draw(3, 64)
    assert bc.draw(3, 64)[:7] == bc.draw(3, 7)                                     # image b's draw does not depend on B
    assert bc.draw(3, 64) != bc.draw(4, 64) and bc.draw(3, 64) != RandomBrightnessContrast(0.3, (-0.1, 0.4), p=0.5, seed=12).draw(3, 64)
    assert bc.draw(0, 5) == RandomBrightnessContrast.draw_coefs(11, 0, 5, 0.5, bc.brightness_limit, bc.contrast_limit)


def test_draw_equals_the_numpy_fp32_restatement_of_step_2():
    for seed, limits in ((0, (0.2, 0.2)), (5, ((-0.3, 0.1), (0.05, 0.7))), (2 ** 63 + 9, (1.0, (-0.9, 3.0)))):
        bc = RandomBrightnessContrast(*limits, p=0.37, seed=seed)
        for counter in (0, 1, 12345678901):
            assert bc.draw(counter, 65) == _restate_draw(seed, counter, 65, F32(0.37), bc.brightness_limit, bc.contrast_limit)


def test_the_three_salts_give_independent_streams_inside_their_ranges():
    salts = (augment.BC_SALT_APPLY, augment.BC_SALT_CONTRAST, augment.BC_SALT_BRIGHTNESS)
    others = (augment.COLOR_SALT_APPLY, augment.COLOR_SALT_ORDER, *augment.COLOR_SALT_FACTOR, augment.CROP_SALT_APPLY, augment.AFFINE_SALT_APPLY,
              augment.SHORT_SIDE_SALT, 0)
    assert len(set(salts) | set(others)) == len(salts) + len(others)               # new salts: no stream of another draw is reused
    rows = [d for k in range(32) for d in RandomBrightnessContrast(0.2, 0.4, p=0.5, seed=3).draw(k, 64)]
    a = np.array([r[0] for r in rows], np.float64)
    alpha, beta = np.array([r[1] for r in rows]), np.array([r[2] for r in rows])
    assert 0.6 <= alpha.min() and alpha.max() <= 1.4 and -0.2 <= beta.min() and beta.max() <= 0.2
    assert alpha.max() - alpha.min() > 0.7 and beta.max() - beta.min() > 0.35      # the whole range is used
    assert 0.45 < a.mean() < 0.55
    for x, y in ((a, alpha), (a, beta), (alpha, beta)):
        assert abs(np.corrcoef(x, y)[0, 1]) < 0.06                                 # 2048 samples: sigma = 0.022


def test_p_0_never_applies_p_1_always_and_both_still_draw_the_coefficients():
    never, always = RandomBrightnessContrast(p=0.0, seed=1), RandomBrightnessContrast(p=1.0, seed=1)
    for k in range(8):
        assert not any(a for a, _, _ in never.draw(k, 64)) and all(a for a, _, _ in always.draw(k, 64))
        assert [r[1:] for r in never.draw(k, 64)] == [r[1:] for r in always.draw(k, 64)]


# ---- 2. limits and state ----------------------------------------------------------------------------------------------------
def test_limits_take_albumentations_scalars_and_pairs_and_are_checked():
    bc = RandomBrightnessContrast()
    assert bc.brightness_limit == bc.contrast_limit == (float(F32(-0.2)), float(F32(0.2)))
    assert bc.p == 0.5 and bc.brightness_by_max is True and bc.seed == 0
    bc = RandomBrightnessContrast(brightness_limit=(0.3, -0.1), contrast_limit=[0.0, 0.5], brightness_by_max=False, p=1)
    assert bc.brightness_limit == (float(F32(-0.1)), float(F32(0.3))) and bc.contrast_limit == (0.0, 0.5) and not bc.brightness_by_max
    for bad in ((0.1, 0.2, 0.3), float("inf"), (0.0, float("nan"))):
        with pytest.raises(ValueError):
            RandomBrightnessContrast(brightness_limit=bad)
        with pytest.raises(ValueError):
            RandomBrightnessContrast(contrast_limit=bad)
    for p in (-0.1, 1.1):
        with pytest.raises(ValueError):
            RandomBrightnessContrast(p=p)
    assert "RandomBrightnessContrast(" in repr(bc) and "brightness_by_max=False" in repr(bc)


def test_state_dict_round_trips_and_set_limits_and_reseed_change_the_draws():
    bc = RandomBrightnessContrast(0.3, 0.1, brightness_by_max=False, p=0.7, seed=9)
    for _ in range(3):
        bc.next_draw(4)
    assert bc.counter == 3 and bc.drawn == bc.draw(2, 4)
    other = RandomBrightnessContrast()
    other.load_state_dict(bc.state_dict())
    assert other.state_dict() == bc.state_dict() and other.next_draw(4) == bc.next_draw(4) and other.counter == 4
    before = bc.draw(7, 16)
    bc.set_limits(contrast_limit=(0.5, 0.5))
    assert bc.brightness_limit == (float(F32(-0.3)), float(F32(0.3)))              # the one not given stays
    assert all(alpha == 1.5 for _, alpha, _ in bc.draw(7, 16)) and [r[2] for r in bc.draw(7, 16)] == [r[2] for r in before]
    bc.set_limits(brightness_limit=0.0)
    assert all(beta == 0.0 for _, _, beta in bc.draw(7, 16))
    bc.p = 0.0
    assert not any(a for a, _, _ in bc.draw(7, 16))
    twin = RandomBrightnessContrast(seed=9)
    twin.set_rank(3)
    assert twin.seed == 12 and twin.draw(0, 8) == RandomBrightnessContrast(seed=12).draw(0, 8)
    bc.brightness_by_max = True                                                    # no device block yet: a plain setting
    assert bc.brightness_by_max is True


def test_the_state_block_layout_round_trips_on_the_cpu():
    lay = draw_state.BRIGHTNESS_CONTRAST
    assert lay.name == "rn_brightness_contrast_state" and lay.nbytes == 40
    assert [(n, f.offset) for n, f in lay.fields.items()] == [("seed", 0), ("counter", 8), ("p", 16), ("brightness", 20), ("contrast", 28), ("by_max", 36)]
    assert lay not in draw_state.LAYOUTS or len(draw_state.LAYOUTS) == 6
    block = draw_state.new(lay, torch.device("cpu"), seed=2 ** 64 - 3, counter=5, p=0.25, brightness=(-0.5, 0.25), contrast=(0.0, 2.0), by_max=False)
    assert block.dtype == torch.uint8 and block.numel() == 40
    assert draw_state.read(lay, block) == (2 ** 64 - 3, 5, 0.25, (-0.5, 0.25), (0.0, 2.0), False)
    raw = block.numpy().tobytes()
    assert np.frombuffer(raw, np.float32, 5, 16).tolist() == [0.25, -0.5, 0.25, 0.0, 2.0] and np.frombuffer(raw, np.int32, 1, 36)[0] == 0
    draw_state.write(lay, block, by_max=True, contrast=(0.5, 1.0))
    assert draw_state.read(lay, block) == (2 ** 64 - 3, 5, 0.25, (-0.5, 0.25), (0.5, 1.0), True)
    with pytest.raises(TypeError):
        draw_state.new(lay, torch.device("cpu"), seed=0, counter=0, p=0.5)
    with pytest.raises(ValueError):
        draw_state.check(lay, torch.zeros(56, dtype=torch.uint8))


# ---- 3. the arithmetic --------------------------------------------------------------------------------------------------------
def _hand_made():
    "[3, 2, 4]: exact 0 and 1, values that clamp at either end under the coefficients below, and ordinary ones."
    return torch.tensor([[[0.0, 1.0, 0.5, 0.25], [0.75, 0.1, 0.9, 0.01]],
                         [[1.0, 0.0, 0.999, 0.3]  , [0.6, 0.05, 0.95, 0.5]],
                         [[0.2, 0.8, 0.001, 1.0], [0.0, 0.45, 0.55, 0.7]]], dtype=torch.float32)


@pytest.mark.parametrize("alpha, beta", [(1.0, 0.0), (1.4, 0.2), (0.6, -0.2), (1.7, -0.5), (0.3, 0.9), (-0.5, 0.4)])
@pytest.mark.parametrize("by_max", [True, False])
def test_apply_equals_a_float64_evaluation(alpha, beta, by_max):
    x = _hand_made()
    ref = 1.0 if by_max else augment.image_mean_of(x)
    if not by_max:
        assert abs(ref - float(x.double().mean())) <= 2.0 ** -24                   # fp32(fp64 mean): half an ulp below 1
    got = apply_brightness_contrast(x, alpha, beta, 1.0 if by_max else None)
    assert got.dtype == torch.float32 and got.shape == x.shape
    want = (float(F32(alpha)) * x.double() + float(F32(beta)) * ref).clamp(0.0, 1.0)
    # three fp32 roundings (beta ref, alpha x, the sum) of magnitudes below 2.5: 3 * 2^-23
    assert float((got.double() - want).abs().max()) <= 3 * 2.0 ** -23
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    if (alpha, beta) in ((1.7, -0.5), (0.6, -0.2)):
        assert bool((got == 0.0).any())                                            # clamps at 0 ...
    if (alpha, beta) == (1.4, 0.2) or ((alpha, beta) == (0.3, 0.9) and by_max):      # (by-mean: 0.3 x + 0.9 * 0.48 stays below 1)
        assert bool((got == 1.0).any())                                            # ... and at 1
    if (alpha, beta) == (1.0, 0.0):
        assert torch.equal(got, x)
    # and the exact fp32 order: one multiply, one add
    add = F32(beta) * F32(ref)
    exact = np.clip((F32(alpha) * x.numpy()).astype(F32) + add, F32(0.0), F32(1.0))
    assert np.array_equal(got.numpy(), exact)
    with pytest.raises(ValueError):
        apply_brightness_contrast(x.double(), alpha, beta)


# ---- 4. the transform module on CPU tensors --------------------------------------------------------------------------------------
SHAPES = [(24, 40), (33, 21), (40, 40), (17, 30)]


def _module():
    from pytorch_retinanet_amd.transform import GeneralizedRCNNTransform
    return GeneralizedRCNNTransform(24, 48, MEAN, STD, size_divisible=32).train()


def _batch(seed=0):
    g = torch.Generator().manual_seed(seed)
    images = [torch.rand((3, h, w), generator=g) for h, w in SHAPES]
    targets = [{"boxes": torch.tensor([[2.0, 3.0, 15.0, 16.0]]), "labels": torch.tensor([1])} for _ in SHAPES]
    return images, targets


@pytest.mark.parametrize("by_max", [True, False])
@pytest.mark.parametrize("with_jitter", [False, True])
def test_module_on_cpu_tensors_draws_and_applies_the_restated_stream(by_max, with_jitter):
    t, plain = _module(), _module()
    bc = t.brightness_contrast = RandomBrightnessContrast(0.3, 0.4, brightness_by_max=by_max, p=0.7, seed=6)
    assert plain.brightness_contrast is None
    cj = ColorJitter(brightness=0.4, contrast=0.4, saturation=0.5, hue=0.1, p=0.8, seed=2) if with_jitter else None
    t.color_jitter = cj
    applied_any = False
    for k in range(3):
        images, targets = _batch(k)
        got, _ = t(images, [dict(x) for x in targets])
        restated = images
        if cj is not None:
            restated = [apply_color_ops(im, fac, order) for im, (fac, order) in zip(restated, cj.draw(k, 4))]      # the jitter first
        draws = bc.draw(k, 4)
        assert bc.drawn == draws and bc.counter == k + 1
        restated = [apply_brightness_contrast(im, a, b_, 1.0 if by_max else None) if on else im for im, (on, a, b_) in zip(restated, draws)]
        applied_any |= any(on for on, _, _ in draws)
        want, _ = plain(restated, [dict(x) for x in targets])
        assert torch.equal(got.tensors, want.tensors), k
    assert applied_any


def test_eval_mode_and_missing_targets_leave_the_image_and_the_counter_alone():
    t, plain = _module(), _module()
    bc = t.brightness_contrast = RandomBrightnessContrast(p=1.0, seed=6)
    images, targets = _batch()
    got, _ = t(images, None)                                                       # training mode, no targets
    want, _ = plain(images, None)
    assert torch.equal(got.tensors, want.tensors)
    t.eval(), plain.eval()
    got, _ = t(images, [dict(x) for x in targets])
    want, _ = plain(images, [dict(x) for x in targets])
    assert torch.equal(got.tensors, want.tensors)
    assert bc.counter == 0 and bc.drawn is None and bc.coef is None


# ---- 5. the hparams ---------------------------------------------------------------------------------------------------------------
DEMO = [{"class_name": "albumentations.HorizontalFlip", "params": {"p": 0.5}},
        {"class_name": "albumentations.ShiftScaleRotate", "params": {"p": 0.5}},
        {"class_name": "albumentations.RandomBrightnessContrast", "params": {"p": 0.5}}]


def test_from_transforms_maps_albumentations_defaults_and_skips_a_second_entry(caplog):
    from pytorch_retinanet_amd.augment import brightness_contrast_from_transforms, from_transforms
    assert brightness_contrast_from_transforms(None) is None and brightness_contrast_from_transforms([{"class_name": "albumentations.HorizontalFlip"}]) is None
    bc = brightness_contrast_from_transforms(DEMO, seed=4)
    ref = RandomBrightnessContrast()
    assert isinstance(bc, RandomBrightnessContrast) and bc.seed == 4
    assert (bc.p, bc.brightness_limit, bc.contrast_limit, bc.brightness_by_max) == (0.5, ref.brightness_limit, ref.contrast_limit, True)
    assert brightness_contrast_from_transforms(["RandomBrightnessContrast"]).state_dict() == ref.state_dict()
    bc = brightness_contrast_from_transforms([{"class_name": "RandomBrightnessContrast", "params": {
        "brightness_limit": [0.0, 0.3], "contrast_limit": 0.1, "brightness_by_max": False, "p": 0.25, "always_apply": True}}])
    assert (bc.p, bc.brightness_limit, bc.brightness_by_max) == (1.0, (0.0, float(F32(0.3))), False)
    assert bc.contrast_limit == (float(F32(-0.1)), float(F32(0.1)))
    with caplog.at_level(logging.WARNING):
        caplog.clear()
        bc = brightness_contrast_from_transforms(DEMO + [{"class_name": "RandomBrightnessContrast", "params": {"p": 0.9}}])
        assert bc.p == 0.5
        msgs = [r.getMessage() for r in caplog.records]
        assert len(msgs) == 1 and "second" in msgs[0] and "RandomBrightnessContrast" in msgs[0] and "skipped" in msgs[0]
        caplog.clear()
        assert from_transforms(DEMO) is not None                                   # without the switch: one warning naming the entry
        msgs = [r.getMessage() for r in caplog.records]
        assert len(msgs) == 1 and "albumentations.RandomBrightnessContrast" in msgs[0] and "skipped" in msgs[0]
        assert "device_brightness_contrast" in msgs[0]
        caplog.clear()
        assert from_transforms(DEMO, brightness_contrast=True).p == 0.5            # with it: the entry is the other mapping's business
        assert not caplog.records


def test_prepare_data_installs_it_only_with_the_switch(tmp_path, caplog):
    import pytorch_retinanet_amd as P
    from test_hflip import _model, _png_csv
    path = _png_csv(tmp_path)
    named = lambda: [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING and "RandomBrightnessContrast" in r.getMessage()]
    with caplog.at_level(logging.WARNING):
        model = _model("csv", path, DEMO)
        assert len(named()) == 1 and "skipped" in named()[0]
        assert model.net.transform.brightness_contrast is None and model.net.transform.hflip is not None
        # the trainer's switch, as fit() hands it to the model before prepare_data
        caplog.clear()
        conf = P.load_hparams()
        conf.model.update(backbone_kind="resnet18", pretrained=False, num_classes=5, min_size=40, max_size=56)
        conf.dataset.kind, conf.dataset.trn_paths, conf.transforms = "csv", path, DEMO + [{"class_name": "RandomBrightnessContrast"}]
        model = P.RetinaNetModel(conf)
        trainer = P.SimpleTrainer(device="cpu", device_brightness_contrast=True)
        assert trainer.resolve_device_brightness_contrast(conf) is True
        model.device_brightness_contrast = True
        model.prepare_data()
        bc = model.net.transform.brightness_contrast
        assert isinstance(bc, RandomBrightnessContrast) and bc.state_dict() == RandomBrightnessContrast().state_dict()
        assert len(named()) == 1 and "second" in named()[0]                        # no warning for the entry itself, one for the second
        assert model.net.transform.hflip is not None and model.net.transform.shift_scale_rotate is not None
        # the hparams' switch
        caplog.clear()
        conf.transforms = DEMO
        conf.trainer = {"device_brightness_contrast": True}
        off = P.SimpleTrainer(device="cpu")
        assert off.device_brightness_contrast is False and off.brightness_contrast is None and off.resolve_device_brightness_contrast(conf) is True
        model = P.RetinaNetModel(conf)
        model.prepare_data()
        assert isinstance(model.net.transform.brightness_contrast, RandomBrightnessContrast) and not named()
        conf.trainer = {}
        assert off.resolve_device_brightness_contrast(conf) is False
        # a model prepared before the switch was known: fit()'s own part installs the mapping
        model = _model("csv", path, DEMO)
        assert model.net.transform.brightness_contrast is None
        trainer._install_brightness_contrast(model)
        model.net.transform.set_rank(2)                                            # (what fit() does as rank 2 of a process group)
        assert trainer.brightness_contrast is model.net.transform.brightness_contrast and trainer.brightness_contrast.seed == 2
    import os
    assert "device_brightness_contrast" in open(os.path.join(os.path.dirname(P.__file__), "hparams.yaml")).read()


def test_the_new_entry_points_are_exported_and_check_their_arguments():
    import ctypes as C
    from pytorch_retinanet_amd import _lib
    lib = _lib.lib
    for name in ("rn_brightness_contrast_draw", "rn_brightness_contrast_mean_workspace_bytes", "rn_brightness_contrast_mean"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    EINVAL, EALIGN = -1, -2
    buf = (C.c_double * 64)()                      # host memory standing in for device pointers: every check precedes the launch
    p = C.addressof(buf)
    assert lib.rn_brightness_contrast_draw(None, 1, p, 1, None) == EINVAL
    assert lib.rn_brightness_contrast_draw(p, 1, None, 1, None) == EINVAL
    assert lib.rn_brightness_contrast_draw(p, 0, p, 1, None) == EINVAL
    assert lib.rn_brightness_contrast_draw(p + 4, 1, p, 0, None) == EALIGN
    ws = lib.rn_brightness_contrast_mean_workspace_bytes
    # the partial sums (what rn_color_mean needs) and f32[B] behind them, rounded up to 8 bytes
    assert ws(0) == 0 and [ws(B) - lib.rn_color_mean_workspace_bytes(B) for B in (1, 2, 3, 65)] == [8, 8, 16, 264]
    ptrs, hw = (C.c_void_p * 1)(p), (C.c_int32 * 2)(2, 2)
    need = ws(1)
    assert lib.rn_brightness_contrast_mean(None, None, None, 0, None, 1, p, p, need, None) == EINVAL        # no images at all
    assert lib.rn_brightness_contrast_mean(ptrs, hw, None, 0, None, 0, p, p, need, None) == EINVAL          # B <= 0
    assert lib.rn_brightness_contrast_mean(ptrs, hw, None, 0, None, 1, None, p, need, None) == EINVAL       # no coef
    assert lib.rn_brightness_contrast_mean(ptrs, hw, None, 0, None, 1, p, p, need - 1, None) == EINVAL      # one byte short
    assert lib.rn_brightness_contrast_mean(ptrs, hw, p, 64, p, 1, p, p, need, None) == EINVAL               # both input forms
    assert lib.rn_brightness_contrast_mean(ptrs, hw, None, 0, None, 1, p, p + 4, need, None) == EALIGN
    assert lib.rn_abi_version() == 10 if hasattr(lib, "rn_abi_version") else True
