"""CPU suite: the host side of global-norm gradient clipping -- ``optim.GradClip``'s fp32 restatement of the coefficient against
``torch.nn.utils.clip_grad_norm_``, argument validation, the capability flag the trainer keys on, ``CapturedTrainStep``'s signature
(the installed object, not its ``max_norm``), and the hparams / ``SimpleTrainer`` wiring.
(The norm kernel, the clipped steps and the captured / exchanged / trainer paths are in test_grad_clip_gpu.py, -m gpu.)"""
import math

import numpy as np
import pytest
import torch


def _grads(seed, scale):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) * scale for n in (1, 7, 64, 1000, 4097)]


@pytest.mark.parametrize("scale", [1e-3, 0.05, 1.0, 30.0, 1e4])
@pytest.mark.parametrize("foreach", [False, True])
def test_coef_equals_clip_grad_norm_bit_for_bit(scale, foreach):
    """norms far below, around and far above max_norm = 2.5: g * coef(total, max_norm) is what clip_grad_norm_ leaves in .grad"""
    from pytorch_retinanet_amd.optim import GradClip
    max_norm = 2.5
    grads = _grads(3, scale)
    params = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads]
    for p, g in zip(params, grads):
        p.grad = g.clone()
    total = torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=foreach)
    c = GradClip.coef(float(total), max_norm)
    assert (c < 1.0) == (scale * math.sqrt(5169) > max_norm)       # (5169 elements of N(0, scale): 0.07 stays below 2.5, 3.6 and up clip)
    for p, g in zip(params, grads):
        assert torch.equal(p.grad, g * torch.tensor(c, dtype=torch.float32))


def test_coef_at_the_threshold_and_for_non_finite_norms():
    from pytorch_retinanet_amd.optim import GradClip
    # exactly at max_norm: torch's own fp32 expression decides, whatever it gives
    for total, max_norm in [(2.5, 2.5), (1.0, 1.0), (0.1, 0.1), (3.0, 1e-3), (1e-3, 3.0), (0.0, 1.0), (1e-7, 1e-7)]:
        t = torch.tensor(total, dtype=torch.float32)
        want = torch.clamp(max_norm / (t + 1e-6), max=1.0)
        got = GradClip.coef(total, max_norm)
        assert np.float32(got).tobytes() == want.numpy().tobytes(), (total, max_norm, got, float(want))
    assert GradClip.coef(float("inf"), 1.0) == 0.0
    assert math.isnan(GradClip.coef(float("nan"), 1.0))
    # and through clip_grad_norm_ itself
    for bad in (float("inf"), float("nan")):
        p = torch.nn.Parameter(torch.zeros(4))
        p.grad = torch.tensor([1.0, bad, -2.0, 0.5])
        total = torch.nn.utils.clip_grad_norm_([p], 1.0)
        c = GradClip.coef(float(total), 1.0)
        want = torch.tensor([1.0, bad, -2.0, 0.5]) * torch.tensor(c, dtype=torch.float32)
        assert p.grad.numpy().tobytes() == want.numpy().tobytes()


def test_argument_validation():
    from pytorch_retinanet_amd.optim import GradClip, MasterAdamW, MasterSGD
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError, match="max_norm"):
            GradClip(bad)
    for bad in (1.0, float("inf"), 0.0):
        with pytest.raises(ValueError, match="norm_type"):
            GradClip(1.0, norm_type=bad)
    c = GradClip(2.0)
    assert c.max_norm == 2.0 and GradClip(1, norm_type=2).max_norm == 1.0
    c.max_norm = 0.5                                    # (no device block yet: only the host value changes)
    assert c.max_norm == 0.5 and "0.5" in repr(c)
    with pytest.raises(ValueError, match="max_norm"):
        c.max_norm = 0.0
    assert c.max_norm == 0.5
    assert c.stats() == {"calls": 0, "clipped": 0, "nonfinite": 0}
    with pytest.raises(RuntimeError, match="no step"):
        c.total_norm
    net = torch.nn.Conv2d(3, 4, 1)
    with pytest.raises(ValueError, match="max_norm"):
        MasterSGD(net.parameters(), lr=0.1, max_grad_norm=-1.0)
    with pytest.raises(ValueError, match="max_norm"):
        MasterAdamW(net.parameters(), max_grad_norm=0.0)


def test_capability_flag_and_constructor_keyword():
    from pytorch_retinanet_amd.optim import GradClip, MasterAdam, MasterAdamW, MasterSGD
    net = torch.nn.Conv2d(3, 4, 1)
    for cls in (MasterSGD, MasterAdam, MasterAdamW):
        assert cls._rn_grad_clip is True
        opt = cls(net.parameters(), lr=1e-3)
        assert opt.grad_clip is None
        opt = cls(net.parameters(), lr=1e-3, max_grad_norm=3.0)
        assert isinstance(opt.grad_clip, GradClip) and opt.grad_clip.max_norm == 3.0
        assert "max_grad_norm" not in opt.defaults and "max_grad_norm" not in opt.param_groups[0]      # (no part of a checkpoint)
    for cls in (torch.optim.SGD, torch.optim.AdamW):
        assert not getattr(cls, "_rn_grad_clip", False)


def test_clipped_step_refuses_cpu_parameters_like_the_plain_one():
    from pytorch_retinanet_amd.optim import MasterSGD
    net = torch.nn.Conv2d(3, 4, 1)
    opt = MasterSGD(net.parameters(), lr=0.1, max_grad_norm=1.0)
    net(torch.rand(1, 3, 2, 2)).sum().backward()
    with pytest.raises(TypeError, match="CUDA"):
        opt.step()


def _signature_of(opt, net):
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16)
    images = [torch.zeros(3, 16, 16)]
    targets = [{"boxes": torch.zeros(2, 4), "labels": torch.zeros(2, dtype=torch.int64)}]
    return lambda: step._signature(images, targets)


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_signature_keys_the_installed_clip_not_its_max_norm(kind):
    from pytorch_retinanet_amd.optim import GradClip, MasterAdamW, MasterSGD
    net = torch.nn.Conv2d(3, 4, 1)
    opt = MasterSGD(net.parameters(), lr=1e-2, momentum=0.9) if kind == "sgd" else MasterAdamW(net.parameters(), lr=1e-3)
    sig = _signature_of(opt, net)
    none = sig()
    a, b = GradClip(1.0), GradClip(1.0)
    opt.grad_clip = a
    with_a = sig()
    opt.grad_clip = b
    with_b = sig()
    assert len({none, with_a, with_b}) == 3
    opt.grad_clip = a
    a.max_norm = 0.25
    assert sig() == with_a
    opt.grad_clip = None
    assert sig() == none


def _conf():
    import pytorch_retinanet_amd as P
    conf = P.load_hparams()
    conf.model.update(backbone_kind="resnet18", pretrained=False, num_classes=5, min_size=128, max_size=160)
    return conf


def test_hparams_max_grad_norm_reaches_the_optimizer():
    import pytorch_retinanet_amd as P
    from pytorch_retinanet_amd.optim import GradClip, MasterAdamW, MasterSGD
    for name, cls, params in (("MasterSGD", MasterSGD, {"lr": 1e-3, "momentum": 0.9, "max_grad_norm": 0.75}),
                              ("MasterAdamW", MasterAdamW, {"lr": 1e-4, "max_grad_norm": 0.75})):
        conf = _conf()
        conf.optimizer.class_name = "pytorch_retinanet_amd.optim." + name
        conf.optimizer.params = params
        conf.scheduler.class_name = None
        opt = P.RetinaNetModel(conf).configure_optimizers()[0]
        assert isinstance(opt, cls) and isinstance(opt.grad_clip, GradClip) and opt.grad_clip.max_norm == 0.75


def test_trainer_takes_gradient_clip_val_from_its_argument_or_the_hparams():
    import pytorch_retinanet_amd as P
    conf = _conf()
    assert "trainer" not in conf                                          # the shipped file keeps the reference's key set
    t = P.SimpleTrainer(device="cpu")
    assert t.gradient_clip_val == 0.0 and t.resolve_gradient_clip_val(conf) == 0.0 and t.grad_clip is None
    assert P.SimpleTrainer(device="cpu", gradient_clip_val=1.5).resolve_gradient_clip_val(conf) == 1.5
    conf.trainer = {"gradient_clip_val": 0.3}
    assert t.resolve_gradient_clip_val(conf) == 0.3
    assert P.SimpleTrainer(device="cpu", gradient_clip_val=1.5).resolve_gradient_clip_val(conf) == 1.5      # the argument wins
    conf.trainer = {"max_epochs": 3}
    assert t.resolve_gradient_clip_val(conf) == 0.0
    conf.trainer = {"gradient_clip_val": -1.0}
    with pytest.raises(ValueError, match="gradient_clip_val"):
        t.resolve_gradient_clip_val(conf)
    with pytest.raises(ValueError, match="gradient_clip_val"):
        P.SimpleTrainer(device="cpu", gradient_clip_val=-0.5)


def test_shipped_hparams_mention_the_optional_block_in_a_comment_only():
    import os
    import pytorch_retinanet_amd as P
    path = os.path.join(os.path.dirname(P.__file__), "hparams.yaml")
    text = open(path).read()
    assert "gradient_clip_val" in text and "max_grad_norm" in text
    conf = P.load_hparams()
    assert set(conf) == {"model", "dataset", "dataloader", "transforms", "optimizer", "scheduler"}
    assert "max_grad_norm" not in conf.optimizer.params
    opt = P.RetinaNetModel(_conf()).configure_optimizers()[0][0]
    assert isinstance(opt, torch.optim.SGD) and not hasattr(opt, "grad_clip")


def test_new_entry_points_reject_bad_arguments_before_any_gpu_call():
    import ctypes as C
    from pytorch_retinanet_amd._lib import RN_BF16, lib
    EINVAL, EALIGN, EUNSUP = -1, -2, -4
    p = 4096
    assert lib.rn_grad_clip_set(0, 1.0, 0) == EINVAL
    assert lib.rn_grad_clip_set(p, 0.0, 0) == EINVAL and lib.rn_grad_clip_set(p, float("nan"), 0) == EINVAL
    assert lib.rn_grad_clip_set(p + 4, 1.0, 0) == EALIGN
    one = lambda v: (C.c_void_p * 1)(v)
    n1 = lambda v: (C.c_int64 * 1)(v)
    assert lib.rn_grad_norm_clip(one(p), one(0), n1(100), 1, 1, 7, None, p, 1, p, 0) == EUNSUP
    assert lib.rn_grad_norm_clip(one(p), one(0), n1(100), 1, 1, RN_BF16, None, 0, 1, p, 0) == EINVAL          # no scratch
    assert lib.rn_grad_norm_clip(one(0), one(0), n1(100), 1, 1, RN_BF16, None, p, 1, p, 0) == EINVAL          # a null gradient
    assert lib.rn_grad_norm_clip(one(p), one(0), n1(40000), 1, 1, RN_BF16, None, p, 2, p, 0) == EINVAL        # 3 chunks, 2 slots
    assert lib.rn_grad_norm_clip(one(p + 8), one(0), n1(100), 1, 1, RN_BF16, None, p, 1, p, 0) == EALIGN      # fp32 gradient: 16 bytes
    assert lib.rn_grad_norm_clip(one(p + 4), one(p), n1(100), 1, 1, RN_BF16, None, p, 1, p, 0) == EALIGN      # 16-bit gradient: 8 bytes


def test_step_entry_points_reject_bad_arguments_before_any_gpu_call():
    """``rn_sgd_master_step`` / ``rn_adam_master_step`` (the only two step entry points; a null ``clip_coef`` is the unclipped step):
    every tensor is checked before the first launch, so no case below touches a device."""
    import ctypes as C
    from pytorch_retinanet_amd._lib import RN_BF16, lib
    EINVAL, EALIGN, EUNSUP = -1, -2, -4
    p = 4096
    arr = lambda vs: (C.c_void_p * len(vs))(*vs)
    num = lambda vs: (C.c_int64 * len(vs))(*vs)

    def sgd(masters, moms, grads, p16s, ns, n=None, grads16=1, dt=RN_BF16, momentum=0.9):
        a = [arr(v) if v is not None else None for v in (masters, moms, grads, p16s)]
        return lib.rn_sgd_master_step(*a, num(ns) if ns is not None else None, len(ns) if n is None else n, grads16, dt, 0.1, momentum, 0.0,
                                      1e-3, 0, 1, None, None, None, 0)

    def adam(masters, ms, vs, grads, p16s, ns, n=None, grads16=1, dt=RN_BF16, hp=p):
        a = [arr(v) if v is not None else None for v in (masters, ms, vs, grads, p16s)]
        return lib.rn_adam_master_step(*a, num(ns) if ns is not None else None, len(ns) if n is None else n, grads16, dt, 1, hp, None, None, None, 0)

    # -- SGD
    assert sgd([p], [p], [p], [0], [100], dt=7) == EUNSUP                          # a bad dtype16
    for hole in range(5):                                                          # null tables
        t = [[p], [p], [p], [0], [100]]
        t[hole] = None
        assert sgd(*t, n=1) == EINVAL
    assert sgd([p], [p], [p], [0], [100], n=-1) == EINVAL
    assert sgd([0], [p], [p], [0], [100]) == EINVAL                                # a null master
    assert sgd([p], [p], [0], [0], [100]) == EINVAL                                # a null gradient
    assert sgd([p], [0], [p], [0], [100]) == EINVAL                                # a null momentum buffer with momentum != 0
    assert sgd([p], [p], [p], [0], [-1]) == EINVAL                                 # a negative numel
    assert sgd([p + 8], [p], [p], [0], [100]) == EALIGN                            # master: 16 bytes
    assert sgd([p], [p + 8], [p], [0], [100]) == EALIGN                            # momentum buffer: 16 bytes
    assert sgd([p], [p], [p + 8], [0], [100]) == EALIGN                            # fp32 gradient: 16 bytes
    assert sgd([p], [p], [p + 8], [p], [100]) == EALIGN                            # 16-bit gradient: 16 bytes too (parallel.py's views)
    assert sgd([p], [p], [p], [p + 4], [100]) == EALIGN                            # the 16-bit copy: 8 bytes
    assert sgd([p], [p], [p], [0], [100], n=0) == 0                                # nothing to do: no launch
    # the first 48 tensors (one launch) are valid, the 49th is not: the error comes back and nothing has been launched
    good = [p] * 48
    assert sgd(good + [0], good + [p], good + [p], [0] * 49, [0] * 49) == EINVAL
    assert sgd(good + [p + 8], good + [p], good + [p], [0] * 49, [0] * 49) == EALIGN
    assert sgd(good + [p], good + [p], good + [p], [0] * 49, [0] * 48 + [-1]) == EINVAL
    # -- Adam / AdamW
    assert adam([p], [p], [p], [p], [0], [100], dt=7) == EUNSUP
    for hole in range(6):
        t = [[p], [p], [p], [p], [0], [100]]
        t[hole] = None
        assert adam(*t, n=1) == EINVAL
    assert adam([p], [p], [p], [p], [0], [100], hp=0) == EINVAL and adam([p], [p], [p], [p], [0], [100], hp=p + 4) == EALIGN
    assert adam([p], [p], [p], [p], [0], [100], n=-1) == EINVAL
    assert adam([0], [p], [p], [p], [0], [100]) == EINVAL                          # a null master
    assert adam([p], [0], [p], [p], [0], [100]) == EINVAL and adam([p], [p], [0], [p], [0], [100]) == EINVAL       # a null moment
    assert adam([p], [p], [p], [0], [0], [100]) == EINVAL                          # a null gradient
    assert adam([p], [p], [p], [p], [0], [-1]) == EINVAL
    assert adam([p + 8], [p], [p], [p], [0], [100]) == EALIGN                      # master: 16 bytes
    assert adam([p], [p + 8], [p], [p], [0], [100]) == EALIGN and adam([p], [p], [p + 8], [p], [0], [100]) == EALIGN
    assert adam([p], [p], [p], [p + 8], [0], [100]) == EALIGN                      # fp32 gradient: 16 bytes
    assert adam([p], [p], [p], [p + 4], [p], [100]) == EALIGN                      # 16-bit gradient: 8 bytes
    assert adam([p], [p], [p], [p], [p + 4], [100]) == EALIGN                      # the 16-bit copy: 8 bytes
    good = [p] * 40
    assert adam(good + [0], good + [p], good + [p], good + [p], [0] * 41, [0] * 41) == EINVAL
