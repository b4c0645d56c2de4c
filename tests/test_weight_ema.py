"""CPU suite: the host side of the weight average -- the four entry points in the ABI table and their argument checks,
``optim.WeightEMA``'s argument validation, the pure-Python restatement of the update factor against hand-computed values, the
hparams resolution of ``SimpleTrainer(weight_ema_decay=, weight_ema_warmup=)``, ``CapturedTrainStep``'s signature (unchanged without
an average; the installed object with one) and the trainer's refusal of an optimizer that cannot keep one.
(The kernels, the skip, the swap, the captured step and the trainer's device path are in test_weight_ema_gpu.py, -m gpu.)"""
import ctypes as C

import numpy as np
import pytest
import torch


def test_the_four_entry_points_are_in_the_abi_table():
    from pytorch_retinanet_amd._lib import SIGNATURES, lib
    for name in ("rn_ema_set", "rn_ema_update", "rn_ema_advance", "rn_ema_swap"):
        assert name in SIGNATURES and SIGNATURES[name][0] is C.c_int
        assert getattr(lib, name).argtypes == SIGNATURES[name][1]
    assert len(SIGNATURES["rn_ema_set"][1]) == 5 and len(SIGNATURES["rn_ema_update"][1]) == 7
    assert len(SIGNATURES["rn_ema_advance"][1]) == 3 and len(SIGNATURES["rn_ema_swap"][1]) == 7


def test_weight_ema_argument_validation():
    from pytorch_retinanet_amd.optim import WeightEMA
    for bad in (1, 1.0, 1.5, -0.1, -1, float("nan")):
        with pytest.raises(ValueError, match="decay must be in"):
            WeightEMA(bad)
    for bad in (-1, -1e-9, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="warmup"):
            WeightEMA(0.99, bad)
    e = WeightEMA()
    assert e.decay == 0.9998 and e.warmup == 0.0 and "0.9998" in repr(e)
    assert WeightEMA(0).decay == 0.0 and WeightEMA(0.5, 10).warmup == 10.0
    e.decay = 0.5                                          # (no device block yet: only the host values change)
    e.warmup = 3
    assert (e.decay, e.warmup) == (0.5, 3.0)
    with pytest.raises(ValueError, match="decay must be in"):
        e.decay = 1.0
    with pytest.raises(ValueError, match="warmup"):
        e.warmup = -2
    assert (e.decay, e.warmup) == (0.5, 3.0)
    assert e.updates == 0 and e.stats() == {"updates": 0, "skipped": 0} and not e.is_swapped and not e.ready and e.parameters() == []
    assert e.update([]) == 0                               # nothing to do, no device needed
    with pytest.raises(RuntimeError, match="nothing to swap"):
        e.swap([])
    with pytest.raises(RuntimeError, match="no update"):
        e.next_factor
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        e.update([torch.nn.Parameter(torch.zeros(3))])
    sd = e.state_dict()
    assert sd == {"decay": 0.5, "warmup": 3.0, "updates": 0, "ema": []}


def test_one_minus_decay_against_hand_computed_values():
    """warmup = 10, decay = 0.9998: d_t = min(0.9998, (1 + t) / (10 + t)) = 1/10, 2/11, 10/19 for t = 0, 1, 9 -- so 1 - d_t = 9/10, 9/11,
    9/19 -- and 0.9998 at t = 10**6 ((10**6 + 1) / (10**6 + 10) = 0.999991...); without a warm-up 1 - decay at every t."""
    from pytorch_retinanet_amd.optim import WeightEMA
    om = WeightEMA.one_minus_decay
    assert om(0, 0.9998, 10) == np.float32(0.9)
    assert om(1, 0.9998, 10) == np.float32(0.8181818181818182)
    assert om(9, 0.9998, 10) == np.float32(0.47368421052631576)
    assert om(10 ** 6, 0.9998, 10) == np.float32(0.0002)
    for t in (0, 1, 9, 10 ** 6):
        assert om(t, 0.9998, 0) == np.float32(0.0002) and om(t, 0.9998, 0.0).dtype == np.float32
        assert om(t, 0.5, 0) == np.float32(0.5) and om(t, 0.0, 0) == np.float32(1.0)
    assert om(3, 0.25, 10) == np.float32(0.75)             # (1 + 3) / (10 + 3) > 0.25: the decay itself
    assert om(0, 0.9998, 2) == np.float32(0.5)             # (1 + 0) / (2 + 0)
    assert om(0, 0.9998) == np.float32(0.0002)             # warmup defaults to 0


def test_one_minus_decay_warmup_one_is_the_decay():
    from pytorch_retinanet_amd.optim import WeightEMA
    # (1 + t) / (1 + t) = 1 >= decay at every t: min() picks the decay
    assert WeightEMA.one_minus_decay(0, 0.9, 1) == np.float32(1.0 - 0.9)


def test_trainer_options_and_hparams_resolution():
    import pytorch_retinanet_amd as P
    conf = P.load_hparams()
    assert "trainer" not in conf                           # the shipped file keeps the reference's key set
    t = P.SimpleTrainer(device="cpu")
    assert t.weight_ema_decay == 0.0 and t.weight_ema_warmup == 0.0 and t.weight_ema is None
    assert t.resolve_weight_ema_decay(conf) == 0.0 and t.resolve_weight_ema_warmup(conf) == 0.0        # absent: off
    mine = P.SimpleTrainer(device="cpu", weight_ema_decay=0.99, weight_ema_warmup=10)
    assert mine.resolve_weight_ema_decay(conf) == 0.99 and mine.resolve_weight_ema_warmup(conf) == 10.0
    for bad in (1.0, -0.5, 2):
        with pytest.raises(ValueError, match="weight_ema_decay must be in"):
            P.SimpleTrainer(device="cpu", weight_ema_decay=bad)
    with pytest.raises(ValueError, match="weight_ema_warmup"):
        P.SimpleTrainer(device="cpu", weight_ema_warmup=-1)
    conf.trainer = {"weight_ema_decay": 0.999, "weight_ema_warmup": 5}
    assert t.resolve_weight_ema_decay(conf) == 0.999 and t.resolve_weight_ema_warmup(conf) == 5.0
    assert mine.resolve_weight_ema_decay(conf) == 0.99 and mine.resolve_weight_ema_warmup(conf) == 10.0   # the constructor wins
    conf.trainer = {"gradient_clip_val": 0.5}
    assert t.resolve_weight_ema_decay(conf) == 0.0 and t.resolve_weight_ema_warmup(conf) == 0.0
    assert t.resolve_gradient_clip_val(conf) == 0.5 and t.resolve_accumulate_grad_batches(conf) == 1      # (the others are untouched)
    conf.trainer = {"weight_ema_decay": 1.0}
    with pytest.raises(ValueError, match="trainer.weight_ema_decay"):
        t.resolve_weight_ema_decay(conf)
    conf.trainer = {"weight_ema_warmup": -3}
    with pytest.raises(ValueError, match="trainer.weight_ema_warmup"):
        t.resolve_weight_ema_warmup(conf)


def test_trainer_refuses_an_average_with_torch_sgd():
    import pytorch_retinanet_amd as P
    from test_grad_accum import _ToyModel
    model = _ToyModel()
    before = [p.detach().clone() for p in model.net.parameters()]
    trainer = P.SimpleTrainer(max_epochs=1, device="cpu", precision="32", channels_last=False, weight_ema_decay=0.99)
    with pytest.raises(ValueError, match="MasterSGD / MasterAdam / MasterAdamW"):
        trainer.fit(model)
    assert trainer.weight_ema is None
    assert all(torch.equal(a, b) for a, b in zip(model.net.parameters(), before))      # refused before the first step
    # and without the option the same model trains as before
    assert P.SimpleTrainer(max_epochs=1, device="cpu", precision="32", channels_last=False).fit(_ToyModel()) == 5


def test_master_optimizers_carry_the_flag_and_no_average_by_default():
    from pytorch_retinanet_amd.optim import MasterAdam, MasterAdamW, MasterSGD
    net = torch.nn.Conv2d(3, 4, 1)
    for cls in (MasterSGD, MasterAdam, MasterAdamW):
        opt = cls(net.parameters(), lr=1e-3)
        assert opt._rn_weight_ema is True and opt.weight_ema is None
    assert not getattr(torch.optim.SGD(net.parameters(), lr=0.1), "_rn_weight_ema", False)


def test_signature_is_unchanged_without_an_average_and_keys_the_object_with_one():
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from pytorch_retinanet_amd.optim import GradAccumulator, MasterSGD, WeightEMA
    net = torch.nn.Conv2d(3, 4, 1)
    opt = MasterSGD(net.parameters(), lr=1e-2, momentum=0.9)
    images = [torch.zeros(3, 16, 16)]
    targets = [{"boxes": torch.zeros(2, 4), "labels": torch.zeros(2, dtype=torch.int64)}]
    step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16)
    none = step._signature(images, targets)
    assert len(none) == 8                                   # the key of the parent commit
    a, b = WeightEMA(0.99), WeightEMA(0.99)
    opt.weight_ema = a
    with_a = step._signature(images, targets)
    assert with_a[:-1] == none and with_a[-1] == ("weight_ema", a) and with_a[-1][1] is a
    a.decay = 0.5                                           # decay and warmup are no part of the key
    assert step._signature(images, targets) == with_a
    opt.weight_ema = b
    assert step._signature(images, targets) != with_a
    opt.weight_ema = None
    assert step._signature(images, targets) == none        # removed: the plain key again
    acc = GradAccumulator(2)
    opt.weight_ema = a
    both = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, accumulate=acc)._signature(images, targets)
    assert both[:8] == none and both[8] is acc and both[9] == ("weight_ema", a)


def test_entry_points_reject_bad_arguments_before_any_gpu_call():
    from pytorch_retinanet_amd._lib import RN_BF16, RN_F16, lib
    EINVAL, EALIGN, EUNSUP = -1, -2, -4
    p = 4096
    one = lambda v: (C.c_void_p * 1)(v)
    n1 = lambda v: (C.c_int64 * 1)(v)
    # rn_ema_set
    assert lib.rn_ema_set(0, 0.99, 0.0, -1, 0) == EINVAL
    for decay, warmup, updates in ((1.0, 0.0, 0), (-0.1, 0.0, 0), (float("nan"), 0.0, 0), (0.9, -1.0, 0), (0.9, float("nan"), 0), (0.9, 0.0, -2)):
        assert lib.rn_ema_set(p, decay, warmup, updates, 0) == EINVAL, (decay, warmup, updates)
    assert lib.rn_ema_set(p + 4, 0.99, 0.0, 0, 0) == EALIGN
    # rn_ema_advance
    assert lib.rn_ema_advance(0, 0, 0) == EINVAL and lib.rn_ema_advance(p + 4, 0, 0) == EALIGN and lib.rn_ema_advance(p, p + 2, 0) == EALIGN
    # rn_ema_update
    assert lib.rn_ema_update(0, one(p), n1(100), 1, p, 0, 0) == EINVAL                  # a null table
    assert lib.rn_ema_update(one(p), 0, n1(100), 1, p, 0, 0) == EINVAL
    assert lib.rn_ema_update(one(p), one(p), 0, 1, p, 0, 0) == EINVAL
    assert lib.rn_ema_update(one(p), one(p), n1(100), 1, 0, 0, 0) == EINVAL             # no block
    assert lib.rn_ema_update(one(p), one(p), n1(100), -1, p, 0, 0) == EINVAL
    assert lib.rn_ema_update(one(0), one(p), n1(100), 1, p, 0, 0) == EINVAL             # a null average
    assert lib.rn_ema_update(one(p), one(0), n1(100), 1, p, 0, 0) == EINVAL             # a null master
    assert lib.rn_ema_update(one(p), one(p), n1(-1), 1, p, 0, 0) == EINVAL
    assert lib.rn_ema_update(one(p + 4), one(p), n1(100), 1, p, 0, 0) == EALIGN         # fp32 arrays: 16 bytes
    assert lib.rn_ema_update(one(p), one(p + 8), n1(100), 1, p, 0, 0) == EALIGN
    assert lib.rn_ema_update(one(p), one(p), n1(100), 1, p + 4, 0, 0) == EALIGN         # the block: 8 bytes
    assert lib.rn_ema_update(one(p), one(p), n1(0), 1, p, 0, 0) == 0                    # nothing to do: no launch
    assert lib.rn_ema_update(one(p), one(p), n1(100), 0, p, 0, 0) == 0
    # rn_ema_swap
    assert lib.rn_ema_swap(one(p), one(p), one(0), n1(100), 1, 7, 0) == EUNSUP
    assert lib.rn_ema_swap(one(p), one(p), one(0), n1(100), 1, 0, 0) == EUNSUP          # RN_F32 is no 16-bit type
    assert lib.rn_ema_swap(0, one(p), one(0), n1(100), 1, RN_BF16, 0) == EINVAL
    assert lib.rn_ema_swap(one(p), 0, one(0), n1(100), 1, RN_BF16, 0) == EINVAL
    assert lib.rn_ema_swap(one(p), one(p), one(0), 0, 1, RN_BF16, 0) == EINVAL
    assert lib.rn_ema_swap(one(0), one(p), one(0), n1(100), 1, RN_F16, 0) == EINVAL
    assert lib.rn_ema_swap(one(p), one(p), one(0), n1(-5), 1, RN_F16, 0) == EINVAL
    assert lib.rn_ema_swap(one(p + 4), one(p), one(0), n1(100), 1, RN_BF16, 0) == EALIGN
    assert lib.rn_ema_swap(one(p), one(p + 8), one(0), n1(100), 1, RN_BF16, 0) == EALIGN
    assert lib.rn_ema_swap(one(p), one(p), one(p + 4), n1(100), 1, RN_BF16, 0) == EALIGN          # 16-bit arrays: 8 bytes
    assert lib.rn_ema_swap(one(p), one(p), 0, n1(0), 1, RN_BF16, 0) == 0                # params16 itself may be null; nothing to do
    assert lib.rn_ema_swap(one(p), one(p), one(0), n1(100), 0, RN_BF16, 0) == 0


def test_state_dict_waits_in_a_fresh_object_and_documents_mention_the_option():
    import os
    import pytorch_retinanet_amd as P
    from pytorch_retinanet_amd.optim import WeightEMA
    saved = {"decay": 0.9, "warmup": 4.0, "updates": 7, "ema": [torch.arange(3.0), torch.ones(2, 2)]}
    e = WeightEMA()
    e.load_state_dict(saved)
    assert (e.decay, e.warmup, e.updates) == (0.9, 4.0, 7) and not e.ready
    back = e.state_dict()
    assert back["updates"] == 7 and all(torch.equal(a, b) for a, b in zip(back["ema"], saved["ema"]))
    with pytest.raises(ValueError, match="decay must be in"):
        e.load_state_dict(dict(saved, decay=1.0))
    with pytest.raises(ValueError, match="updates"):
        e.load_state_dict(dict(saved, updates=-1))
    text = open(os.path.join(os.path.dirname(P.__file__), "hparams.yaml")).read()
    assert "weight_ema_decay" in text and "weight_ema_warmup" in text


def test_denseness_check_of_the_flat_walk():
    from pytorch_retinanet_amd.optim import _is_dense
    x = torch.zeros(4, 6, 3, 3)
    assert _is_dense(x) and _is_dense(x.contiguous(memory_format=torch.channels_last)) and _is_dense(x.permute(1, 0, 3, 2))
    assert _is_dense(torch.zeros(0)) and _is_dense(torch.zeros(())) and _is_dense(torch.zeros(5, 1)[:, 0]) and _is_dense(x[1:3])
    assert not _is_dense(x[:, ::2]) and not _is_dense(x[..., 1:]) and not _is_dense(torch.zeros(8)[::2]) and not _is_dense(torch.zeros(3).expand(2, 3))
