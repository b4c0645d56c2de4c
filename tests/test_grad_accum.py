"""CPU suite: the host side of gradient accumulation -- argument validation of ``optim.GradAccumulator``, ``CapturedTrainStep(accumulate=)``
and ``SimpleTrainer(accumulate_grad_batches=)``, the hparams resolution, ``CapturedTrainStep``'s signature (unchanged without an
accumulator; the installed object, not its ``n``, with one), the new entry points' argument checks, and the trainer's eager path
against a hand-written loop, bit for bit.
(The kernel, found_inf, the optimizers, the captured step and the trainer's device path are in test_grad_accum_gpu.py, -m gpu.)"""
import pytest
import torch


def test_accumulator_argument_validation():
    from pytorch_retinanet_amd.optim import GradAccumulator, check_accumulate_grad_batches
    for bad in (0, -1, 2.0, 1.5, True, "4", None):
        with pytest.raises(ValueError, match="int >= 1"):
            GradAccumulator(bad)
    with pytest.raises(ValueError, match="dict schedules"):
        GradAccumulator({0: 2, 4: 8})
    with pytest.raises(ValueError, match="2\\*\\*24"):
        check_accumulate_grad_batches(1 << 24)
    a = GradAccumulator(4)
    assert a.n == 4 and "4" in repr(a) and GradAccumulator().n == 1
    a.n = 2                                             # (no device block yet: only the host value changes)
    assert a.n == 2
    with pytest.raises(ValueError, match="int >= 1"):
        a.n = 0
    assert a.n == 2
    assert a.position == 0 and a.stats() == {"windows": 0, "nonfinite": 0, "micro_batches": 0} and a.grad_views() == {}
    with pytest.raises(RuntimeError, match="nothing has been accumulated"):
        a.found_inf()
    with pytest.raises(RuntimeError, match="nothing has been accumulated"):
        a.advance(True)
    assert a.accumulate([torch.nn.Parameter(torch.zeros(3))]) == 0          # no gradient: nothing to do, no device needed


def test_n_cannot_change_in_mid_window():
    from pytorch_retinanet_amd.optim import GradAccumulator
    a = GradAccumulator(3)
    assert not a.next_is_final()
    a.note_step(False)                                  # (what an eager advance / a replayed micro step records)
    with pytest.raises(RuntimeError, match="mid-window"):
        a.n = 2
    assert a.n == 3
    a.note_step(False)
    assert a.next_is_final()
    a.note_step(True)
    a.n = 2                                             # between windows: fine
    assert a.n == 2 and not a.next_is_final()


def test_accumulator_refuses_cpu_gradients():
    from pytorch_retinanet_amd.optim import GradAccumulator
    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = torch.ones(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GradAccumulator(2).accumulate([p])


def _stepper(opt, net, **kw):
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    return CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, **kw)


def test_captured_step_argument_validation():
    from pytorch_retinanet_amd.optim import GradAccumulator, MasterSGD
    from pytorch_retinanet_amd.parallel import ExchangeGradScaler
    net = torch.nn.Conv2d(3, 4, 1)
    opt = MasterSGD(net.parameters(), lr=1e-2, momentum=0.9)

    class FakeExchange:
        deferred = False
    with pytest.raises(ValueError, match="single-process"):
        _stepper(opt, net, accumulate=GradAccumulator(2), ddp=FakeExchange())
    with pytest.raises(TypeError, match="GradAccumulator"):
        _stepper(opt, net, accumulate=2)
    with pytest.raises(ValueError, match="MasterSGD"):
        _stepper(torch.optim.SGD(net.parameters(), lr=0.1), net, accumulate=GradAccumulator(2))
    with pytest.raises(ValueError, match="ExchangeGradScaler"):
        _stepper(opt, net, accumulate=GradAccumulator(2), scaler=torch.amp.GradScaler("cuda", enabled=False))
    _stepper(opt, net, accumulate=GradAccumulator(2), scaler=ExchangeGradScaler("cuda", enabled=False))
    plain = _stepper(opt, net)
    assert plain.accumulate is None
    with pytest.raises(ValueError, match="final=False"):
        plain([torch.zeros(3, 16, 16)], [{"boxes": torch.zeros(1, 4), "labels": torch.zeros(1, dtype=torch.int64)}], final=False)


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_signature_is_unchanged_without_an_accumulator_and_keys_the_object_with_one(kind):
    from pytorch_retinanet_amd.optim import GradAccumulator, MasterAdamW, MasterSGD
    net = torch.nn.Conv2d(3, 4, 1)
    opt = MasterSGD(net.parameters(), lr=1e-2, momentum=0.9) if kind == "sgd" else MasterAdamW(net.parameters(), lr=1e-3)
    images = [torch.zeros(3, 16, 16)]
    targets = [{"boxes": torch.zeros(2, 4), "labels": torch.zeros(2, dtype=torch.int64)}]
    plain = _stepper(opt, net)
    none = plain._signature(images, targets)
    assert len(none) == 8 and none[-2:] == (None, None)                 # (..., amp dtype, hflip, clip): the key of the parent commit
    assert none == _stepper(opt, net, accumulate=None)._signature(images, targets)
    a, b = GradAccumulator(4), GradAccumulator(4)
    with_a = _stepper(opt, net, accumulate=a)._signature(images, targets)
    with_b = _stepper(opt, net, accumulate=b)._signature(images, targets)
    assert with_a[:-1] == none and with_a[-1] is a and with_b[-1] is b and with_a != with_b
    a.n = 2                                                              # n and the window position are no part of the key
    a.note_step(False)
    assert _stepper(opt, net, accumulate=a)._signature(images, targets) == with_a


def test_trainer_argument_validation_and_hparams_resolution():
    import pytorch_retinanet_amd as P
    conf = P.load_hparams()
    assert "trainer" not in conf                                          # the shipped file keeps the reference's key set
    t = P.SimpleTrainer(device="cpu")
    assert t.accumulate_grad_batches == 1 and t.resolve_accumulate_grad_batches(conf) == 1 and t.grad_accumulator is None
    assert P.SimpleTrainer(device="cpu", accumulate_grad_batches=4).resolve_accumulate_grad_batches(conf) == 4
    for bad in (0, -2, 2.0, True):
        with pytest.raises(ValueError, match="accumulate_grad_batches must be an int >= 1"):
            P.SimpleTrainer(device="cpu", accumulate_grad_batches=bad)
    with pytest.raises(ValueError, match="dict schedules"):
        P.SimpleTrainer(device="cpu", accumulate_grad_batches={0: 2})
    conf.trainer = {"accumulate_grad_batches": 8}
    assert t.resolve_accumulate_grad_batches(conf) == 8
    assert P.SimpleTrainer(device="cpu", accumulate_grad_batches=4).resolve_accumulate_grad_batches(conf) == 4      # the argument wins
    conf.trainer = {"gradient_clip_val": 0.5}
    assert t.resolve_accumulate_grad_batches(conf) == 1
    for bad in (0, 2.5, {0: 2}):
        conf.trainer = {"accumulate_grad_batches": bad}
        with pytest.raises(ValueError, match="trainer.accumulate_grad_batches"):
            t.resolve_accumulate_grad_batches(conf)
    import os
    text = open(os.path.join(os.path.dirname(P.__file__), "hparams.yaml")).read()
    assert "accumulate_grad_batches" in text


def test_new_entry_points_reject_bad_arguments_before_any_gpu_call():
    import ctypes as C
    from pytorch_retinanet_amd._lib import RN_BF16, lib
    EINVAL, EALIGN, EUNSUP = -1, -2, -4
    p = 4096
    assert lib.rn_grad_accum_set(0, 2, 0) == EINVAL and lib.rn_grad_accum_set(p, 0, 0) == EINVAL and lib.rn_grad_accum_set(p, -3, 0) == EINVAL
    assert lib.rn_grad_accum_set(p + 4, 2, 0) == EALIGN
    assert lib.rn_grad_accum_advance(0, 1, 0) == EINVAL and lib.rn_grad_accum_advance(p + 4, 0, 0) == EALIGN
    one = lambda v: (C.c_void_p * 1)(v)
    n1 = lambda v: (C.c_int64 * 1)(v)
    assert lib.rn_grad_accumulate(one(p), one(p), one(0), n1(100), 1, 1, 7, p, 0) == EUNSUP
    assert lib.rn_grad_accumulate(one(p), one(p), one(0), n1(100), 1, 1, RN_BF16, 0, 0) == EINVAL            # no block
    assert lib.rn_grad_accumulate(one(0), one(p), one(0), n1(100), 1, 1, RN_BF16, p, 0) == EINVAL            # a null accumulator
    assert lib.rn_grad_accumulate(one(p), one(0), one(0), n1(100), 1, 1, RN_BF16, p, 0) == EINVAL            # a null gradient
    assert lib.rn_grad_accumulate(one(p), one(p), one(0), n1(-1), 1, 1, RN_BF16, p, 0) == EINVAL
    assert lib.rn_grad_accumulate(one(p + 8), one(p), one(0), n1(100), 1, 1, RN_BF16, p, 0) == EALIGN        # accumulator: 16 bytes
    assert lib.rn_grad_accumulate(one(p), one(p + 8), one(0), n1(100), 1, 1, RN_BF16, p, 0) == EALIGN        # fp32 gradient: 16 bytes
    assert lib.rn_grad_accumulate(one(p), one(p + 4), one(p), n1(100), 1, 1, RN_BF16, p, 0) == EALIGN        # 16-bit gradient: 8 bytes
    assert lib.rn_grad_accumulate(one(p), one(p), one(0), n1(100), 1, 1, RN_BF16, p + 4, 0) == EALIGN        # the block: 8 bytes
    assert lib.rn_grad_accumulate(one(p), one(p), one(0), n1(0), 1, 1, RN_BF16, p, 0) == 0                   # nothing to do: no launch
    assert lib.rn_grad_accumulate(one(p), one(p), one(0), n1(100), 0, 1, RN_BF16, p, 0) == 0


# ---- the trainer's eager path against a hand-written loop --------------------------------------------------------------------------
BATCHES, EPOCHS, FEATURES = 5, 2, 6


class _ToyNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.transform = torch.nn.Identity()            # (SimpleTrainer looks for a train-time flip on net.transform)
        self.body = torch.nn.Sequential(torch.nn.Linear(FEATURES, 8), torch.nn.Tanh(), torch.nn.Linear(8, 1))

    def forward(self, x):
        return self.body(x)


class _ToyModel(torch.nn.Module):
    "The hooks SimpleTrainer drives, around a two-layer regression net on 5 fixed batches (its training_step is not RetinaNetModel's: eager)."

    def __init__(self, seed=0):
        super().__init__()
        torch.manual_seed(seed)
        self.net = _ToyNet()
        self.conf = {}
        g = torch.Generator().manual_seed(7)
        self.trn_ds = [((torch.randn(3, FEATURES, generator=g),), ({"y": torch.randn(3, 1, generator=g)},), (i,)) for i in range(BATCHES)]
        self.scheduler_steps = 0

    def train_dataloader(self):
        return list(self.trn_ds)                        # (batches in the collate_fn layout: images, targets, ids)

    def val_dataloader(self):
        return None

    def configure_optimizers(self):
        self.optimizer = torch.optim.SGD(self.net.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-3)
        self.lr_sched = torch.optim.lr_scheduler.StepLR(self.optimizer, step_size=1, gamma=0.9)
        return [self.optimizer], [{"scheduler": self.lr_sched, "interval": "step", "frequency": 1}]

    def training_step(self, batch, batch_idx):
        images, targets, _ = batch
        loss = ((self.net(images[0]) - targets[0]["y"]) ** 2).mean()
        return {"loss": loss}


def _hand_written(n, epochs=EPOCHS, max_steps=None):
    model = _ToyModel()
    opt = torch.optim.SGD(model.net.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-3)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.9)
    steps = 0
    for _ in range(epochs):
        for i, (images, targets, _) in enumerate(model.trn_ds):
            if i % n == 0:
                opt.zero_grad()
            loss = ((model.net(images[0]) - targets[0]["y"]) ** 2).mean()
            (loss / n).backward()
            if (i + 1) % n == 0 or i + 1 == BATCHES:                     # N = 2: after batches 2, 4 and 5 of each epoch
                opt.step()
                sched.step()
                steps += 1
                if max_steps and steps >= max_steps:
                    return model, opt, steps
    return model, opt, steps


def test_trainer_eager_accumulation_equals_a_hand_written_loop_bit_for_bit():
    import pytorch_retinanet_amd as P
    model = _ToyModel()
    trainer = P.SimpleTrainer(max_epochs=EPOCHS, device="cpu", precision="32", channels_last=False, accumulate_grad_batches=2)
    steps = trainer.fit(model)
    ref, ref_opt, ref_steps = _hand_written(2)
    assert steps == ref_steps == 3 * EPOCHS                              # optimizer steps, not the 10 batches
    assert trainer.grad_accumulator is None and trainer.captured_steps == 0
    for a, b in zip(model.net.parameters(), ref.net.parameters()):
        assert torch.equal(a, b)
    # the per-step scheduler advanced once per optimizer step: lr = 0.1 * 0.9 ** 6
    assert model.lr_sched.last_epoch == 3 * EPOCHS
    assert model.optimizer.param_groups[0]["lr"] == ref_opt.param_groups[0]["lr"] == pytest.approx(0.1 * 0.9 ** 6, rel=1e-12)
    # and it differs from plain training on the same batches (the test would otherwise pass with the argument ignored)
    plain = _ToyModel()
    assert P.SimpleTrainer(max_epochs=EPOCHS, device="cpu", precision="32", channels_last=False).fit(plain) == BATCHES * EPOCHS
    assert not all(torch.equal(a, b) for a, b in zip(plain.net.parameters(), ref.net.parameters()))


def test_trainer_max_steps_counts_optimizer_steps():
    import pytorch_retinanet_amd as P
    model = _ToyModel()
    trainer = P.SimpleTrainer(max_epochs=EPOCHS, device="cpu", precision="32", channels_last=False, accumulate_grad_batches=2, max_steps=4)
    assert trainer.fit(model) == 4                                       # three in epoch 0, then batches 1-2 of epoch 1: 7 batches
    ref, _, ref_steps = _hand_written(2, max_steps=4)
    assert ref_steps == 4 and model.lr_sched.last_epoch == 4
    for a, b in zip(model.net.parameters(), ref.net.parameters()):
        assert torch.equal(a, b)


def test_trainer_with_n_1_is_the_plain_loop():
    import pytorch_retinanet_amd as P
    a = _ToyModel()
    assert P.SimpleTrainer(max_epochs=1, device="cpu", precision="32", channels_last=False, accumulate_grad_batches=1).fit(a) == BATCHES
    ref, _, ref_steps = _hand_written(1, epochs=1)
    assert ref_steps == BATCHES
    for x, y in zip(a.net.parameters(), ref.net.parameters()):
        assert torch.equal(x, y)
