"""GPU: the weight average of the master optimizers -- ``rn_ema_update`` / ``rn_ema_advance`` / ``rn_ema_swap`` / ``rn_ema_set``
(csrc/ema.hip) through ``optim.WeightEMA``: the update against its torch restatement bit for bit, the skip on ``found_inf``, the swap
and its undo, the argument checks, the update inside a captured ``MasterSGD`` step, under fp16 loss scaling, under gradient
accumulation, through ``SimpleTrainer``, and the checkpoint round trip.

Bars: the kernel's arithmetic is fixed -- ``ema = w`` at the first update, then ``ema + (w - ema) * om`` in fp32 with three roundings, ``om``
the float32 of a double expression that ``WeightEMA.one_minus_decay`` restates -- so every comparison is bit-equality.  The captured
step is compared against the restatement applied to ITS OWN masters, never against a second run (the convolutions' weight gradients
are not bit-reproducible between runs)."""
import numpy as np
import pytest
import torch

import synth
from test_master_adam_gpu import SIZES, _make, _r18

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = 16384
MODES = ["bf16", "f16"]
SENTINEL32, SENTINEL16 = -77.0, 123.0
# every path of the chunked map: below one vector, whole vectors, the chunk boundary and both neighbours, more than two chunks with a
# tail; then a channels-last 4-D tensor; then 170 small tensors -- more than either table holds (160 / 120): a second launch
FLAT = [1, 3, 7, 8, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5]
CONV = (16, 8, 3, 3)
SMALL = [(i * 7) % 37 + 1 for i in range(170)]


class _Set:
    """The fixture's tensors, each carved from one buffer per kind (masters, averages, 16-bit copies) with 4 sentinel elements in front
    of, between and behind them; every other tensor has a 16-bit working copy.  ``install(ema)`` hands the carved averages to a
    ``WeightEMA`` in place of the ones it would allocate, so that the sentinels around the averages are checked too."""

    def __init__(self, mode, seed=0):
        self.dt16 = torch.bfloat16 if mode == "bf16" else torch.float16
        shapes = [(n,) for n in FLAT] + [CONV] + [(n,) for n in SMALL]
        spans, off = [], 4
        for shape in shapes:
            n = int(np.prod(shape))
            spans.append((off, n))
            off = (off + n + 3) // 4 * 4 + 4                 # fp32 views 16-byte aligned, 16-bit views 8-byte aligned
        self.total = off
        self.masters_buf = torch.full((off,), SENTINEL32, device=DEV)
        self.emas_buf = torch.full((off,), SENTINEL32, device=DEV)
        self.p16_buf = torch.full((off,), SENTINEL16, device=DEV, dtype=self.dt16)
        self.inside = torch.zeros(off, dtype=torch.bool, device=DEV)
        self.inside16 = torch.zeros(off, dtype=torch.bool, device=DEV)
        self.params, self.emas = [], []

        def carve(buf, o, n, shape):
            v = buf[o:o + n]
            return v.view(shape[0], shape[2], shape[3], shape[1]).permute(0, 3, 1, 2) if len(shape) == 4 else v
        for i, ((o, n), shape) in enumerate(zip(spans, shapes)):
            w = carve(self.masters_buf, o, n, shape)
            self.inside[o:o + n] = True
            if i % 2 == 0:
                p = torch.nn.Parameter(carve(self.p16_buf, o, n, shape))
                p.master = w
                self.inside16[o:o + n] = True
            else:
                p = torch.nn.Parameter(w)
            assert (p.master if hasattr(p, "master") else p.data).data_ptr() == w.data_ptr() and w.data_ptr() % 16 == 0
            self.params.append(p)
            self.emas.append(carve(self.emas_buf, o, n, shape))
        assert self.params[len(FLAT)].master.is_contiguous(memory_format=torch.channels_last)
        self.gen = torch.Generator(device=DEV).manual_seed(seed)
        self.randomise()

    def masters(self):
        return [p.master if hasattr(p, "master") else p.data for p in self.params]

    def randomise(self):
        "Fresh finite random masters, the 16-bit copies their rounding (what an optimizer step leaves behind)."
        for p, w in zip(self.params, self.masters()):
            w.copy_(torch.randn(w.shape, device=DEV, generator=self.gen))
            if hasattr(p, "master"):
                p.data.copy_(w)

    def install(self, ema):
        for p, a in zip(self.params, self.emas):
            a.fill_(float("nan"))                            # the first update overwrites: nothing of this survives
            ema.preallocate(p, a)
        return ema

    def sentinels_untouched(self):
        return (bool((self.masters_buf[~self.inside] == SENTINEL32).all()) and bool((self.emas_buf[~self.inside] == SENTINEL32).all())
                and bool((self.p16_buf[~self.inside16] == SENTINEL16).all()))


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _restate(ema, w, t, decay, warmup):
    "The update number t in torch's fp32 ops: three separately rounded kernels, om from the pure-Python restatement."
    from pytorch_retinanet_amd.optim import WeightEMA
    if t == 0:
        return w.clone()
    om = torch.tensor(WeightEMA.one_minus_decay(t, decay, warmup), dtype=torch.float32, device=w.device)
    d = w - ema
    m = d * om
    return ema + m


# ---- 1. the update against its restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("warmup", [0.0, 10.0])
def test_update_equals_its_restatement_bit_for_bit(mode, warmup):
    from pytorch_retinanet_amd.optim import WeightEMA
    s = _Set(mode, seed=1)
    ema = s.install(WeightEMA(0.9998 if warmup else 0.9, warmup))
    want = [None] * len(s.params)
    for t in range(4):
        s.randomise()
        want = [_restate(a, w, t, ema.decay, warmup) for a, w in zip(want, s.masters())]
        assert ema.update(s.params) == len(s.params)
        torch.cuda.synchronize()
        assert ema.updates == t + 1
        for i, (a, r) in enumerate(zip(s.emas, want)):
            assert torch.equal(_bits(a), _bits(r)), (t, i, tuple(a.shape), float((a - r).abs().max()))
        assert float(ema.next_factor) == float(WeightEMA.one_minus_decay(t + 1, ema.decay, warmup))
        assert s.sentinels_untouched()
    assert ema.stats() == {"updates": 4, "skipped": 0}
    for a, p in zip(s.emas, s.params):
        assert ema.average_of(p) is a and a.stride() == (p.master if hasattr(p, "master") else p.data).stride()


def test_update_allocates_its_averages_in_the_masters_strides():
    from pytorch_retinanet_amd.optim import WeightEMA
    s = _Set("bf16", seed=2)
    ema = WeightEMA(0.5)
    ema.update(s.params)
    torch.cuda.synchronize()
    assert ema.ready and ema.parameters() == s.params
    for p, w in zip(s.params, s.masters()):
        a = ema.average_of(p)
        assert a.dtype == torch.float32 and a.stride() == w.stride() and torch.equal(a, w)        # the first update copies


# ---- 2. the skip -----------------------------------------------------------------------------------------------------------------------
def test_found_inf_skips_the_update_on_the_device():
    from pytorch_retinanet_amd.optim import WeightEMA
    s = _Set("bf16", seed=3)
    ema = s.install(WeightEMA(0.9))
    ema.update(s.params)
    s.randomise()
    ema.update(s.params)
    torch.cuda.synchronize()
    snap = s.emas_buf.clone()
    found = torch.ones((), dtype=torch.float32, device=DEV)
    s.randomise()
    ema.update(s.params, found)
    torch.cuda.synchronize()
    assert torch.equal(_bits(s.emas_buf), _bits(snap))
    assert ema.updates == 2 and ema.stats() == {"updates": 2, "skipped": 1}
    found.zero_()
    want = [_restate(a.clone(), w, 2, 0.9, 0.0) for a, w in zip(s.emas, s.masters())]
    ema.update(s.params, found)
    torch.cuda.synchronize()
    assert ema.stats() == {"updates": 3, "skipped": 1}
    for a, r in zip(s.emas, want):
        assert torch.equal(_bits(a), _bits(r))
    assert not torch.equal(_bits(s.emas_buf), _bits(snap)) and s.sentinels_untouched()


# ---- 3. the swap -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_swap_exchanges_and_a_second_swap_restores_every_bit(mode):
    from pytorch_retinanet_amd.optim import WeightEMA
    s = _Set(mode, seed=4)
    ema = s.install(WeightEMA(0.5))
    ema.update(s.params)
    s.randomise()
    ema.update(s.params)                                     # (the averages now differ from the masters)
    torch.cuda.synchronize()
    start = (s.masters_buf.clone(), s.emas_buf.clone(), s.p16_buf.clone())
    old_w, old_a = [w.clone() for w in s.masters()], [a.clone() for a in s.emas]
    assert not ema.is_swapped
    ema.swap(s.params)
    torch.cuda.synchronize()
    assert ema.is_swapped
    for p, w, a, ow, oa in zip(s.params, s.masters(), s.emas, old_w, old_a):
        assert torch.equal(_bits(w), _bits(oa)) and torch.equal(_bits(a), _bits(ow))
        if hasattr(p, "master"):
            assert torch.equal(_bits(p.data), _bits(w.to(s.dt16)))
    assert any(not torch.equal(ow, oa) for ow, oa in zip(old_w, old_a)) and s.sentinels_untouched()
    with pytest.raises(RuntimeError, match="while swapped"):
        ema.update(s.params)
    with pytest.raises(RuntimeError, match="all 179 averaged parameters"):
        ema.swap(s.params[:5])                               # a subset is refused: is_swapped is one flag for all
    assert ema.is_swapped
    with pytest.raises(RuntimeError, match="while swapped"):
        ema.state_dict()
    ema.swap(s.params)
    torch.cuda.synchronize()
    assert not ema.is_swapped
    for now, then in zip((s.masters_buf, s.emas_buf, s.p16_buf), start):
        assert torch.equal(_bits(now), _bits(then))          # masters, fp32-only parameters, averages, 16-bit copies and sentinels
    with ema.swapped():                                      # the context manager, over every averaged parameter
        assert ema.is_swapped and torch.equal(_bits(s.masters()[5]), _bits(old_a[5]))
    with pytest.raises(KeyError):
        with ema.swapped(s.params):
            raise KeyError("validation failed")
    torch.cuda.synchronize()
    assert not ema.is_swapped                                # undone when the block raises, too
    for now, then in zip((s.masters_buf, s.emas_buf, s.p16_buf), start):
        assert torch.equal(_bits(now), _bits(then))


def test_a_parameter_that_is_not_dense_in_memory_is_refused():
    from pytorch_retinanet_amd.optim import WeightEMA
    base = torch.randn(8, 8, device=DEV)
    before = base.clone()
    ema = WeightEMA(0.5)
    with pytest.raises(ValueError, match="not dense"):
        ema.update([torch.nn.Parameter(base[:, ::2])])       # numel() consecutive elements from data_ptr() are not this view
    torch.cuda.synchronize()
    assert not ema.ready and torch.equal(base, before)
    assert ema.update([torch.nn.Parameter(base.t())]) == 1   # a transposed view IS dense: the average takes its strides
    with pytest.raises(ValueError, match="storage"):
        WeightEMA(0.5).preallocate(torch.nn.Parameter(base), torch.empty(8, 8, device=DEV).t())


# ---- 4. the argument checks ------------------------------------------------------------------------------------------------------------
def test_argument_checks_come_before_any_launch():
    import ctypes as C
    from pytorch_retinanet_amd._lib import RN_BF16, lib
    EINVAL, EALIGN, EUNSUP = -1, -2, -4
    buf = torch.arange(64, dtype=torch.float32, device=DEV)
    a, w, blk = buf[0:16], buf[16:32], torch.zeros(8, dtype=torch.float64, device=DEV)
    p16 = torch.full((16,), 5.0, dtype=torch.bfloat16, device=DEV)
    before, st = buf.clone(), torch.cuda.current_stream().cuda_stream
    ptrs = lambda *v: (C.c_void_p * len(v))(*v)
    ns = lambda *v: (C.c_int64 * len(v))(*v)
    assert lib.rn_ema_update(None, ptrs(w.data_ptr()), ns(16), 1, blk.data_ptr(), None, st) == EINVAL                     # a null table
    assert lib.rn_ema_update(ptrs(a.data_ptr()), None, ns(16), 1, blk.data_ptr(), None, st) == EINVAL
    assert lib.rn_ema_update(ptrs(a.data_ptr(), 0), ptrs(w.data_ptr(), w.data_ptr()), ns(8, 8), 2, blk.data_ptr(), None, st) == EINVAL
    assert lib.rn_ema_update(ptrs(a.data_ptr(), a[1:].data_ptr()), ptrs(w.data_ptr(), w.data_ptr()), ns(8, 8), 2, blk.data_ptr(), None, st) == EALIGN
    assert lib.rn_ema_update(ptrs(a.data_ptr()), ptrs(w[1:].data_ptr()), ns(8), 1, blk.data_ptr(), None, st) == EALIGN    # a 4-byte-offset view
    assert lib.rn_ema_swap(None, ptrs(w.data_ptr()), ptrs(0), ns(16), 1, RN_BF16, st) == EINVAL
    assert lib.rn_ema_swap(ptrs(a.data_ptr()), ptrs(w[1:].data_ptr()), ptrs(0), ns(8), 1, RN_BF16, st) == EALIGN
    assert lib.rn_ema_swap(ptrs(a.data_ptr()), ptrs(w.data_ptr()), ptrs(p16[1:].data_ptr()), ns(8), 1, RN_BF16, st) == EALIGN
    assert lib.rn_ema_swap(ptrs(a.data_ptr()), ptrs(w.data_ptr()), ptrs(p16.data_ptr()), ns(16), 1, 0, st) == EUNSUP      # RN_F32
    assert lib.rn_ema_swap(ptrs(a.data_ptr()), ptrs(w.data_ptr()), ptrs(p16.data_ptr()), ns(16), 1, 9, st) == EUNSUP
    assert lib.rn_ema_set(blk.data_ptr(), 1.0, 0.0, 0, st) == EINVAL and lib.rn_ema_set(None, 0.5, 0.0, 0, st) == EINVAL
    assert lib.rn_ema_advance(None, None, st) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and bool((p16 == 5.0).all()) and bool((blk == 0).all())       # nothing was launched


# ---- 5. inside the captured step -------------------------------------------------------------------------------------------------------
def _batches(n, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        images = [torch.from_numpy(rng.random((3, 128, 160), dtype=np.float32)).to(DEV) for _ in range(2)]
        targets = []
        for _ in range(2):
            b, l = synth.gt_boxes(rng, 3, 128, 160, num_classes=5, wh_lo=20.0, wh_hi=90.0)
            targets.append({"boxes": torch.from_numpy(b).to(DEV), "labels": torch.from_numpy(l).to(DEV)})
        out.append((images, targets))
    return out


def _masters(net):
    return [p.master if hasattr(p, "master") else p.data for p in net.parameters()]


def test_captured_master_sgd_step_updates_the_average():
    """R18, B = 2, bf16, MasterSGD, six steps (one eager, one capturing, replays): after each the average equals the restatement applied
    to its own snapshot and the masters as they are now; decay rewritten before the fifth step, no new capture."""
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from pytorch_retinanet_amd.optim import MasterSGD, WeightEMA, use_bf16_conv_weights
    net = _r18(seed=11)
    use_bf16_conv_weights(net)
    opt = MasterSGD(net.parameters(), lr=1e-2, momentum=0.9, weight_decay=1e-3)
    ema = opt.weight_ema = WeightEMA(0.9, warmup=3.0)
    step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=1)
    params = list(net.parameters())
    start = [w.clone() for w in _masters(net)]
    for i, (im, tg) in enumerate(_batches(6)):
        if i == 4:
            captures = step.captures
            ema.decay = 0.5                                  # between two replays: one tiny launch
        snap = [ema.average_of(p).clone() for p in params] if i else [None] * len(params)
        assert ema.updates == i
        loss = float(step(im, tg)["loss"])
        torch.cuda.synchronize()
        assert np.isfinite(loss) and ema.updates == i + 1
        for k, (p, a, w) in enumerate(zip(params, snap, _masters(net))):
            r = _restate(a, w, i, ema.decay, 3.0)
            assert torch.equal(_bits(ema.average_of(p)), _bits(r)), (i, k, tuple(w.shape))
    assert step.captures == 1 and captures == 1 and step.replays >= 4
    assert sum(not torch.equal(a, b) for a, b in zip(start, _masters(net))) > len(start) // 2       # (the steps really stepped)
    assert sum(not torch.equal(ema.average_of(p), w) for p, w in zip(params, _masters(net))) > len(start) // 2
    assert ema.stats() == {"updates": 6, "skipped": 0}
    # an average installed or removed afterwards is another key: no graph captured without it is replayed with it
    key = step._signature(*_batches(1)[0])
    opt.weight_ema = None
    assert step._signature(*_batches(1)[0]) != key


# ---- 6. under fp16 loss scaling ---------------------------------------------------------------------------------------------------------
def test_a_step_skipped_by_the_loss_scaler_leaves_the_average_alone():
    from pytorch_retinanet_amd.optim import GradAccumulator, MasterSGD, WeightEMA
    from pytorch_retinanet_amd.parallel import ExchangeGradScaler
    from test_grad_accum_gpu import _rand_grads
    params, _, dt16 = _make(SIZES[:10], "f16", seed=4)
    opt = MasterSGD(params, lr=0.05, momentum=0.9)
    ema = opt.weight_ema = WeightEMA(0.9)
    scaler = ExchangeGradScaler("cuda", init_scale=2.0 ** 10, growth_interval=1000)
    scaler.scale(torch.ones(1, device=DEV))              # (creates the scale tensor, as the first scaled loss does)
    acc = GradAccumulator(1)
    master = lambda p: p.master if hasattr(p, "master") else p.data

    def one_step(k, poisoned):
        for p, g in zip(params, _rand_grads(params, 10 + k)):
            p.grad = (g.float() * 2.0 ** 10).to(p.dtype)
        if poisoned:
            params[3].grad[0] = float("inf")
        acc.accumulate(params)
        scaler.step_exchanged(opt, acc)
        scaler.update()
        acc.advance(True)
        torch.cuda.synchronize()

    one_step(0, False)
    one_step(1, False)
    assert ema.updates == 2
    snap_a, snap_w = [ema.average_of(p).clone() for p in params], [master(p).clone() for p in params]
    one_step(2, True)
    assert ema.stats() == {"updates": 2, "skipped": 1} and float(scaler.get_scale()) == 2.0 ** 9
    for p, a, w in zip(params, snap_a, snap_w):
        assert torch.equal(_bits(ema.average_of(p)), _bits(a)) and torch.equal(_bits(master(p)), _bits(w))
    one_step(3, False)
    assert ema.stats() == {"updates": 3, "skipped": 1}
    for p, a in zip(params, snap_a):
        assert torch.equal(_bits(ema.average_of(p)), _bits(_restate(a, master(p), 2, 0.9, 0.0)))
        assert not torch.equal(ema.average_of(p), a)


# ---- 7. under gradient accumulation -------------------------------------------------------------------------------------------------------
def test_accumulation_micro_steps_do_not_update():
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from pytorch_retinanet_amd.optim import GradAccumulator, MasterSGD, WeightEMA, use_bf16_conv_weights
    net = _r18(seed=11)
    use_bf16_conv_weights(net)
    opt = MasterSGD(net.parameters(), lr=1e-2, momentum=0.9)
    ema = opt.weight_ema = WeightEMA(0.9)
    acc = GradAccumulator(2)
    step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=1, accumulate=acc)
    seen = []
    for im, tg in _batches(4):
        step(im, tg)
        torch.cuda.synchronize()
        seen.append(ema.updates)
    assert seen == [0, 1, 1, 2] and acc.stats()["windows"] == 2


# ---- 8. the trainer -----------------------------------------------------------------------------------------------------------------------
def test_simple_trainer_validates_and_tests_on_the_average():
    import pytorch_retinanet_amd as P
    from pytorch_retinanet_amd.optim import WeightEMA
    torch.manual_seed(7)
    conf = P.load_hparams()
    conf.model.update(backbone_kind="resnet18", pretrained=False, num_classes=5, min_size=128, max_size=160)
    conf.dataset.kind = "synthetic"
    conf.dataset.update(length=8, height=128, width=160, boxes_per_image=3)
    conf.dataloader.train_bs = conf.dataloader.valid_bs = conf.dataloader.test_bs = 2
    conf.dataloader.args.pin_memory = False
    conf.optimizer.class_name = "pytorch_retinanet_amd.optim.MasterSGD"
    conf.optimizer.params = {"lr": 1e-3, "momentum": 0.9, "weight_decay": 1e-3}
    conf.scheduler.class_name = None
    seen = {"val": [], "test": []}

    class Model(P.RetinaNetModel):
        def validation_step(self, batch, batch_idx, *args, **kwargs):
            seen["val"].append(trainer.weight_ema.is_swapped)
            return super().validation_step(batch, batch_idx, *args, **kwargs)

        def test_step(self, batch, batch_idx, *args, **kwargs):
            seen["test"].append(trainer.weight_ema.is_swapped)
            return super().test_step(batch, batch_idx, *args, **kwargs)

    model = Model(conf)
    model.prepare_data()
    trainer = P.SimpleTrainer(max_epochs=2, device=DEV, weight_ema_decay=0.99, weight_ema_warmup=2.0)
    steps = trainer.fit(model)
    ema = trainer.weight_ema
    assert steps == 8 and isinstance(ema, WeightEMA) and model.optimizer.weight_ema is ema and (ema.decay, ema.warmup) == (0.99, 2.0)
    assert seen["val"] == [True] * 8 and not ema.is_swapped           # 4 validation batches per epoch, all on the average
    assert ema.stats() == {"updates": steps, "skipped": 0} and trainer.captured_steps > 0
    params = list(model.net.parameters())
    assert ema.parameters() == params
    before = [(p.data.clone(), (p.master if hasattr(p, "master") else p.data).clone(), ema.average_of(p).clone()) for p in params]
    assert sum(not torch.equal(w, a) for _, w, a in before) > len(params) // 2      # the average lags the weights
    trainer.test(model)
    assert seen["test"] == [True] * 4 and not ema.is_swapped
    for p, (c, w, a) in zip(params, before):                          # a swap and its undo restore the training weights bit for bit
        assert torch.equal(_bits(p.data), _bits(c)) and torch.equal(_bits(p.master if hasattr(p, "master") else p.data), _bits(w))
        assert torch.equal(_bits(ema.average_of(p)), _bits(a))

    class Other:                                                      # another model: its parameters are not the averaged ones
        net = torch.nn.Linear(2, 2).to(DEV)
    with pytest.raises(RuntimeError, match="without an average"):
        with trainer._ema_weights(Other()):
            pass
    assert not ema.is_swapped

    class Failing(Exception):
        pass

    def boom(*a, **k):
        raise Failing()
    model.validation_step = boom
    with pytest.raises(Failing):
        trainer._validate(model)
    assert not ema.is_swapped                                         # undone when validation raises
    for p, (c, w, a) in zip(params, before):
        assert torch.equal(_bits(p.master if hasattr(p, "master") else p.data), _bits(w))


def test_simple_trainer_refuses_an_average_with_torch_sgd_on_the_gpu():
    import pytorch_retinanet_amd as P
    from test_grad_accum_gpu import _trainer_conf
    model = _trainer_conf("torch.optim.SGD", {"lr": 1e-2, "momentum": 0.9}, length=4)
    with pytest.raises(ValueError, match="MasterSGD / MasterAdam / MasterAdamW"):
        P.SimpleTrainer(max_epochs=1, device=DEV, weight_ema_decay=0.99).fit(model)


# ---- 9. the checkpoint ---------------------------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_into_a_fresh_object():
    from pytorch_retinanet_amd.optim import WeightEMA
    s = _Set("bf16", seed=6)
    a = WeightEMA(0.9998, warmup=10.0)
    for _ in range(3):
        s.randomise()
        a.update(s.params)
    sd = a.state_dict()
    assert sd["updates"] == 3 and sd["decay"] == 0.9998 and sd["warmup"] == 10.0 and len(sd["ema"]) == len(s.params)
    sd["ema"] = [t.cpu() for t in sd["ema"]]                 # (as a checkpoint read from disk)
    b = WeightEMA()
    b.load_state_dict(sd)
    assert b.updates == 3 and (b.decay, b.warmup) == (0.9998, 10.0)
    s.randomise()
    a.update(s.params)
    b.update(s.params)
    torch.cuda.synchronize()
    assert a.stats() == b.stats() == {"updates": 4, "skipped": 0}
    assert float(a.next_factor) == float(b.next_factor) == float(WeightEMA.one_minus_decay(4, 0.9998, 10.0))
    for p in s.params:
        assert a.average_of(p) is not b.average_of(p) and torch.equal(_bits(a.average_of(p)), _bits(b.average_of(p)))
        assert b.average_of(p).stride() == a.average_of(p).stride()
    # and into an object that already has its averages: by position
    a.load_state_dict(sd)
    torch.cuda.synchronize()
    assert a.updates == 3
    for p, t in zip(s.params, sd["ema"]):
        assert torch.equal(a.average_of(p).cpu(), t)
