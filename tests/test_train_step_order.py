"""CPU suite: the ORDER in which ``graph.CapturedTrainStep`` drives its collaborators -- net, autograd, gradient exchange, loss scaler,
accumulator, optimizer -- on every path of the step: plain, exchanged, segmented, accumulating, each with and without a scaler.
The collaborators are stubs that append to one log; the net is a chain of four ``Linear``s whose trunk cuts after three of them, so
the staged backward pass has the real one's four parts (head | layer4, layer3 | layer2 .. stem).  On a CPU every call runs the
eager step, which is the function a capture records.
(What the step computes on the device is in test_graph_gpu.py, test_traj_gpu.py and test_grad_accum_gpu.py, -m gpu.)"""
import pytest
import torch

from pytorch_retinanet_amd.graph import CapturedTrainStep
from pytorch_retinanet_amd.optim import GradAccumulator

SCALE = 4.0
BACKWARD = ["backward:head", "backward:layer4", "backward:layer3", "backward:stem"]
ZERO = "opt.zero_grad(set_to_none=True)"


class _Trunk(torch.nn.Module):
    "``net.backbone.backbone``: three stages, each followed by a cut when the step has installed a ``StageCuts``."
    _cuts = None

    def __init__(self, log):
        super().__init__()
        self.log = log
        self.stem, self.layer3, self.layer4 = (torch.nn.Linear(6, 6) for _ in range(3))

    @property
    def stage_cuts(self):
        return self._cuts

    @stage_cuts.setter
    def stage_cuts(self, value):
        self.log.append("stage_cuts=None" if value is None else "stage_cuts=StageCuts")
        self._cuts = value

    def forward(self, x):
        for name in ("stem", "layer3", "layer4"):
            x = torch.tanh(getattr(self, name)(x))
            x.register_hook(lambda g, name=name: self.log.append("backward:" + name))
            if self._cuts is not None:
                x = self._cuts.cut(x)
        return x


class _Net(torch.nn.Module):
    def __init__(self, log, seed=0):
        super().__init__()
        torch.manual_seed(seed)
        self.log = log
        self.backbone = torch.nn.Module()
        self.backbone.backbone = _Trunk(log)
        self.head = torch.nn.Linear(6, 2)
        self.fail = False
        self.loss_grads = []          # d(what went backward) / d(classification_loss): 1, or the scaler's scale
        self.autocast = []            # the CPU autocast dtype seen by each forward pass (None: autocast off)

    def forward(self, images, targets):
        self.log.append("net")
        assert isinstance(images, list) and isinstance(targets, list) and all(isinstance(t, dict) for t in targets)
        self.autocast.append(torch.get_autocast_dtype("cpu") if torch.is_autocast_enabled("cpu") else None)
        if self.fail:
            raise RuntimeError("the net failed")
        y = self.head(self.backbone.backbone(torch.stack(images)))
        y.register_hook(lambda g: self.log.append("backward:head"))
        cls, reg = y[:, 0].float().pow(2).mean(), y[:, 1].float().abs().mean()
        cls.register_hook(lambda g: self.loss_grads.append(float(g)))
        return {"classification_loss": cls, "regression_loss": reg}


class _SGD(torch.optim.SGD):
    "torch's SGD (so that the steps are real), logging; ``master=True``: it takes ``step(grads=...)`` like the master optimizers."

    def __init__(self, params, log, master=False):
        super().__init__(params, lr=0.1, momentum=0.9)
        self.log = log
        if master:
            self._rn_master_weights = True

    def zero_grad(self, set_to_none=True):
        self.log.append(f"opt.zero_grad(set_to_none={set_to_none})")
        super().zero_grad(set_to_none=set_to_none)

    def step(self, closure=None, grads=None):
        self.log.append("opt.step()" if grads is None else f"opt.step(grads={grads['of']}.grad_views())")
        super().step()


class _Exchange:
    deferred = False

    def __init__(self, net, log):
        self.net, self.log = net, log

    def zero_grad(self):
        self.log.append("ddp.zero_grad")
        for p in self.net.parameters():
            p.grad = None

    def issue_ready(self):
        self.log.append("ddp.issue_ready")
        return []

    def issue(self, ids):
        self.log.append("ddp.issue")

    def finish(self):
        self.log.append("ddp.finish")

    def grad_views(self):
        return {"of": "ddp"}

    def reset(self):
        self.log.append("ddp.reset")


class _Scaler:
    def __init__(self, log, names):
        self.log, self.names = log, names

    def scale(self, t):
        self.log.append("scaler.scale")
        return t * SCALE

    def step(self, opt):
        self.log.append("scaler.step(opt)")

    def step_exchanged(self, opt, source):
        self.log.append(f"scaler.step_exchanged(opt, {self.names[id(source)]})")

    def update(self):
        self.log.append("scaler.update()")


class _Accumulator(GradAccumulator):
    def __init__(self, log, n=2):
        super().__init__(n)
        self.log, self.seen = log, None

    def accumulate(self, params):
        self.log.append("acc.accumulate(params)")
        self.seen = list(params)

    def advance(self, final):
        self.log.append(f"acc.advance({final})")

    def grad_views(self):
        return {"of": "acc"}


def _batch(seed=1):
    g = torch.Generator().manual_seed(seed)
    images = [torch.randn(6, generator=g) for _ in range(3)]
    targets = [{"boxes": torch.zeros(1, 4), "labels": torch.zeros(1, dtype=torch.int64)} for _ in images]
    return images, targets


def _make(exchange=False, segmented=None, scaler=False, master=False, accumulate=False, amp_dtype=None, seed=0):
    log = []
    net = _Net(log, seed)
    opt = _SGD(net.parameters(), log, master=master or accumulate)
    ddp = _Exchange(net, log) if exchange else None
    acc = _Accumulator(log) if accumulate else None
    sc = _Scaler(log, {id(ddp): "ddp", id(acc): "acc"}) if scaler else None
    step = CapturedTrainStep(net, opt, ddp, amp_dtype=amp_dtype, segmented=segmented, scaler=sc, accumulate=acc)
    return step, net, opt, log


def _check_losses(out):
    assert set(out) == {"classification_loss", "regression_loss", "loss"}
    assert not any(v.requires_grad or v.grad_fn is not None for v in out.values())
    assert torch.equal(out["loss"], out["classification_loss"] + out["regression_loss"])


STAGED = ["ddp.zero_grad", "stage_cuts=StageCuts", "net", "stage_cuts=None", "backward:head", "ddp.issue_ready",
          "backward:layer4", "backward:layer3", "ddp.issue_ready", "backward:stem", "ddp.issue_ready", "ddp.finish"]
STAGED_SCALED = STAGED[:4] + ["scaler.scale"] + STAGED[4:]
EXCHANGED = ["ddp.zero_grad", "net"] + BACKWARD + ["ddp.finish"]
EXCHANGED_SCALED = ["ddp.zero_grad", "net", "scaler.scale"] + BACKWARD + ["ddp.finish"]
SCALED_APPLY = ["scaler.step_exchanged(opt, ddp)", "scaler.update()"]

CASES = {
    "plain": (dict(), [ZERO, "net"] + BACKWARD + ["opt.step()"]),
    "plain, master optimizer": (dict(master=True), [ZERO, "net"] + BACKWARD + ["opt.step()"]),
    "plain, scaler": (dict(scaler=True), [ZERO, "net", "scaler.scale"] + BACKWARD + ["scaler.step(opt)", "scaler.update()"]),
    "exchange, master optimizer": (dict(exchange=True, segmented=False, master=True), EXCHANGED + ["opt.step(grads=ddp.grad_views())"]),
    "exchange, other optimizer": (dict(exchange=True, segmented=False), EXCHANGED + ["opt.step()"]),
    "exchange, scaler": (dict(exchange=True, segmented=False, scaler=True, master=True), EXCHANGED_SCALED + SCALED_APPLY),
    "segmented, master optimizer": (dict(exchange=True, master=True), STAGED + ["opt.step(grads=ddp.grad_views())"]),
    "segmented, other optimizer": (dict(exchange=True), STAGED + ["opt.step()"]),
    "segmented, scaler": (dict(exchange=True, scaler=True, master=True), STAGED_SCALED + SCALED_APPLY),
}


@pytest.mark.parametrize("case", list(CASES))
def test_whole_step_call_sequence(case):
    kw, want = CASES[case]
    step, net, opt, log = _make(**kw)
    assert step.segmented == (kw.get("exchange", False) and kw.get("segmented") is not False)
    images, targets = _batch()
    for _ in range(2):                                   # (the second call: nothing of the first one lingers)
        del log[:]
        _check_losses(step(images, targets))
        assert log == want
    assert net.loss_grads == [SCALE if kw.get("scaler") else 1.0] * 2
    assert net.backbone.backbone.stage_cuts is None and net.autocast == [None, None]


@pytest.mark.parametrize("segmented", [False, True])
def test_forward_runs_under_autocast_and_only_the_forward(segmented):
    step, net, opt, log = _make(exchange=segmented, amp_dtype=torch.bfloat16)
    _check_losses(step(*_batch()))
    assert net.autocast == [torch.bfloat16] and not torch.is_autocast_enabled("cpu")


def test_segmented_step_removes_the_cuts_when_the_net_raises():
    step, net, opt, log = _make(exchange=True)
    net.fail = True
    with pytest.raises(RuntimeError, match="the net failed"):
        step(*_batch())
    assert log == ["ddp.zero_grad", "stage_cuts=StageCuts", "net", "stage_cuts=None"]
    assert net.backbone.backbone.stage_cuts is None


MICRO = [ZERO, "net"] + BACKWARD + ["acc.accumulate(params)"]
MICRO_SCALED = [ZERO, "net", "scaler.scale"] + BACKWARD + ["acc.accumulate(params)"]


@pytest.mark.parametrize("scaler", [False, True])
def test_accumulating_step_call_sequence(scaler):
    step, net, opt, log = _make(accumulate=True, scaler=scaler)
    micro = MICRO_SCALED if scaler else MICRO
    apply = ["scaler.step_exchanged(opt, acc)", "scaler.update()"] if scaler else ["opt.step(grads=acc.grad_views())"]
    images, targets = _batch()
    for final, want in ((False, micro + ["acc.advance(False)"]), (True, micro + apply + ["acc.advance(True)"])):
        del log[:]
        _check_losses(step(images, targets, final=final))
        assert log == want                                # a micro step touches neither the optimizer's step nor the scaler's
        assert [id(p) for p in step.accumulate.seen] == [id(p) for g in opt.param_groups for p in g["params"]]
    # the UNDIVIDED loss went backward in both calls (1 / n is the accumulator's business)
    assert net.loss_grads == [SCALE if scaler else 1.0] * 2


def test_plain_exchanged_and_segmented_steps_compute_the_same_bits():
    runs = []
    for kw in (dict(), dict(exchange=True, segmented=False), dict(exchange=True)):
        step, net, opt, log = _make(**kw)
        losses = [step(*_batch(seed))["loss"] for seed in (1, 2, 3)]
        runs.append((losses, [p.detach().clone() for p in net.parameters()]))
    (l0, p0), rest = runs[0], runs[1:]
    assert not any(torch.equal(a, b) for a, b in zip(p0, _Net([]).parameters()))         # (the three steps moved every parameter)
    for losses, params in rest:
        assert all(torch.equal(a, b) for a, b in zip(losses, l0))
        assert all(torch.equal(a, b) for a, b in zip(params, p0))
