"""CPU suite: the host side of ``optim.MasterSGD(capturable=True)`` -- the two ABI symbols, the device block's layout constant,
constructor validation, the settings that are fixed once a block exists, the hparams wiring, ``SimpleTrainer``'s capture decision
for per-step schedulers and the CPU refusal.  (The numerics against the by-value step are in test_master_sgd_capturable_gpu.py.)"""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3), torch.nn.BatchNorm2d(8)).parameters()


def test_abi_symbols_and_signatures():
    from pytorch_retinanet_amd._lib import lib
    vp, f32 = C.c_void_p, C.c_float
    assert lib.rn_version() == 10                                       # additive: the ABI version stays
    assert lib.rn_sgd_hparams_set.restype is C.c_int and lib.rn_sgd_master_step_dev.restype is C.c_int
    assert list(lib.rn_sgd_hparams_set.argtypes) == [vp, f32, f32, f32, f32, C.c_int, C.c_int64, vp]
    assert list(lib.rn_sgd_master_step_dev.argtypes) == [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    # the by-value entry is what it was
    assert list(lib.rn_sgd_master_step.argtypes) == [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, f32, f32, f32, f32, C.c_int, C.c_int,
                                                     vp, vp, vp, vp]
    # argument checks come before any launch (no GPU is touched)
    assert lib.rn_sgd_hparams_set(None, 0.1, 0.9, 0.0, 0.0, 0, -1, None) != 0
    assert lib.rn_sgd_master_step_dev(None, None, None, None, None, 0, 0, 1, 1, None, None, None, None, None) != 0


def test_block_layout_constant_matches_the_header():
    from pytorch_retinanet_amd import optim
    header = open(os.path.join(ROOT, "include", "retinanet_hip.h")).read()
    assert int(re.search(r"#define\s+RN_SGD_HPARAMS\s+(\d+)", header).group(1)) == optim.RN_SGD_HPARAMS == 8
    words = {name: int(i) for i, name in re.findall(r"word (\d)\s+[fi]32 (\w+)", header[header.index("RN_SGD_HPARAMS 32-bit words"):][:1200])}
    assert words == {"lr": 0, "momentum": 1, "dampening": 2, "weight_decay": 3, "nesterov": 4, "steps": 5, "first": 6}
    assert optim._SHP_STEPS == words["steps"]
    assert int(re.search(r"#define\s+RN_ABI_VERSION\s+(\d+)", header).group(1)) == 10


def test_constructor_validation_and_defaults():
    from pytorch_retinanet_amd.optim import MasterSGD
    default, cap = MasterSGD(_params(), lr=0.1, momentum=0.9), MasterSGD(_params(), lr=0.1, momentum=0.9, capturable=True)
    assert not default.capturable and not getattr(default, "_rn_device_hparams", False)
    assert cap.capturable and cap._rn_device_hparams is True and not getattr(MasterSGD, "_rn_device_hparams", False)
    assert default.defaults == cap.defaults and "capturable" not in cap.defaults
    assert cap._rn_master_weights and cap._step_supports_amp_scaling and cap._rn_grad_clip and cap._rn_weight_ema
    with pytest.raises(TypeError):
        MasterSGD(_params(), 0.1, 0.9, 0.0, 0.0, False, None, True)     # keyword-only
    with pytest.raises(TypeError, match="bool"):
        MasterSGD(_params(), capturable="yes")
    for bad in (dict(lr=-1.0), dict(momentum=-0.1), dict(weight_decay=-1.0), dict(lr=float("nan")), dict(lr=torch.tensor(0.1)),
                dict(dampening=float("inf")), dict(lr=1e39)):
        with pytest.raises(ValueError):
            MasterSGD(_params(), capturable=True, **bad)
    for kw in (dict(momentum=0.0, nesterov=True), dict(momentum=0.9, dampening=0.1, nesterov=True)):
        with pytest.raises(ValueError, match="Nesterov"):
            MasterSGD(_params(), capturable=True, **kw)
    assert MasterSGD(_params(), capturable=True, max_grad_norm=1.0).grad_clip.max_norm == 1.0


def test_structural_changes_raise_and_rewritable_values_do_not():
    "The check sync_device_hparams() and step() run for every group, on a group whose block exists (recorded here by hand: no GPU)."
    from pytorch_retinanet_amd.optim import MasterSGD
    opt = MasterSGD(_params(), lr=0.1, momentum=0.9, capturable=True)
    g = opt.param_groups[0]
    opt._structure[0] = (True, False)                                   # what the first step records: buffers, no nesterov
    g.update(lr=0.01, momentum=0.5, dampening=0.2, weight_decay=1e-3)
    assert opt._hparams(0, g) == (0.01, 0.5, 0.2, 1e-3, 0)
    g["momentum"] = 0.0                                                 # legal with buffers
    assert opt._hparams(0, g)[1] == 0.0
    g.update(momentum=0.9, dampening=0.0, nesterov=True)
    with pytest.raises(ValueError, match="nesterov"):
        opt._hparams(0, g)
    g.update(nesterov=False, lr=-1.0)
    with pytest.raises(ValueError, match="lr"):
        opt._hparams(0, g)
    plain = MasterSGD(_params(), lr=0.1, capturable=True)
    plain._structure[0] = (False, False)
    plain.param_groups[0]["momentum"] = 0.9
    with pytest.raises(ValueError, match="momentum"):
        plain._hparams(0, plain.param_groups[0])
    on = MasterSGD(_params(), lr=0.1, momentum=0.9, nesterov=True, capturable=True)
    on._structure[0] = (True, True)
    on.param_groups[0]["nesterov"] = False
    with pytest.raises(ValueError, match="nesterov"):
        on._hparams(0, on.param_groups[0])
    # the CPU groups of this test have no block: the sync skips them, in either mode
    opt.param_groups[0]["lr"] = 0.1
    opt.sync_device_hparams()
    MasterSGD(_params(), lr=0.1).sync_device_hparams()
    assert opt._blocks == {} and opt.group_steps() == [0]


def _conf(capturable):
    import pytorch_retinanet_amd as P
    conf = P.load_hparams()
    conf.model.update(backbone_kind="resnet18", pretrained=False, num_classes=5, min_size=128, max_size=160)
    conf.optimizer.class_name = "pytorch_retinanet_amd.optim.MasterSGD"
    conf.optimizer.params = {"lr": 1e-2, "momentum": 0.9, "weight_decay": 1e-4}
    if capturable is not None:
        conf.optimizer.params["capturable"] = capturable
    conf.scheduler.class_name = "torch.optim.lr_scheduler.LambdaLR"
    conf.scheduler.params = {"lr_lambda": lambda s: min(1.0, (s + 1) / 10)}
    conf.scheduler.interval, conf.scheduler.monitor = "step", None
    return conf


@pytest.mark.parametrize("capturable", [None, False, True])
def test_hparams_capturable_reaches_the_constructor(capturable):
    import pytorch_retinanet_amd as P
    from pytorch_retinanet_amd.optim import MasterSGD
    m = P.RetinaNetModel(_conf(capturable))
    opts, scheds = m.configure_optimizers()
    assert isinstance(opts[0], MasterSGD) and opts[0].capturable == bool(capturable)
    assert bool(getattr(opts[0], "_rn_device_hparams", False)) == bool(capturable)
    assert scheds[0]["interval"] == "step" and opts[0].param_groups[0]["lr"] == pytest.approx(1e-3)


def test_signature_ignores_the_hyperparameters_in_capturable_mode_only():
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    from pytorch_retinanet_amd.optim import MasterSGD
    net = torch.nn.Conv2d(3, 4, 1)
    images = [torch.zeros(3, 16, 16)]
    targets = [{"boxes": torch.zeros(2, 4), "labels": torch.zeros(2, dtype=torch.int64)}]
    keys = {}
    for capturable in (False, True):
        opt = MasterSGD(net.parameters(), lr=1e-2, momentum=0.9, capturable=capturable)
        step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16)
        before = step._signature(images, targets)
        opt.param_groups[0].update(lr=5e-3, momentum=0.8, weight_decay=1e-3, dampening=0.1)
        keys[capturable] = (before, step._signature(images, targets))
    assert keys[True][0] == keys[True][1] and keys[False][0] != keys[False][1]
    assert ((1e-2, 0.9, 0.0, 0.0, False),) in keys[False][0]             # the default mode's key holds the by-value tuple, as before


def test_simple_trainer_admits_step_schedulers_for_the_flag_only():
    """SimpleTrainer.fit's ``capturable`` condition keys on the optimizer INSTANCE's ``_rn_device_hparams``: evaluated here on the
    attributes it reads, for a per-step scheduler, with and without the flag (the whole fit: test_master_sgd_capturable_gpu.py)."""
    from pytorch_retinanet_amd.optim import MasterSGD
    src = open(os.path.join(ROOT, "pytorch_retinanet_amd", "model.py")).read()
    assert 'getattr(optimizer, "_rn_device_hparams", False)' in src
    schedulers = [{"interval": "step"}]
    for capturable in (False, True):
        optimizer = MasterSGD(_params(), lr=0.1, momentum=0.9, capturable=capturable)
        admits = bool(getattr(optimizer, "_rn_device_hparams", False)
                      or not any(s["interval"] == "step" and "monitor" not in s for s in schedulers))
        assert admits == capturable


def test_cpu_step_is_refused_and_state_dict_is_torch_format():
    from pytorch_retinanet_amd.optim import MasterSGD
    net = torch.nn.Conv2d(3, 4, 1)
    opt = MasterSGD(net.parameters(), lr=1e-2, momentum=0.9, capturable=True)
    sd = opt.state_dict()
    assert sd["state"] == {} and sd["param_groups"][0]["params"] == [0, 1]
    torch.optim.SGD(net.parameters(), lr=0.5).load_state_dict(sd)       # torch takes the format as it is
    net(torch.rand(1, 3, 2, 2)).sum().backward()
    with pytest.raises(TypeError, match="CUDA"):
        opt.step()
    assert opt._blocks == {}
    # a by-value checkpoint with unequal counts in one group is refused before anything is written
    z = torch.zeros_like
    state = {0: {"momentum_buffer": z(net.weight), "steps": 3}, 1: {"momentum_buffer": z(net.bias), "steps": 4}}
    with pytest.raises(RuntimeError, match="different numbers of steps"):
        opt.load_state_dict({"state": state, "param_groups": [dict(opt.param_groups[0], params=[0, 1])]})
    with pytest.raises(ValueError, match="maximize"):
        opt.load_state_dict({"state": {}, "param_groups": [dict(opt.param_groups[0], params=[0, 1], maximize=True)]})
