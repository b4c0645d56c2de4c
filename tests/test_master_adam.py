"""CPU suite: the host side of ``optim.MasterAdam`` / ``MasterAdamW`` -- argument validation, the hparams wiring, the
optimizer-capability attributes the graph / exchange / trainer layers key on, and ``CapturedTrainStep``'s signature, which leaves
out the hyperparameters of a device-hparams optimizer while it keeps keying ``MasterSGD`` by its learning rate.
(The numerics against torch.optim.Adam / AdamW are in test_master_adam_gpu.py, -m gpu.)"""
import pytest
import torch


def _params():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3), torch.nn.BatchNorm2d(8)).parameters()


def test_constructor_follows_torch_and_refuses_what_it_does_not_implement():
    from pytorch_retinanet_amd.optim import MasterAdam, MasterAdamW
    a, w = MasterAdam(_params()), MasterAdamW(_params())
    ta, tw = torch.optim.Adam(_params()), torch.optim.AdamW(_params())
    for mine, ref in ((a, ta), (w, tw)):
        for k in ("lr", "betas", "eps", "weight_decay", "amsgrad", "maximize"):
            assert mine.defaults[k] == ref.defaults[k], k
    assert a.defaults["weight_decay"] == 0.0 and w.defaults["weight_decay"] == 1e-2
    for cls in (MasterAdam, MasterAdamW):
        with pytest.raises(ValueError, match="AMSGrad"):
            cls(_params(), amsgrad=True)
        with pytest.raises(ValueError, match="maximize"):
            cls(_params(), maximize=True)
        for bad in (dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(weight_decay=-1.0),
                    dict(betas=(0.9,))):
            with pytest.raises(ValueError):
                cls(_params(), **bad)
    assert MasterAdamW(_params(), betas=[0.8, 0.99]).param_groups[0]["betas"] == (0.8, 0.99)


def test_capability_attributes():
    from pytorch_retinanet_amd.optim import MasterAdam, MasterAdamW, MasterSGD
    for cls in (MasterAdam, MasterAdamW):
        assert cls._rn_master_weights and cls._rn_device_hparams and cls._step_supports_amp_scaling
    assert MasterAdamW._decoupled and not MasterAdam._decoupled
    assert MasterSGD._rn_master_weights and not getattr(MasterSGD, "_rn_device_hparams", False)
    for cls in (torch.optim.SGD, torch.optim.AdamW):
        assert not getattr(cls, "_rn_master_weights", False) and not getattr(cls, "_rn_device_hparams", False)


def test_empty_state_dict_is_torch_format_and_cpu_step_is_refused():
    from pytorch_retinanet_amd.optim import MasterAdamW
    net = torch.nn.Conv2d(3, 4, 1)
    opt = MasterAdamW(net.parameters(), lr=1e-3)
    sd = opt.state_dict()
    assert sd["state"] == {} and sd["param_groups"][0]["params"] == [0, 1]
    torch.optim.AdamW(net.parameters()).load_state_dict(sd)              # torch takes the format as it is
    net(torch.rand(1, 3, 2, 2)).sum().backward()
    with pytest.raises(TypeError, match="CUDA"):
        opt.step()


def test_load_state_dict_refuses_unequal_steps_and_amsgrad():
    from pytorch_retinanet_amd.optim import MasterAdamW
    net = torch.nn.Conv2d(3, 4, 1)
    opt = MasterAdamW(net.parameters())
    z = lambda t: torch.zeros_like(t)
    groups = [dict(opt.param_groups[0], params=[0, 1])]
    state = {0: {"step": torch.tensor(3.0), "exp_avg": z(net.weight), "exp_avg_sq": z(net.weight)},
             1: {"step": torch.tensor(4.0), "exp_avg": z(net.bias), "exp_avg_sq": z(net.bias)}}
    with pytest.raises(RuntimeError, match="different numbers of steps"):
        opt.load_state_dict({"state": state, "param_groups": groups})
    with pytest.raises(ValueError, match="AMSGrad"):
        opt.load_state_dict({"state": {}, "param_groups": [dict(groups[0], amsgrad=True)]})


def test_hparams_class_name_selects_the_master_optimizer():
    import pytorch_retinanet_amd as P
    from pytorch_retinanet_amd.optim import MasterAdamW
    conf = P.load_hparams()
    conf.model.update(backbone_kind="resnet18", pretrained=False, num_classes=5, min_size=128, max_size=160)
    conf.optimizer.class_name = "pytorch_retinanet_amd.optim.MasterAdamW"
    conf.optimizer.params = {"lr": 2e-4, "betas": [0.9, 0.98], "weight_decay": 0.05}
    conf.scheduler.class_name = "torch.optim.lr_scheduler.LambdaLR"
    conf.scheduler.params = {"lr_lambda": lambda s: min(1.0, (s + 1) / 10)}
    conf.scheduler.interval, conf.scheduler.monitor = "step", None
    m = P.RetinaNetModel(conf)
    opts, scheds = m.configure_optimizers()
    opt = opts[0]
    assert isinstance(opt, MasterAdamW) and opt.param_groups[0]["betas"] == (0.9, 0.98)
    assert opt.param_groups[0]["weight_decay"] == 0.05 and scheds[0]["interval"] == "step"
    assert opt.param_groups[0]["lr"] == pytest.approx(2e-5)             # LambdaLR applied its first factor


def _signature_of(opt, net):
    from pytorch_retinanet_amd.graph import CapturedTrainStep
    step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16)
    images = [torch.zeros(3, 16, 16)]
    targets = [{"boxes": torch.zeros(2, 4), "labels": torch.zeros(2, dtype=torch.int64)}]
    return lambda: step._signature(images, targets)


def test_signature_ignores_hyperparameters_of_a_device_hparams_optimizer_only():
    from pytorch_retinanet_amd.optim import MasterAdamW, MasterSGD
    net = torch.nn.Conv2d(3, 4, 1)
    adam = MasterAdamW(net.parameters(), lr=1e-3)
    sig = _signature_of(adam, net)
    before = sig()
    g = adam.param_groups[0]
    g["lr"], g["betas"], g["eps"], g["weight_decay"] = 3e-4, (0.8, 0.9), 1e-6, 0.3
    assert sig() == before
    sgd = MasterSGD(net.parameters(), lr=1e-2, momentum=0.9)
    sig = _signature_of(sgd, net)
    before = sig()
    sgd.param_groups[0]["lr"] = 5e-3
    assert sig() != before
