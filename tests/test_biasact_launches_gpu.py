"""GPU: which native entry points ``biasact`` calls, and how often, for the head, the FPN group and the backbone 3x3 paths at the
default switches.  The counts are a property of the host code (which kernel serves which product, what rides in whose epilogue):
they change only when a launch is added, dropped or rerouted."""
from collections import Counter

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class _Recorder:
    "Forwards every attribute of the bound library; counts the calls of everything that is not a size query."

    def __init__(self, lib):
        self._lib, self.calls = lib, Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name.endswith(("_bytes", "_tiles")):
            return fn

        def call(*a, **k):
            self.calls[name] += 1
            return fn(*a, **k)
        return call

    def take(self) -> Counter:
        got, self.calls = self.calls, Counter()
        return got


@pytest.fixture
def rec():
    from pytorch_retinanet_amd import biasact
    biasact._DW_TABLE.clear()
    biasact.invalidate_dgrad_weights()
    real = biasact.lib
    biasact.lib = r = _Recorder(real)
    try:
        yield r
    finally:
        biasact.lib = real


def _x(C, h, w, N=2):
    return torch.randn(N, C, h, w, device=DEV).to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)


def test_head_on_the_canvas(rec):
    from pytorch_retinanet_amd.layers import RetinaNetHead
    torch.manual_seed(1)
    head = RetinaNetHead(256, 256, 9, 6, 0.01).to(DEV).to(memory_format=torch.channels_last)
    feats = [_x(256, h, w) for h, w in ((16, 20), (8, 10), (4, 5), (2, 3), (1, 2))]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = head.forward_levels(feats)
        loss = sum((t.float() ** 2).sum() for t in out["cls_levels"]) + sum((t.float() ** 2).sum() for t in out["bbox_levels"])
    fwd = rec.take()
    print("head forward", dict(fwd))
    assert fwd == Counter({"rn_canvas_pack": 1, "rn_conv3x3_canvas_batched_ex": 4, "rn_conv3x3_canvas_to_levels": 2})
    loss.backward()
    torch.cuda.synchronize()
    bwd = rec.take()
    print("head backward", dict(bwd))
    assert bwd == Counter({
        # the two output convs: flipped weight, data gradient with the top tower layer's ReLU backward in its epilogue, bias gradient
        "rn_conv3x3_levels_dgrad_weight": 2, "rn_conv3x3_levels_to_canvas_relu": 2, "rn_colsum_rows": 2,
        # weight gradients: class output on the gathering kernel, box output on the narrow kernel over a scattered 64-channel canvas
        "rn_conv3x3_levels_wgrad": 1, "rn_conv3x3_wgrad_narrow": 1,
        # four paired tower layers: flipped weights, data gradient (three carry the ReLU backward of the layer below, the first sums
        # the two towers into the shared input), weight gradient; no rn_bias_act_backward anywhere
        "rn_conv3x3_dgrad_weight_batched": 4, "rn_conv3x3_canvas_dgrad_relu_batched": 3, "rn_conv3x3_canvas_sum2": 1,
        "rn_conv3x3_canvas_wgrad_batched": 4,
        # the box gradient's scatter and the unpack of the canvas gradient
        "rn_canvas_pack": 2})
    assert all(f.grad is not None for f in feats) and all(p.grad is not None for n, p in head.named_parameters())


def test_fpn_dense_group(rec):
    from pytorch_retinanet_amd import biasact
    torch.manual_seed(2)
    convs = [torch.nn.Conv2d(256, 256, 3, 1, padding=1).to(DEV).to(memory_format=torch.channels_last) for _ in range(3)]
    xs = [_x(256, h, w) for h, w in ((8, 10), (4, 5), (2, 3))]
    assert biasact.dense_group_fusable(xs, convs)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        ys = biasact.dense_conv_group(xs, convs)
    fwd = rec.take()
    print("fpn forward", dict(fwd))
    assert fwd == Counter({"rn_conv3x3_dense_batched": 1})
    sum((y.float() ** 2).sum() for y in ys).backward()
    torch.cuda.synchronize()
    bwd = rec.take()
    print("fpn backward", dict(bwd))
    assert bwd == Counter({"rn_conv3x3_dgrad_weight_batched": 1, "rn_conv3x3_dense_batched": 1, "rn_conv3x3_dense_wgrad_batched": 1,
                           "rn_colsum_rows": 3})
    assert all(x.grad is not None for x in xs) and all(c.weight.grad is not None and c.bias.grad is not None for c in convs)


def _bf16_conv(C):
    return torch.nn.Conv2d(C, C, 3, 1, padding=1, bias=False).to(DEV).to(torch.bfloat16).to(memory_format=torch.channels_last)


def test_conv2_256(rec):
    from pytorch_retinanet_amd import biasact
    torch.manual_seed(3)
    conv, x = _bf16_conv(256), _x(256, 8, 10)
    assert biasact.conv3x3_bwd_fusable(conv, x)
    y = biasact.conv3x3_mfma_bwd(conv, x)
    fwd = rec.take()
    print("conv2 forward", dict(fwd))
    assert fwd == Counter({"rn_conv3x3_dense_batched": 1})
    (y.float() ** 2).sum().backward()
    torch.cuda.synchronize()
    bwd = rec.take()
    print("conv2 backward", dict(bwd))
    assert bwd == Counter({"rn_conv3x3_dgrad_weight_batched": 1, "rn_conv3x3_dense_batched": 1, "rn_conv3x3_dense_wgrad_batched": 1})
    assert x.grad is not None and conv.weight.grad is not None


@pytest.mark.parametrize("C,kernel", [(64, "rn_conv3x3_narrow_forward"), (128, "rn_conv3x3_dense_band"), (512, "rn_conv3x3_dense_splitk")])
def test_conv3x3_dgrad_fwd(rec, C, kernel):
    "Forward and data gradient on the same forward kernel (narrow / band / split-K), the weight gradient on the narrow kernel."
    from pytorch_retinanet_amd import biasact
    torch.manual_seed(4)
    conv, x = _bf16_conv(C), _x(C, 8, 10)
    assert biasact.conv3x3_dgrad_fwd_fusable(conv, x)
    if C == 512:
        assert biasact.dense_splitk_bytes(x, conv.weight) > 0
    y = biasact.conv3x3_dgrad_fwd(conv, x)
    fwd = rec.take()
    print(C, "forward", dict(fwd))
    assert fwd == Counter({kernel: 1})
    (y.float() ** 2).sum().backward()
    torch.cuda.synchronize()
    bwd = rec.take()
    print(C, "backward", dict(bwd))
    assert bwd == Counter({"rn_conv3x3_dgrad_weight_batched": 1, kernel: 1, "rn_conv3x3_wgrad_narrow": 1})
    assert x.grad is not None and conv.weight.grad is not None
