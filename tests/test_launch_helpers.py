"""CPU: the host-side launch helpers (``_launch``) -- the identity rule of ``as_cl`` and the get-or-grow rule of ``scratch``."""
import torch

from pytorch_retinanet_amd import _launch

CPU = torch.device("cpu")


def test_as_cl_returns_the_tensor_itself_when_nothing_has_to_change():
    t = torch.randn(2, 8, 3, 5).contiguous(memory_format=torch.channels_last)
    assert _launch.cl(t) and _launch.as_cl(t) is t and _launch.as_cl(t, torch.float32) is t
    h = _launch.as_cl(t, torch.bfloat16)
    assert h is not t and h.dtype == torch.bfloat16 and _launch.cl(h) and torch.equal(h, t.to(torch.bfloat16))
    n = torch.randn(2, 8, 3, 5)                                   # NCHW-contiguous: a copy, same values
    c = _launch.as_cl(n)
    assert not _launch.cl(n) and c is not n and _launch.cl(c) and torch.equal(c, n)
    assert not _launch.cl(torch.randn(8, 3, 5))                   # channels-last is a property of 4-D tensors


def test_scratch_keeps_a_buffer_until_a_call_needs_more():
    _launch._SCRATCH.clear()
    try:
        a = _launch.scratch("a", CPU, 7, 100, floor=256)
        assert a.dtype == torch.uint8 and a.numel() == 256                                  # a new buffer: max(need, floor)
        assert _launch.scratch("a", CPU, 7, 200, floor=256) is a and _launch.scratch("a", CPU, 7, 256) is a
        b = _launch.scratch("a", CPU, 7, 257)
        assert b is not a and b.numel() == 257 and _launch.scratch("a", CPU, 7, 10, floor=4096) is b   # the floor never grows a live buffer
        assert _launch.scratch("b", CPU, 7, 10) is not b and _launch.scratch("a", CPU, 8, 10) is not b  # one per name and per stream
        assert _launch.scratch("a", CPU, 7, 1) is b
    finally:
        _launch._SCRATCH.clear()


def test_pointer_and_int_arrays():
    t = torch.zeros(4)
    p = _launch.ptr_array([t, None])
    assert len(p) == 2 and p[0] == t.data_ptr() and not p[1]
    assert list(_launch.int_array([3, 5.0])) == [3, 5]
