"""Host-side helpers every kernel wrapper needs before it can launch: which stream, is the layout the kernel's, pointer / int
arrays for the batched entry points, a page of zeros, and per-(device, stream) scratch buffers."""
import ctypes as C
from typing import Dict, Optional

import torch
from torch import Tensor


def cl(t: Tensor) -> bool:
    return t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last)


def as_cl(t: Tensor, dtype: Optional[torch.dtype] = None) -> Tensor:
    """``t`` as a channels-last tensor of ``dtype`` (default: its own) -- ``t`` ITSELF when it already is one: gradients handed from
    one kernel to the next are recognised by ``data_ptr()`` and ``_version`` (``biasact.TowerLink``)."""
    dtype = t.dtype if dtype is None else dtype
    return t if (t.dtype == dtype and cl(t)) else t.to(dtype).contiguous(memory_format=torch.channels_last)


def stream_on(dev: torch.device) -> int:
    "The current stream's handle on ``dev``, which becomes the current device if it is not (no context switch otherwise)."
    if dev.index != torch.cuda.current_device():
        torch.cuda.set_device(dev)
    return torch.cuda.current_stream().cuda_stream


def ptr_array(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() if t is not None else 0 for t in ts])


def int_array(v):
    return (C.c_int * len(v))(*[int(i) for i in v])


_ZEROS: Dict[int, Tensor] = {}


def zero_page(dev: torch.device) -> Tensor:
    z = _ZEROS.get(dev.index)
    if z is None:
        z = _ZEROS[dev.index] = torch.empty((256,), dtype=torch.uint8, device=dev).fill_(0)
    return z


_SCRATCH: Dict[tuple, Tensor] = {}


def scratch(name: str, dev: torch.device, stream: int, need: int, floor: int = 0) -> Tensor:
    """The u8 buffer ``name`` of (device, stream), at least ``need`` bytes: kept until a call needs more, then replaced by one of
    max(need, floor) bytes.  Kernels of one stream are ordered, so a buffer is dead when the call that used it has run; a captured
    graph holds its pointer, so buffers of different names never share storage."""
    key = (name, dev.index, stream)
    ws = _SCRATCH.get(key)
    if ws is None or ws.numel() < need:
        ws = _SCRATCH[key] = torch.empty((max(need, floor),), dtype=torch.uint8, device=dev)
    return ws
