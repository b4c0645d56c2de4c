"""The device state blocks of the train-time draws (``augment.py``): one table per struct of ``include/retinanet_hip.h`` and one codec.

Every block begins ``{u64 seed; i64 counter; ...}`` and is a uint8 tensor that a draw kernel reads and whose counter it advances.  A
captured graph holds the block's address, and after a replay the device counter is ahead of anything the host knows, so a block is
never rebuilt from host values: ``write`` sends the fields it is given, one host->device copy each, and leaves every other byte alone.
``csrc/augment.hip`` and ``csrc/affine.hip`` assert these sizes and offsets against the structs at build time.  Needs torch only.
"""
import struct
from typing import Callable, Dict, NamedTuple, Tuple

import torch
from torch import Tensor

COLOR_OPS = ("brightness", "contrast", "saturation", "hue")        # the operation ids 0..3 (rn_color_coef)
COLOR_IDENTITY = (1.0, 1.0, 1.0, 0.0)    # the factor that leaves the pixel alone (what a disabled operation's range holds)
SHORT_SIDE_MAX = 16                      # candidate short sides a block holds (RN_SHORT_SIDE_MAX)


class Field(NamedTuple):
    offset: int
    fmt: str                             # struct format of the field's bytes
    encode: Callable                     # value -> the tuple ``struct.pack(fmt, ...)`` takes
    decode: Callable                     # the tuple ``struct.unpack`` gives -> value


def _field(offset: int, fmt: str, encode: Callable = None, decode: Callable = None) -> Field:
    "A scalar (``<f``) or a vector (``<4f``) of ints or floats, unless the field brings its own encode / decode."
    conv = float if fmt[-1] == "f" else int
    if struct.calcsize(fmt) == struct.calcsize("<" + fmt[-1]):
        return Field(offset, fmt, encode or (lambda v: (conv(v),)), decode or (lambda t: t[0]))
    return Field(offset, fmt, encode or (lambda v: tuple(conv(x) for x in v)), decode or tuple)


class Layout(NamedTuple):
    name: str                            # the struct's name
    nbytes: int
    fields: Dict[str, Field]             # in the struct's order; ``read`` returns them in this order


def _sizes_encode(sizes) -> Tuple[int, ...]:
    "n, the reserved word and all 16 entries, padded with the last value (the kernel indexes sizes[] below n only)."
    sizes = [int(v) for v in sizes]
    if not 1 <= len(sizes) <= SHORT_SIDE_MAX or min(sizes) <= 0:
        raise ValueError(f"need 1..{SHORT_SIDE_MAX} positive short sides, got {sizes}")
    return (len(sizes), 0, *sizes, *[sizes[-1]] * (SHORT_SIDE_MAX - len(sizes)))


def _sizes_decode(t) -> Tuple[int, ...]:
    return tuple(t[2:2 + max(0, min(t[0], SHORT_SIDE_MAX))])


_HEAD = {"seed": _field(0, "<Q", lambda v: (int(v) & (2 ** 64 - 1),)), "counter": _field(8, "<q")}
HFLIP = Layout("rn_hflip_state", 24, {**_HEAD, "p": _field(16, "<f")})                       # bytes 20..24 are reserved: zero
BBOX_CROP = Layout("rn_bbox_crop_state", 24, HFLIP.fields)
SHORT_SIDE = Layout("rn_short_side_state", 24 + 4 * SHORT_SIDE_MAX,
                    {**_HEAD, "sizes": _field(16, f"<ii{SHORT_SIDE_MAX}i", _sizes_encode, _sizes_decode)})
COLOR_JITTER = Layout("rn_color_jitter_state", 56, {**_HEAD, "p": _field(16, "<f"), "lo": _field(20, "<4f"), "hi": _field(36, "<4f"),
                                                    "enabled_mask": _field(52, "<i", lambda v: (int(v) & 0xF,))})
AFFINE = Layout("rn_affine_state", 56, {**_HEAD, "p": _field(16, "<f"), "min_visibility": _field(20, "<f"),
                                        "lo": _field(24, "<4f"), "hi": _field(40, "<4f")})       # lo / hi of (angle, scale, dx, dy)
LAYOUTS = (HFLIP, SHORT_SIDE, COLOR_JITTER, BBOX_CROP, AFFINE)
# ``brightness`` / ``contrast``: (lo, hi) of beta and of alpha - 1 -- the struct's blo, bhi and clo, chi; ``by_max``: ref = 1, else the mean
BRIGHTNESS_CONTRAST = Layout("rn_brightness_contrast_state", 40,
                             {**_HEAD, "p": _field(16, "<f"), "brightness": _field(20, "<2f"), "contrast": _field(28, "<2f"),
                              "by_max": _field(36, "<i", lambda v: (1 if v else 0,), lambda t: bool(t[0]))})


def check(layout: Layout, block: Tensor) -> torch.device:
    "``block`` is a whole, 8-byte aligned uint8 block of this layout -> its device."
    if block.dtype != torch.uint8 or block.numel() != layout.nbytes or block.data_ptr() % 8:
        raise ValueError(f"block must be an {layout.name} made by draw_state.new()")
    return block.device


def new(layout: Layout, dev: torch.device, **fields) -> Tensor:
    "A new block on ``dev`` holding ``fields`` -- all of the layout's -- and zeros elsewhere; outside any capture."
    if fields.keys() != layout.fields.keys():
        raise TypeError(f"{layout.name} takes {tuple(layout.fields)}, got {tuple(fields)}")
    block = torch.zeros((layout.nbytes,), dtype=torch.uint8, device=dev)
    write(layout, block, **fields)
    return block


def write(layout: Layout, block: Tensor, **fields) -> None:
    """Overwrite the given fields of a block (the others keep their device values): one host->device copy per field on the current
    stream, so they are ordered with the draws around them.  Not inside a capture: the values would be baked into the graph."""
    check(layout, block)
    if block.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{layout.name} written inside a stream capture")
    for name, value in fields.items():
        f = layout.fields[name]
        raw = struct.pack(f.fmt, *f.encode(value))
        block[f.offset:f.offset + len(raw)].copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))


def read(layout: Layout, block: Tensor) -> tuple:
    "The fields of a block in the layout's order: one device->host copy (synchronises)."
    check(layout, block)
    raw = block.cpu().numpy().tobytes()
    return tuple(f.decode(struct.unpack_from(f.fmt, raw, f.offset)) for f in layout.fields.values())
