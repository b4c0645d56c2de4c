"""CPU: the state-block codec (``draw_state``: the five layout tables, pack / unpack on a CPU uint8 tensor) and the contract that
``augment._DrawStream`` keeps for the five augmentations while no device block exists: reseed, set_rank, state_dict round trips and
the host draw that advances the counter by exactly one."""
import struct

import numpy as np
import pytest
import torch

from pytorch_retinanet_amd import augment, draw_state
from pytorch_retinanet_amd.augment import BBoxSafeRandomCrop, ColorJitter, RandomHorizontalFlip, RandomShortSide, ShiftScaleRotate

M64 = 2 ** 64 - 1
# two sets of values per layout (every float exact in fp32): A fills a block, B overwrites it field by field
VALUES = {
    "rn_hflip_state": (dict(seed=M64 - 2, counter=7, p=0.25), dict(seed=11, counter=2 ** 40 + 3, p=0.75)),
    "rn_bbox_crop_state": (dict(seed=5, counter=0, p=1.0), dict(seed=M64, counter=9, p=0.5)),
    "rn_short_side_state": (dict(seed=3, counter=1, sizes=(8, 12, 16)), dict(seed=4, counter=6, sizes=tuple(range(1, 17)))),
    "rn_color_jitter_state": (dict(seed=17, counter=4, p=0.5, lo=(0.5, 0.75, 1.0, -0.25), hi=(1.5, 1.25, 1.0, 0.25), enabled_mask=0xB),
                              dict(seed=18, counter=5, p=0.125, lo=(0.25, 1.0, 0.5, 0.0), hi=(2.0, 1.0, 1.5, 0.0), enabled_mask=0x5)),
    "rn_affine_state": (dict(seed=2, counter=3, p=0.5, min_visibility=0.25, lo=(-45.0, 0.5, -0.0625, -0.0625), hi=(45.0, 1.5, 0.0625, 0.0625)),
                        dict(seed=9, counter=8, p=1.0, min_visibility=0.0, lo=(-10.0, 1.0, -0.5, -0.5), hi=(10.0, 2.0, 0.5, 0.5))),
}
LAYOUTS = pytest.mark.parametrize("layout", draw_state.LAYOUTS, ids=lambda l: l.name)


def _bytes(block):
    return block.numpy().tobytes()


def _span(f):
    return f.offset, f.offset + struct.calcsize(f.fmt)


# ---- the layout tables ------------------------------------------------------------------------------------------------
def test_there_are_five_layouts_and_ops_aliases_their_sizes():
    from pytorch_retinanet_amd import ops
    assert sorted(l.name for l in draw_state.LAYOUTS) == sorted(VALUES)
    assert (ops.HFLIP_STATE_BYTES, ops.SHORT_SIDE_STATE_BYTES, ops.COLOR_JITTER_STATE_BYTES, ops.BBOX_CROP_STATE_BYTES,
            ops.AFFINE_STATE_BYTES) == (24, 88, 56, 24, 56) == tuple(l.nbytes for l in draw_state.LAYOUTS)
    assert ops.COLOR_OPS is augment.COLOR_OPS is draw_state.COLOR_OPS and ops.SHORT_SIDE_MAX is augment.SHORT_SIDE_MAX is draw_state.SHORT_SIDE_MAX


@LAYOUTS
def test_fields_are_ordered_disjoint_and_inside_the_block(layout):
    spans = [_span(f) for f in layout.fields.values()]
    assert layout.nbytes % 8 == 0 and spans[0][0] == 0 and spans[-1][1] <= layout.nbytes
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))                      # ordered, no overlap
    names = list(layout.fields)
    assert names[:2] == ["seed", "counter"]
    assert layout.fields["seed"][:2] == (0, "<Q") and layout.fields["counter"][:2] == (8, "<q")
    assert list(VALUES[layout.name][0]) == names                                     # (the values below cover every field)


@LAYOUTS
def test_new_then_read_gives_the_values_and_zero_padding(layout):
    a = VALUES[layout.name][0]
    block = draw_state.new(layout, torch.device("cpu"), **a)
    assert block.dtype == torch.uint8 and block.numel() == layout.nbytes and draw_state.check(layout, block) == torch.device("cpu")
    assert draw_state.read(layout, block) == tuple(a.values())
    raw, covered = _bytes(block), set()
    for f in layout.fields.values():
        covered.update(range(*_span(f)))
    assert all(raw[i] == 0 for i in range(layout.nbytes) if i not in covered)
    if layout.nbytes == 24:
        assert raw[20:24] == bytes(4)                                                # the flip's / the crop's reserved word
    with pytest.raises(TypeError):
        draw_state.new(layout, torch.device("cpu"), seed=1, counter=0)               # a block is never made half filled


@LAYOUTS
def test_writing_one_field_leaves_every_other_byte_alone(layout):
    a, b = VALUES[layout.name]
    block = torch.full((layout.nbytes,), 0xAB, dtype=torch.uint8)                    # (padding included: a write touches its field only)
    draw_state.write(layout, block, **a)
    for i, (name, f) in enumerate(layout.fields.items()):
        before = _bytes(block)
        draw_state.write(layout, block, **{name: b[name]})
        after, (lo, hi) = _bytes(block), _span(f)
        assert after[:lo] == before[:lo] and after[hi:] == before[hi:], name
        want = list(b.values())[:i + 1] + list(a.values())[i + 1:]
        assert draw_state.read(layout, block) == tuple(want), name
    assert draw_state.read(layout, block) == tuple(b.values())


def test_the_seed_is_masked_to_64_bits_and_the_mask_to_four():
    block = draw_state.new(draw_state.HFLIP, torch.device("cpu"), seed=2 ** 64 + 5, counter=-1, p=0.5)
    assert draw_state.read(draw_state.HFLIP, block) == (5, -1, 0.5)
    a = dict(VALUES["rn_color_jitter_state"][0], enabled_mask=0x1F)
    assert draw_state.read(draw_state.COLOR_JITTER, draw_state.new(draw_state.COLOR_JITTER, torch.device("cpu"), **a))[5] == 0xF


def test_short_sides_are_one_field_padded_with_the_last_value_and_trimmed_to_n():
    L = draw_state.SHORT_SIDE
    block = draw_state.new(L, torch.device("cpu"), seed=1, counter=2, sizes=(8, 12, 16))
    draw_state.write(L, block, sizes=(32,))
    assert draw_state.read(L, block) == (1, 2, (32,))
    assert struct.unpack_from("<ii16i", _bytes(block), 16) == (1, 0) + (32,) * 16    # n, the reserved word, 16 entries
    for bad in ((), tuple(range(1, 18)), (8, 0), (-4,)):
        with pytest.raises(ValueError):
            draw_state.write(L, block, sizes=bad)
    assert draw_state.read(L, block) == (1, 2, (32,))


def test_check_refuses_what_is_not_a_whole_aligned_block():
    good = torch.zeros((64,), dtype=torch.uint8)
    assert good.data_ptr() % 8 == 0
    for bad in (good[:24].to(torch.int8), good[:23], good[:25], good[4:28]):
        with pytest.raises(ValueError, match="block must be an rn_hflip_state"):
            draw_state.check(draw_state.HFLIP, bad)
    with pytest.raises(ValueError, match="rn_affine_state"):
        draw_state.write(draw_state.AFFINE, good[:24], p=0.5)
    with pytest.raises(ValueError, match="rn_short_side_state"):
        draw_state.read(draw_state.SHORT_SIDE, good[:56])


# ---- the shared contract of the five classes, without a device block --------------------------------------------------
HW = [(8, 8)] * 3
BOXES = [torch.tensor([[1.0, 1.0, 5.0, 6.0]]) for _ in HW]
MAX_SIZE = 64


def _coefs(c):
    return c.m.tolist(), c.inv.tolist(), c.applied


# class -> (constructor for (seed, p), the entry that draws one batch on the host -> something comparable)
CLASSES = {
    "flip": (lambda seed, p: RandomHorizontalFlip(p=p, seed=seed), lambda o: o.next_flags(len(HW), "cpu").tolist()),
    "short_side": (lambda seed, p: RandomShortSide((8, 12, 16) if p < 1 else (16,), seed=seed),
                   lambda o: [t.tolist() for t in o.next_sizes(HW, MAX_SIZE, "cpu")]),
    "color_jitter": (lambda seed, p: ColorJitter(brightness=0.4, contrast=(0.5, 1.5), hue=0.1, p=p, seed=seed), lambda o: o.next_draw(len(HW))),
    "bbox_crop": (lambda seed, p: BBoxSafeRandomCrop(p=p, seed=seed), lambda o: o.next_rects(HW, BOXES)),
    "shift_scale_rotate": (lambda seed, p: ShiftScaleRotate(p=p, seed=seed), lambda o: _coefs(o.next_coefs(HW, BOXES))),
}
EACH = pytest.mark.parametrize("kind", list(CLASSES))


@EACH
def test_reseed_and_set_rank(kind):
    make, _ = CLASSES[kind]
    o = make(M64 - 1, 0.5)
    assert (o.base_seed, o.seed, o.counter, o._block) == (M64 - 1, M64 - 1, 0, None)
    o.reseed(2 ** 64 + 9, 41)
    assert (o.seed, o.counter, o.base_seed) == (9, 41, M64 - 1)
    o.set_rank(3)
    assert (o.seed, o.counter) == ((M64 - 1 + 3) % 2 ** 64, 41)                      # base_seed + rank, wrapped; the counter kept
    o.reseed(6)
    assert (o.seed, o.counter) == (6, 0)


@EACH
def test_the_host_draw_advances_the_counter_by_exactly_one(kind):
    make, draw = CLASSES[kind]
    o = make(21, 0.5)
    o.reseed(21, 5)
    for k in range(3):
        draw(o)
        assert (o.counter, o._counter, o._block) == (6 + k, 6 + k, None)
    twin = make(21, 0.5)
    twin.reseed(21, 8)
    assert draw(o) == draw(twin) and o.counter == twin.counter == 9                  # the draw follows the counter, not the object


@EACH
def test_state_dict_round_trip_continues_the_same_stream(kind):
    make, draw = CLASSES[kind]
    o = make(33, 0.5)
    draw(o), draw(o)
    state = o.state_dict()
    assert list(state)[:2] == ["seed", "counter"] and (state["seed"], state["counter"]) == (33, 2)
    assert all(type(state[k]) is int for k in ("seed", "counter"))
    if kind != "short_side":
        assert type(state["p"]) is float and state["p"] == 0.5
    fresh = make(1, 1.0)                                                             # another seed, p and (short side) candidates
    fresh.load_state_dict(state)
    assert fresh.state_dict() == state and fresh.counter == 2 and fresh.base_seed == 1
    assert draw(fresh) == draw(o) and fresh.counter == o.counter == 3


def test_state_dict_keys_and_value_types_are_what_checkpoints_hold():
    assert RandomHorizontalFlip(0.5, seed=1).state_dict() == {"seed": 1, "counter": 0, "p": 0.5}
    assert BBoxSafeRandomCrop(0.5, seed=1).state_dict() == {"seed": 1, "counter": 0, "p": 0.5}
    assert ShiftScaleRotate(p=0.5, seed=1).state_dict() == {"seed": 1, "counter": 0, "p": 0.5}
    s = RandomShortSide((8, 12), seed=1).state_dict()
    assert s == {"seed": 1, "counter": 0, "sizes": [8, 12]} and type(s["sizes"]) is list
    c = ColorJitter(brightness=0.5, hue=(-0.25, 0.25), p=0.5, seed=1).state_dict()
    assert c == {"seed": 1, "counter": 0, "p": 0.5, "brightness": [0.5, 1.5], "contrast": None, "saturation": None, "hue": [-0.25, 0.25]}
    assert list(c) == ["seed", "counter", "p", "brightness", "contrast", "saturation", "hue"]


def test_p_is_checked_once_for_all_four():
    for make in (CLASSES[k][0] for k in ("flip", "color_jitter", "bbox_crop", "shift_scale_rotate")):
        o = make(0, 0.3)
        assert o.p == float(np.float32(0.3))                                          # the fp32 value the device compares with
        o.p = 1
        assert o.p == 1.0 and type(o.p) is float
        for bad in (-0.1, 1.5, float("nan")):
            with pytest.raises(ValueError):
                o.p = bad
            with pytest.raises(ValueError):
                make(0, bad)
        assert o.p == 1.0
    assert not hasattr(RandomShortSide((8,)), "p")
