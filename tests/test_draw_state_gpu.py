"""GPU: the state-block codec on device blocks, and per augmentation the rule its shared plumbing (``augment._DrawStream``) keeps: a
setting changed after K device draws is written into the SAME block, the device counter -- which only the device advanced -- is kept,
and the next device draw is the Python restatement at that counter with the new setting.  Block I/O and single-wave kernels: the
smallest shapes suffice (B = 3 images of 8 x 8, one box each); B = 65 is past the 64 images of one launch elsewhere in the file."""
import numpy as np
import pytest
import torch

from test_draw_state import BOXES, HW, LAYOUTS, MAX_SIZE, VALUES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 23


# ---- the codec --------------------------------------------------------------------------------------------------------
@LAYOUTS
def test_new_read_and_single_field_writes_on_the_device(layout):
    from pytorch_retinanet_amd import draw_state
    a, b = VALUES[layout.name]
    block = draw_state.new(layout, torch.device(DEV), **a)
    assert block.device == torch.device(DEV) == draw_state.check(layout, block) and block.numel() == layout.nbytes
    assert draw_state.read(layout, block) == tuple(a.values())
    ptr = block.data_ptr()
    for k, name in enumerate(layout.fields):
        draw_state.write(layout, block, **{name: b[name]})
        assert draw_state.read(layout, block) == tuple(list(b.values())[:k + 1] + list(a.values())[k + 1:]), name
    assert block.data_ptr() == ptr
    if layout.nbytes == 24:
        assert block[20:].tolist() == [0, 0, 0, 0]                                    # the reserved word: zeroed by new, never written


def test_write_refuses_a_stream_capture():
    "The values would be baked into the graph.  (The capture holds one draw, as a captured step does.)"
    from pytorch_retinanet_amd import draw_state, ops
    block = draw_state.new(draw_state.HFLIP, torch.device(DEV), seed=1, counter=0, p=0.5)
    ops.hflip_draw(block, 3)                                                           # (warm-up off the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        ops.hflip_draw(block, 3)
        with pytest.raises(RuntimeError, match="inside a stream capture"):
            draw_state.write(draw_state.HFLIP, block, p=1.0)
    assert draw_state.read(draw_state.HFLIP, block) == (1, 1, 0.5)


# ---- per class: K device draws, one setting changed, the next draw ---------------------------------------------------
def _stage(B):
    "B images of 8 x 8 in an arena, one box each in packed GT."
    from pytorch_retinanet_amd import ops
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(B)
    staged = ops.image_stage([torch.rand(3, 8, 8, generator=g).to(dev) for _ in range(B)], ops.StagedImages.empty(B, 64, dev))
    gt = ops.gt_stage([BOXES[0].to(dev)] * B, [torch.ones((1,), dtype=torch.int64, device=dev)] * B, ops.PackedGT.empty(B, 1, dev))
    return staged, gt


def _one_step(v):
    "one fp32 step of the value (the tolerance the ShiftScaleRotate docstring states for host against device matrices)"
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def _settled(obj, draw_dev, change, want_after):
    "Two device draws, ``change(obj)``, then: the counter, the block and the third draw."
    draw_dev(obj), draw_dev(obj)
    block, ptr = obj._block, obj._block.data_ptr()
    assert block is not None and block.device == torch.device(DEV)
    change(obj)
    assert obj.counter == 2                                                            # the device's, kept by the write
    assert obj._block is block and block.data_ptr() == ptr
    got = draw_dev(obj)
    assert obj.counter == 3
    return got, want_after(obj)


def test_flip_p_changes_in_the_same_block():
    from pytorch_retinanet_amd.augment import RandomHorizontalFlip
    got, want = _settled(RandomHorizontalFlip(p=0.0, seed=SEED), lambda o: o.next_flags(len(HW), torch.device("cuda")),
                         lambda o: setattr(o, "p", 1.0), lambda o: o.draw(2, len(HW)))
    assert got.tolist() == [int(f) for f in want] == [1, 1, 1]                         # (p was 0: a block rebuilt or not written gives zeros)


def test_short_side_sizes_change_in_the_same_block():
    from pytorch_retinanet_amd.augment import RandomShortSide
    ss = RandomShortSide((8, 12, 16), seed=SEED)
    (sizes, ratios), want = _settled(ss, lambda o: o.next_sizes(HW, MAX_SIZE, torch.device(DEV)), lambda o: setattr(o, "sizes", (10,)),
                                     lambda o: o.draw(2, HW, MAX_SIZE))
    assert sizes.tolist() == [list(s) for s in want] == [[10, 10]] * 3                  # (10 was no candidate before)
    assert ratios.tolist() == [v for r in ss.ratios(HW, want) for v in r]
    assert ss.canvas_short == 16 and ss.sizes == (10,)


def test_color_jitter_p_changes_in_the_same_block():
    from pytorch_retinanet_amd.augment import ColorJitter
    images = [torch.rand(3, 8, 8, device=DEV) for _ in HW]
    coef, want = _settled(ColorJitter(brightness=0.4, contrast=(0.5, 1.5), hue=0.1, p=0.0, seed=SEED), lambda o: o.next_coef(images),
                          lambda o: setattr(o, "p", 1.0), lambda o: o.draw(2, len(HW)))
    raw = coef.cpu().numpy()
    got = [(tuple(float(v) for v in r[:4]), int(r[5:6].view(np.int32)[0])) for r in raw]
    assert got == want and all(order != 0xFFFF for _, order in got)                    # (p was 0: every order was 0xFFFF)


def test_bbox_crop_p_changes_in_the_same_block():
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.augment import BBoxSafeRandomCrop
    staged, gt = _stage(len(HW))
    crop = BBoxSafeRandomCrop(p=0.0, seed=SEED)
    _, want = _settled(crop, lambda o: ops.bbox_crop_staged(o, staged, gt), lambda o: setattr(o, "p", 1.0), lambda o: o.draw(2, HW, BOXES))
    assert [tuple(r) for r in crop.rect.tolist()] == want != [(0, 0, 8, 8)] * 3           # (p was 0: nothing was cropped)


def test_shift_scale_rotate_p_changes_in_the_same_block():
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.augment import AffineCoefs, ShiftScaleRotate
    staged, gt = _stage(len(HW))
    ssr = ShiftScaleRotate(p=0.0, seed=SEED)
    _, want = _settled(ssr, lambda o: ops.shift_scale_rotate_staged(o, staged, gt), lambda o: setattr(o, "p", 1.0), lambda o: o.draw(2, HW, BOXES))
    got = AffineCoefs.from_device(ssr.coef)
    assert got.applied == want.applied and any(want.applied)                           # (p was 0: nothing was applied)
    for g, w in ((got.m, want.m), (got.inv, want.inv)):
        assert (np.abs(g.astype(np.float64) - w.astype(np.float64)) <= _one_step(w)).all(), (g, w)


# ---- the shared advance kernel: one call, whatever B ------------------------------------------------------------------
def test_bbox_crop_of_65_images_advances_the_counter_once():
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.augment import BBoxSafeRandomCrop
    staged, gt = _stage(65)
    crop = BBoxSafeRandomCrop(p=0.7, seed=SEED)
    ops.bbox_crop_staged(crop, staged, gt)
    assert crop.counter == 1
    assert [tuple(r) for r in crop.rect.tolist()] == crop.draw(0, [(8, 8)] * 65, [BOXES[0]] * 65)


def test_shift_scale_rotate_of_65_images_advances_the_counter_once():
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.augment import AffineCoefs, ShiftScaleRotate
    staged, gt = _stage(65)
    ssr = ShiftScaleRotate(p=0.7, seed=SEED)
    ops.shift_scale_rotate_staged(ssr, staged, gt)
    assert ssr.counter == 1
    assert AffineCoefs.from_device(ssr.coef).applied == ssr.draw(0, [(8, 8)] * 65, [BOXES[0]] * 65).applied
