"""CPU suite: the host side of uint8 image input -- ``rn_image_stage_u8``'s declaration and its argument checks (made-up pointers:
every rejection returns before anything is launched), the definition of the converted value (``float(v) / 255``, ONE correctly
rounded division, and why it is not the product with 1 / 255), the dataset's ``image_dtype="uint8"`` items and the transform on CPU
uint8 lists.  (The kernel, the staged path and whole steps are in test_u8_stage_gpu.py, -m gpu.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table() -> np.ndarray:
    "The definition: the fp32 quotient of every byte by 255 (numpy divides; it does not multiply by a reciprocal)."
    return np.arange(256, dtype=np.float32) / np.float32(255)


# ---- 1. the symbol ------------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_and_declared():
    from pytorch_retinanet_amd import _lib
    header = open(os.path.join(ROOT, "include", "retinanet_hip.h")).read()
    assert int(re.search(r"#define\s+RN_ABI_VERSION\s+(\d+)", header).group(1)) == 10 and _lib.lib.rn_version() == 10
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+rn_image_stage_u8\s*\(([^;]*?)\)\s*;", header, flags=re.S)
    assert m, "rn_image_stage_u8 is not declared"
    assert "rn_image_stage_u8" in _lib.SIGNATURES and hasattr(_lib.lib, "rn_image_stage_u8")
    res, args = _lib.SIGNATURES["rn_image_stage_u8"]
    assert res is C.c_int and len(args) == len(m.group(1).split(",")) == 8


# ---- 2. argument rejections ------------------------------------------------------------------------------------------------------------
def test_argument_rejections():
    from pytorch_retinanet_amd import _lib
    lib = _lib.lib
    EINVAL, EALIGN = -1, -2
    p = 4096                                                         # an aligned non-null "pointer": never dereferenced on these paths
    hw = (C.c_int32 * 2)(8, 12)
    one = (C.c_void_p * 1)(p)
    lay = (C.c_int32 * 1)(1)
    big = 1 << 16
    i32p = C.POINTER(C.c_int32)
    assert lib.rn_image_stage_u8(None, hw, lay, 1, p, big, p, 0) == EINVAL                              # null pointers, one at a time
    assert lib.rn_image_stage_u8(one, i32p(), lay, 1, p, big, p, 0) == EINVAL
    assert lib.rn_image_stage_u8(one, hw, i32p(), 1, p, big, p, 0) == EINVAL
    assert lib.rn_image_stage_u8(one, hw, lay, 1, 0, big, p, 0) == EINVAL
    assert lib.rn_image_stage_u8(one, hw, lay, 1, p, big, 0, 0) == EINVAL
    assert lib.rn_image_stage_u8((C.c_void_p * 1)(0), hw, lay, 1, p, big, p, 0) == EINVAL               # a null image
    assert lib.rn_image_stage_u8(one, hw, lay, 0, p, big, p, 0) == EINVAL                               # B <= 0
    assert lib.rn_image_stage_u8(one, hw, lay, -3, p, big, p, 0) == EINVAL
    assert lib.rn_image_stage_u8(one, hw, lay, 1, p, 0, p, 0) == EINVAL                                 # slot <= 0
    assert lib.rn_image_stage_u8(one, hw, lay, 1, p, -16, p, 0) == EINVAL
    for bad in ((0, 12), (8, 0), (-1, 12), (8, -5)):                                                    # h or w <= 0
        assert lib.rn_image_stage_u8(one, (C.c_int32 * 2)(*bad), lay, 1, p, big, p, 0) == EINVAL, bad
    assert lib.rn_image_stage_u8(one, hw, lay, 1, p, 3 * 8 * 12 - 1, p, 0) == EINVAL                    # 3 h w > slot
    assert lib.rn_image_stage_u8(one, (C.c_int32 * 2)(46341, 46341), lay, 1, p, big, p, 0) == EINVAL    # h w > 2^31: no overflow into "fits"
    assert lib.rn_image_stage_u8(one, (C.c_int32 * 2)(46341, 46341), lay, 1, p, (1 << 31) + 4, p, 0) == EINVAL
    for bad in (2, -1, 255):                                                                            # a layout other than 0 or 1
        assert lib.rn_image_stage_u8(one, hw, (C.c_int32 * 1)(bad), 1, p, big, p, 0) == EINVAL, bad
    # (the second image's arguments are checked like the first's)
    two, hw2 = (C.c_void_p * 2)(p, p + 1), (C.c_int32 * 4)(8, 12, 8, 12)
    assert lib.rn_image_stage_u8(two, hw2, (C.c_int32 * 2)(0, 7), 2, p, big, p, 0) == EINVAL
    assert lib.rn_image_stage_u8((C.c_void_p * 2)(p, 0), hw2, (C.c_int32 * 2)(0, 1), 2, p, big, p, 0) == EINVAL
    assert lib.rn_image_stage_u8(one, hw, lay, 1, p + 4, big, p, 0) == EALIGN                           # the arena needs 16 bytes
    assert lib.rn_image_stage_u8(one, hw, lay, 1, p + 8, big, p, 0) == EALIGN
    assert lib.rn_image_stage_u8(one, hw, lay, 1, p, big, p + 2, 0) == EALIGN                           # in_hw_dev needs 4


# ---- 3. the definition ---------------------------------------------------------------------------------------------------------------
def test_definition_table_on_the_cpu():
    from pytorch_retinanet_amd import ops
    want = _table()
    planes = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16).repeat(3, 1, 1)
    hwc = torch.arange(256, dtype=torch.uint8).reshape(16, 16, 1).repeat(1, 1, 3)
    for im in (planes, hwc.permute(2, 0, 1)):
        got, = ops.images_u8_to_f32([im])
        assert got.dtype == torch.float32 and tuple(got.shape) == (3, 16, 16) and got.is_contiguous()
        for c in range(3):
            assert np.array_equal(got[c].numpy().reshape(-1).view(np.uint32), want.view(np.uint32))
    # the rule is a division: the product with the rounded reciprocal is another function of the byte
    product = np.arange(256, dtype=np.float32) * (np.float32(1) / np.float32(255))
    differ = np.flatnonzero(product.view(np.uint32) != want.view(np.uint32))
    assert len(differ) == 126 and differ[:5].tolist() == [3, 6, 7, 12, 13]
    assert np.abs(product.view(np.int32) - want.view(np.int32)).max() == 1                              # ... in the last bit


def test_cpu_conversion_refusals():
    from pytorch_retinanet_amd import ops
    assert ops.images_u8_to_f32([]) == []
    for bad in (torch.zeros(3, 4, 4), torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(3, 4, dtype=torch.uint8),
                torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(3, 4, 4, dtype=torch.int8)):
        with pytest.raises(ValueError, match="uint8"):
            ops.images_u8_to_f32([torch.zeros(3, 4, 4, dtype=torch.uint8), bad])
    with pytest.raises(ValueError, match="empty"):                                                      # (as on the device)
        ops.images_u8_to_f32([torch.zeros(3, 0, 5, dtype=torch.uint8)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):                                          # staging is a device op
        ops.image_stage_u8([torch.zeros(3, 4, 4, dtype=torch.uint8)], ops.StagedImages(torch.zeros(1, 64), torch.zeros(1, 2, dtype=torch.int32)))


# ---- 4. the dataset ------------------------------------------------------------------------------------------------------------------
def test_dataset_uint8_items(tmp_path):
    from PIL import Image
    from pytorch_retinanet_amd import CSVDetectionDataset, ops
    H, W = 13, 22
    g = np.random.default_rng(5)
    arr = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    arr.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)                                              # every byte value occurs
    Image.fromarray(arr).save(tmp_path / "a.png")
    (tmp_path / "d.csv").write_text("filename,xmin,ymin,xmax,ymax,labels\na.png,1,2,10,11,1\na.png,3,3,20,12,2\n")
    ref_im, ref_t, _ = CSVDetectionDataset(str(tmp_path / "d.csv"))[0]
    ds = CSVDetectionDataset(str(tmp_path / "d.csv"), image_dtype="uint8")
    im, t, idx = ds[0]
    assert im.dtype == torch.uint8 and tuple(im.shape) == (3, H, W) and im.stride() == (1, 3 * W, 3)
    assert np.array_equal(im.permute(1, 2, 0).numpy(), arr)
    assert ref_im.dtype == torch.float32 and tuple(ref_im.shape) == (3, H, W)
    got, = ops.images_u8_to_f32([im])
    assert torch.equal(got, ref_im) and np.array_equal(got.numpy().view(np.uint32), ref_im.contiguous().numpy().view(np.uint32))
    assert torch.equal(t["boxes"], ref_t["boxes"]) and torch.equal(t["labels"], ref_t["labels"]) and int(idx) == 0
    with pytest.raises(ValueError, match="image_dtype"):
        CSVDetectionDataset(str(tmp_path / "d.csv"), image_dtype="float16")
    with pytest.raises(ValueError, match="image_dtype"):                                                # (a transforms callable builds its own tensor)
        CSVDetectionDataset(str(tmp_path / "d.csv"), transforms=lambda im, b, l: (im, b, l), image_dtype="uint8")


def test_hparams_image_dtype_reaches_the_dataset(tmp_path):
    from PIL import Image
    import pytorch_retinanet_amd as P
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(tmp_path / "a.png")
    (tmp_path / "d.csv").write_text("filename,xmin,ymin,xmax,ymax,labels\na.png,1,2,6,7,1\n")
    for dt, want in ((None, torch.float32), ("uint8", torch.uint8)):
        conf = P.load_hparams()
        conf.model.update(backbone_kind="resnet18", pretrained=False, num_classes=3, min_size=32, max_size=64)
        conf.dataset.kind, conf.dataset.trn_paths = "csv", str(tmp_path / "d.csv")
        if dt is not None:
            conf.dataset.image_dtype = dt
        model = P.RetinaNetModel(conf)
        model.prepare_data()
        assert model.trn_ds[0][0].dtype == want


# ---- 5. the transform on CPU uint8 lists -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("training", [True, False])
def test_transform_on_cpu_uint8_lists(training):
    from pytorch_retinanet_amd import ops
    from pytorch_retinanet_amd.transform import GeneralizedRCNNTransform
    tr = GeneralizedRCNNTransform(48, 64, [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]).train(training)
    g = torch.Generator().manual_seed(3)
    u8 = [torch.randint(0, 256, (3, 37, 53), dtype=torch.uint8, generator=g),                           # planes
          torch.randint(0, 256, (40, 31, 3), dtype=torch.uint8, generator=g).permute(2, 0, 1),          # interleaved
          torch.randint(0, 256, (3, 50, 100), dtype=torch.uint8, generator=g)[:, :, ::2]]               # any other strides
    f32 = [(im.to(torch.float32) / 255).contiguous() for im in u8]
    assert all(torch.equal(a, b) for a, b in zip(ops.images_u8_to_f32(u8), f32))

    def tg():
        return [{"boxes": torch.tensor([[2., 3., 20., 30.], [5., 5., 25., 12.]]), "labels": torch.tensor([1, 2])} for _ in u8] if training else None
    want, want_t = tr(f32, tg())
    got, got_t = tr(u8, tg())
    assert got.tensors.dtype == torch.float32 and torch.equal(got.tensors, want.tensors) and got.image_sizes == want.image_sizes
    mixed, mixed_t = tr([u8[0], f32[1], u8[2]], tg())                                                   # uint8 members converted one by one
    assert torch.equal(mixed.tensors, want.tensors)
    if training:
        for a, b, c in zip(got_t, want_t, mixed_t):
            assert torch.equal(a["boxes"], b["boxes"]) and torch.equal(c["boxes"], b["boxes"])
    assert float(want.tensors.abs().max()) < 3.0                                                        # (normalised [0, 1] values, not 0..255)
