"""GPU: the pure data-movement kernels that every captured step and every gradient exchange run and no other test calls directly:
``rn_copy_many``, ``rn_cast_many_to_f32``, ``rn_transpose_many``, ``rn_conv3x3_levels_dgrad_weight`` (csrc/optim.hip),
``rn_scale_inplace_batched`` (csrc/loss.hip) and ``rn_conv3x3_dgrad_weight_batched`` / ``_many`` (csrc/conv.hip).

Their references are exact, so every comparison is ``torch.equal`` (on integer views: NaN patterns count), each on purpose through the
aligned vector path, the scalar path chosen by pointer alignment, the tail, a second table and a second pass of the capped grid.
Every destination is a slice of a larger sentinel-filled allocation whose rest is checked after the call."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64
RN_EINVAL, RN_EALIGN, RN_EUNSUPPORTED = -1, -2, -4


def _lib():
    from pytorch_retinanet_amd._lib import lib
    return lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _vp(values):
    return (C.c_void_p * max(len(values), 1))(*values)


def _i64(values):
    return (C.c_int64 * max(len(values), 1))(*values)


class _Guarded:
    """``n`` elements (``view``, at address ``ptr``: an empty view has none of its own) starting ``lead`` elements into a fresh
    allocation ``buf`` filled with ``fill``, PAD more behind them."""

    def __init__(self, n, dtype, fill, lead=0):
        self.buf = torch.full((lead + n + PAD,), fill, dtype=dtype, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.view, self.fill, self.lead, self.n = self.buf[lead:lead + n], fill, lead, n
        self.ptr = self.buf.data_ptr() + lead * self.buf.element_size()

    def rest_untouched(self):
        "Everything of the allocation outside the view still holds the fill."
        return bool((self.buf[:self.lead] == self.fill).all()) and bool((self.buf[self.lead + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


# ---- rn_copy_many -----------------------------------------------------------------------------------------------------------------
# one pass of the capped grid moves 512 x 256 x 16 bytes = 2 097 152; 6 291 461 is three passes and a tail of 5
COPY_BYTES = [0, 1, 15, 16, 17, 4095, 2_097_152, 2_097_153, 6_291_461]


class _CopyCase:
    "``nbytes`` random source bytes ``src_off`` bytes past a 16-byte boundary, a guarded destination ``dst_off`` bytes past one"

    def __init__(self, nbytes, src_off, dst_off, gen):
        self.src_buf = torch.randint(0, 256, (src_off + nbytes + 1,), dtype=torch.uint8, device=DEV, generator=gen)
        assert self.src_buf.data_ptr() % 16 == 0
        self.src, self.src_ptr = self.src_buf[src_off:src_off + nbytes], self.src_buf.data_ptr() + src_off
        self.dst = _Guarded(nbytes, torch.uint8, 0xA5, lead=dst_off)

    def exact(self):
        return torch.equal(self.dst.view, self.src) and self.dst.rest_untouched()


def _copy_many(cases, nbytes):
    return _lib().rn_copy_many(_vp([c.src_ptr for c in cases]), _vp([c.dst.ptr for c in cases]), _i64(nbytes), len(cases), _stream())


@pytest.mark.parametrize("src_off,dst_off", [(0, 0), (1, 0), (0, 4), (8, 8), (3, 3)])
def test_copy_many_is_exact_at_every_size_and_alignment(src_off, dst_off):
    "(0, 0): 16-byte vectors and a byte tail; any misalignment of either pointer: the byte path."
    gen = torch.Generator(device=DEV).manual_seed(1)
    cases = [_CopyCase(n, src_off, dst_off, gen) for n in COPY_BYTES]
    assert _copy_many(cases, COPY_BYTES) == 0
    torch.cuda.synchronize()
    for n, c in zip(COPY_BYTES, cases):
        assert c.exact(), (n, src_off, dst_off)


def test_copy_many_splits_130_entries_into_three_tables():
    "64 + 64 + 2 entries, zero-length ones among them (also as the first entry of a table), alignments mixed."
    gen = torch.Generator(device=DEV).manual_seed(2)
    sizes = [(0, 1, 15, 16, 17, 300, 4095)[i % 7] for i in range(130)]
    sizes[64] = 0
    sizes[129] = 70_001
    cases = [_CopyCase(n, (0, 1, 0, 8)[i % 4], (0, 0, 4, 8)[i % 4], gen) for i, n in enumerate(sizes)]
    assert _copy_many(cases, sizes) == 0
    torch.cuda.synchronize()
    for i, c in enumerate(cases):
        assert c.exact(), (i, sizes[i])


def test_copy_many_argument_checks():
    gen = torch.Generator(device=DEV).manual_seed(3)
    c = _CopyCase(4096, 0, 0, gen)
    lib, one = _lib(), _i64([4096])
    assert lib.rn_copy_many(_vp([c.src_ptr]), _vp([c.dst.ptr]), one, 0, _stream()) == 0                     # n = 0: nothing to do
    assert lib.rn_copy_many(_vp([0]), _vp([c.dst.ptr]), one, 1, _stream()) == RN_EINVAL
    assert lib.rn_copy_many(_vp([c.src_ptr]), _vp([0]), one, 1, _stream()) == RN_EINVAL
    assert lib.rn_copy_many(None, _vp([c.dst.ptr]), one, 1, _stream()) == RN_EINVAL
    assert lib.rn_copy_many(_vp([c.src_ptr]), _vp([c.dst.ptr]), _i64([-1]), 1, _stream()) == RN_EINVAL
    assert lib.rn_copy_many(_vp([c.src_ptr]), _vp([c.dst.ptr]), one, -1, _stream()) == RN_EINVAL
    torch.cuda.synchronize()
    assert c.dst.untouched()                                             # none of them wrote


# ---- rn_cast_many_to_f32 ----------------------------------------------------------------------------------------------------------
CAST_DTYPES = [(torch.bfloat16, 1), (torch.float16, 2)]               # (torch dtype, RN_BF16 / RN_F16)


def _patterns(dtype, reps=1):
    "Every 16-bit pattern, in order, ``reps`` times (an aligned fresh allocation)."
    pat = torch.arange(-32768, 32768, dtype=torch.int16, device=DEV).repeat(reps).view(dtype)
    assert pat.data_ptr() % 16 == 0
    return pat


def _cast_many(pat, offs, outs, counts, code):
    "sources: ``counts[i]`` elements from element ``offs[i]`` of ``pat``"
    return _lib().rn_cast_many_to_f32(_vp([pat.data_ptr() + 2 * o for o in offs]), _vp([d.ptr for d in outs]), _i64(counts), len(outs), code, _stream())


def _assert_widened(dst, src, what):
    "dst == src.float(): bit for bit where that is not NaN (subnormals, +-0 and +-inf included), NaN where it is"
    want = src.float()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(dst), nan), what
    assert torch.equal(_bits(dst)[~nan], _bits(want)[~nan]), what


@pytest.mark.parametrize("dtype,code", CAST_DTYPES, ids=["bf16", "f16"])
def test_cast_many_widens_every_16_bit_pattern(dtype, code):
    """All 65 536 patterns through the vector path (both pointers on 16 bytes) and through the scalar path twice: the source one element
    past a 16-byte boundary, and the destination on 4 bytes but not on 16."""
    pat, n = _patterns(dtype, 2), 65536
    offs = [0, 1, 0]
    outs = [_Guarded(n, torch.float32, -77.0), _Guarded(n, torch.float32, -77.0), _Guarded(n, torch.float32, -77.0, lead=1)]
    assert [d.ptr % 16 for d in outs] == [0, 0, 4]
    assert int(torch.isnan(pat[:n].float()).sum()) > 0 and _bits(pat[:n]).unique().numel() == n
    assert _cast_many(pat, offs, outs, [n] * 3, code) == 0
    torch.cuda.synchronize()
    for k, (o, d) in enumerate(zip(offs, outs)):
        _assert_widened(d.view, pat[o:o + n], (str(dtype), k))
        assert d.rest_untouched(), k


@pytest.mark.parametrize("dtype,code", CAST_DTYPES, ids=["bf16", "f16"])
def test_cast_many_counts_table_split_and_a_second_grid_pass(dtype, code):
    """70 tensors (tables of 64 + 6) of 0, 1, 7, 8 and 9 elements at mixed alignments, then one of 2 000 003 elements: above the
    512 x 256 x 8 elements of one pass of the capped grid, with a tail of 3."""
    pat = _patterns(dtype, 32)
    offs, outs, counts = [], [], []
    for i in range(70):
        offs.append(8 * 37 * i + (1 if i % 3 == 1 else 0))             # (every third source one element past a 16-byte boundary)
        counts.append((0, 1, 7, 8, 9)[i % 5])
        outs.append(_Guarded(counts[-1], torch.float32, -77.0, lead=1 if i % 3 == 2 else 0))
    offs.append(0)
    counts.append(2_000_003)
    outs.append(_Guarded(counts[-1], torch.float32, -77.0))
    assert _cast_many(pat, offs, outs, counts, code) == 0
    torch.cuda.synchronize()
    for i, (o, n, d) in enumerate(zip(offs, counts, outs)):
        _assert_widened(d.view, pat[o:o + n], (str(dtype), i, n))
        assert d.rest_untouched(), (i, n)


def test_cast_many_argument_checks():
    pat = _patterns(torch.bfloat16)
    d = _Guarded(8, torch.float32, -77.0)
    lib, one = _lib(), _i64([8])
    assert lib.rn_cast_many_to_f32(_vp([pat.data_ptr()]), _vp([d.ptr]), one, 1, 0, _stream()) == RN_EUNSUPPORTED          # an fp32 source
    assert lib.rn_cast_many_to_f32(_vp([pat.data_ptr() + 1]), _vp([d.ptr]), one, 1, 1, _stream()) == RN_EALIGN            # an odd address
    assert lib.rn_cast_many_to_f32(_vp([pat.data_ptr()]), _vp([d.ptr + 2]), one, 1, 1, _stream()) == RN_EALIGN
    assert lib.rn_cast_many_to_f32(_vp([0]), _vp([d.ptr]), one, 1, 1, _stream()) == RN_EINVAL
    assert lib.rn_cast_many_to_f32(_vp([pat.data_ptr()]), _vp([d.ptr]), _i64([-1]), 1, 1, _stream()) == RN_EINVAL
    torch.cuda.synchronize()
    assert d.untouched()


# ---- rn_transpose_many ------------------------------------------------------------------------------------------------------------
# single rows and columns, ragged tiles, whole tiles, and (2048, 544): 64 x 17 = 1088 tiles, above the 1024-block cap of the grid
TR_SHAPES = [(1, 1), (1, 33), (33, 1), (31, 65), (32, 32), (64, 256), (256, 64), (2048, 544)]
TR_FILL = 0x5A5A


def _transpose_many(src_ptrs, dst_ptrs, shapes, n):
    return _lib().rn_transpose_many(_vp(src_ptrs), _vp(dst_ptrs), (C.c_int * len(shapes))(*[r for r, _ in shapes]),
                                    (C.c_int * len(shapes))(*[c for _, c in shapes]), n, _stream())


def test_transpose_many_sixteen_matrices_in_one_launch():
    gen = torch.Generator(device=DEV).manual_seed(4)
    shapes = TR_SHAPES + TR_SHAPES[:7] + [(31, 65)]
    assert len(shapes) == 16
    srcs = [torch.randint(-32768, 32768, s, dtype=torch.int16, device=DEV, generator=gen) for s in shapes]
    outs = [_Guarded(r * c, torch.int16, TR_FILL) for r, c in shapes]
    assert _transpose_many([s.data_ptr() for s in srcs], [d.ptr for d in outs], shapes, 16) == 0
    torch.cuda.synchronize()
    for (r, c), src, d in zip(shapes, srcs, outs):
        assert torch.equal(d.view.view(c, r), src.t().contiguous()), (r, c)
        assert d.rest_untouched(), (r, c)


def test_transpose_many_argument_checks():
    shapes = [(32, 32)] * 17
    srcs = [torch.zeros(s, dtype=torch.int16, device=DEV) for s in shapes]
    outs = [_Guarded(32 * 32, torch.int16, TR_FILL) for _ in shapes]
    sp, dp = [s.data_ptr() for s in srcs], [d.ptr for d in outs]
    assert _transpose_many(sp, dp, shapes, 17) == RN_EINVAL                      # more than the table holds: there is no second launch
    assert _transpose_many(sp, dp, shapes, 0) == RN_EINVAL
    assert _transpose_many(sp[:2], [dp[0], sp[1]], shapes[:2], 2) == RN_EINVAL   # src == dst
    torch.cuda.synchronize()
    assert all(d.untouched() for d in outs)


# ---- rn_scale_inplace_batched -----------------------------------------------------------------------------------------------------
SCALE_MAX_TENSORS = 16                                              # csrc/loss.hip: the table of one launch


@pytest.mark.parametrize("dtype,fill", [(torch.float32, -77.0), (torch.bfloat16, 123.0), (torch.float16, 123.0)], ids=["f32", "bf16", "f16"])
def test_scale_inplace_batched_equals_scale_inplace_bit_for_bit(dtype, fill):
    "40 tensors of 1, 7 and 4097 elements, a scale each (1.0, the device-side no-op, among them): launches of 16 + 16 + 8."
    from pytorch_retinanet_amd import ops
    gen = torch.Generator(device=DEV).manual_seed(5)
    count = 2 * SCALE_MAX_TENSORS + 8
    sizes = [(1, 7, 4097)[i % 3] for i in range(count)]
    scales = [torch.tensor([1.0 if i % 5 == 4 else 0.37 + 0.61 * i], device=DEV) for i in range(count)]
    outs = [_Guarded(n, dtype, fill) for n in sizes]
    for d in outs:
        d.view.copy_(torch.randn(d.n, device=DEV, generator=gen) + 2.0)
    before = [d.view.clone() for d in outs]
    want = [ops.scale_inplace(b.clone(), s) for b, s in zip(before, scales)]
    ops.scale_inplace_batched([d.view for d in outs], scales)
    torch.cuda.synchronize()
    for i, (d, r, b) in enumerate(zip(outs, want, before)):
        assert torch.equal(_bits(d.view), _bits(r)) and d.rest_untouched(), (i, sizes[i])
        assert torch.equal(_bits(d.view), _bits(b)) == (i % 5 == 4), i          # (a scale of 1 changes nothing, any other does)
    # the C entry point itself takes one table and refuses more
    n = SCALE_MAX_TENSORS + 1
    rc = _lib().rn_scale_inplace_batched(_vp([d.ptr for d in outs[:n]]), _i64(sizes[:n]), _vp([s.data_ptr() for s in scales[:n]]), n,
                                         {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[dtype], _stream())
    torch.cuda.synchronize()
    assert rc == RN_EINVAL and all(torch.equal(_bits(d.view), _bits(r)) for d, r in zip(outs, want))


# ---- the data-gradient weights ------------------------------------------------------------------------------------------------------
DW_FILL = 123.0


def _weight(cout, cin, seed=0):
    """[cout, cin, 3, 3] bf16, channels-last, filled with arange reinterpreted as 16-bit patterns (period 65 521, a prime: no two slots
    within reach of one another hold the same pattern, so every output slot's origin is identifiable)."""
    n = cout * cin * 9
    v = ((torch.arange(n, dtype=torch.int64, device=DEV) + 7919 * seed) % 65521 - 32768).to(torch.int16).view(torch.bfloat16)
    assert v.data_ptr() % 16 == 0
    return v.view(cout, 3, 3, cin).permute(0, 3, 1, 2)


class _GuardedCL(_Guarded):
    "A guarded bf16 tensor of ``shape`` [N, C, 3, 3] in channels-last memory: ``cl``"

    def __init__(self, shape):
        n, c, h, w = shape
        super().__init__(n * c * h * w, torch.bfloat16, DW_FILL)
        self.cl = self.view.view(n, h, w, c).permute(0, 3, 1, 2)


@pytest.mark.parametrize("cin", [8, 256])
@pytest.mark.parametrize("cout", [8, 9, 15, 36, 45, 64, 65, 720, 810])
def test_levels_dgrad_weight_equals_the_torch_form(cout, cin):
    "rn_conv3x3_levels_dgrad_weight against the torch branch of biasact._dgrad_weight (the one a CPU tensor takes)."
    from pytorch_retinanet_amd import biasact
    w = _weight(cout, cin)
    assert w.is_contiguous(memory_format=torch.channels_last)
    kpad = (cout + 63) // 64 * 64
    out = _GuardedCL((cin, kpad, 3, 3))
    assert _lib().rn_conv3x3_levels_dgrad_weight(w.data_ptr(), out.ptr, cout, cin, kpad, _stream()) == 0
    want = biasact._dgrad_weight(w.cpu())
    assert tuple(want.shape) == (cin, kpad, 3, 3)
    assert torch.equal(_bits(out.cl).cpu(), _bits(want)) and out.rest_untouched()
    via = biasact._dgrad_weight(w)                                      # the wrapper's own launch
    assert via.is_contiguous(memory_format=torch.channels_last) and torch.equal(_bits(via).cpu(), _bits(want))


def _flipped(w):
    return w.flip(2, 3).transpose(0, 1)


def _dw_batched(ws, outs, cout, cin):
    return _lib().rn_conv3x3_dgrad_weight_batched(_vp([w.data_ptr() for w in ws]), _vp([o.ptr for o in outs]), len(ws), cout, cin, _stream())


@pytest.mark.parametrize("cout,cin", [(32, 32), (64, 32), (32, 96)])
def test_dgrad_weight_batched_one_weight_a_full_table_and_five_in_two_calls(cout, cin):
    """The smallest shapes the entry point takes (multiples of 32).  One call holds at most CONV_MAX_PROBLEMS = 4 weights: 1 and 4 in
    one launch each, 5 refused (RN_EINVAL, nothing written), 5 as 4 + 1."""
    ws = [_weight(cout, cin, seed=k) for k in range(5)]
    for group in ([0], [0, 1, 2, 3]):
        outs = [_GuardedCL((cin, cout, 3, 3)) for _ in group]
        assert _dw_batched([ws[k] for k in group], outs, cout, cin) == 0
        torch.cuda.synchronize()
        for k, o in zip(group, outs):
            assert torch.equal(_bits(o.cl), _bits(_flipped(ws[k]))) and o.rest_untouched(), (k, len(group))
    outs = [_GuardedCL((cin, cout, 3, 3)) for _ in ws]
    assert _dw_batched(ws, outs, cout, cin) == RN_EINVAL
    assert _dw_batched(ws[:1], outs[:1], cout + 1, cin) == RN_EUNSUPPORTED
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)
    assert _dw_batched(ws[:4], outs[:4], cout, cin) == 0 and _dw_batched(ws[4:], outs[4:], cout, cin) == 0
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        assert torch.equal(_bits(o.cl), _bits(_flipped(ws[k]))) and o.rest_untouched(), k


def test_dgrad_weight_many_mixes_shapes_and_splits_its_table():
    "(64, 64), (128, 64), (512, 512) and the smallest shapes in one call; then 50 weights: more than the 48 of one launch."
    lib = _lib()
    for shapes in ([(64, 64), (128, 64), (512, 512), (32, 32), (32, 64)], [((32, 32), (64, 32), (32, 64))[i % 3] for i in range(50)]):
        ws = [_weight(co, ci, seed=k) for k, (co, ci) in enumerate(shapes)]
        outs = [_GuardedCL((ci, co, 3, 3)) for co, ci in shapes]
        n = len(ws)
        assert lib.rn_conv3x3_dgrad_weight_many(_vp([w.data_ptr() for w in ws]), _vp([o.ptr for o in outs]), (C.c_int * n)(*[co for co, _ in shapes]),
                                                (C.c_int * n)(*[ci for _, ci in shapes]), n, _stream()) == 0
        torch.cuda.synchronize()
        for k, (w, o) in enumerate(zip(ws, outs)):
            assert torch.equal(_bits(o.cl), _bits(_flipped(w))) and o.rest_untouched(), (k, shapes[k])
