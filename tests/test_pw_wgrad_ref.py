"""CPU: the float64 weight-gradient reference of ``pw_wgrad_ref.py`` on its own -- against torch's float64 convolution backward, its
operand prologues against integer arithmetic, and the operand generator's promises (exact small integers in bf16 and fp16, every
partial sum below 2^24) that let ``test_pw_wgrad_gpu.py`` ask the kernel for equality."""
import numpy as np
import pytest
import torch

import pw_wgrad_ref as R

DTYPES = [torch.bfloat16, torch.float16]


@pytest.mark.parametrize("nimg", [1, 2, 3])
@pytest.mark.parametrize("taps,stride", [(1, 1), (1, 2), (9, 1), (9, 2)])
@pytest.mark.parametrize("H,W", [(7, 9), (5, 3), (1, 5)])
def test_reference_equals_the_float64_convolution_backward(nimg, taps, stride, H, W):
    N, Cin, k = 5, 6, (3 if taps == 9 else 1)
    geo, pad = R.geometry(nimg, H, W, taps, stride)
    gen = torch.Generator().manual_seed(100 * nimg + 10 * taps + stride)
    x = torch.randn((nimg, Cin, H, W), dtype=torch.float64, generator=gen)
    g = torch.randn((nimg, N, geo.Ho, geo.Wo), dtype=torch.float64, generator=gen)
    w = torch.zeros((N, Cin, k, k), dtype=torch.float64)
    want = torch.ops.aten.convolution_backward(g, x, w, None, [stride, stride], [pad, pad], [1, 1], False, [0, 0], 1, [False, True, False])[1]
    got = R.wgrad_ref(g.permute(0, 2, 3, 1).reshape(geo.M, N), x.permute(0, 2, 3, 1).reshape(geo.rows, Cin), taps, stride, pad, geo)
    got = got.view(N, k, k, Cin).permute(0, 3, 1, 2)
    assert got.shape == want.shape
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    assert err <= 1e-12 * scale, (err, scale)
    # ... and the sum of magnitudes that the rounding bound is built from: the same gather on |g|, |x|
    want_abs = torch.ops.aten.convolution_backward(g.abs(), x.abs(), w, None, [stride, stride], [pad, pad], [1, 1], False, [0, 0], 1,
                                                   [False, True, False])[1]
    got_abs = R.abs_terms_sum(g.permute(0, 2, 3, 1).reshape(geo.M, N), x.permute(0, 2, 3, 1).reshape(geo.rows, Cin), taps, stride, pad, geo)
    assert float((got_abs.view(N, k, k, Cin).permute(0, 3, 1, 2) - want_abs).abs().max()) <= 1e-12 * float(want_abs.abs().max())


def test_tap_rows_marks_every_border():
    "Hand-worked positions: 3 x 3 / stride 2 / pad 1 over two 5 x 3 images, and the valid-tap count of every pixel of a 4 x 4 image."
    geo, pad = R.geometry(2, 5, 3, 9, 2)
    rows, ok = R.tap_rows(geo, 9, 2, pad, "cpu")
    assert (geo.Ho, geo.Wo) == (3, 2) and rows.shape == (9, 12)
    m = 6 + 1 * 2 + 1                   # image 1, ho 1, wo 1: the window covers y = 1..3, x = 1..3, and x = 3 is outside
    assert [bool(v) for v in ok[:, m]] == [True, True, False] * 3
    assert [int(r) for r in rows[:, m]] == [15 + 3 + 1, 15 + 3 + 2, 0, 15 + 6 + 1, 15 + 6 + 2, 0, 15 + 9 + 1, 15 + 9 + 2, 0]
    assert not bool(ok[0, 0]) and bool(ok[4, 0]) and int(rows[4, 0]) == 0 and int(rows[4, 6]) == 15     # the centre tap of each image's first row
    geo1, _ = R.geometry(1, 4, 4, 9, 1)
    _, ok1 = R.tap_rows(geo1, 9, 1, 1, "cpu")
    assert [int(v) for v in ok1.sum(0)] == [4, 6, 6, 4, 6, 9, 9, 6, 6, 9, 9, 6, 4, 6, 6, 4]     # corners, edges, interior


@pytest.mark.parametrize("dtype", DTYPES)
def test_prologue_restatements_on_integers(dtype):
    "Integer operands and coefficients: every fp32 step is exact, so the restatements must equal plain int64 arithmetic."
    rng = np.random.default_rng(5)
    M, Cc = 37, 64
    gi, zi = rng.integers(-3, 4, (M, Cc)), rng.integers(-3, 4, (M, Cc))
    a, k0, k1 = rng.integers(1, 3, Cc), rng.integers(-1, 2, Cc), rng.integers(-1, 2, Cc)
    fa, fb = rng.integers(1, 3, Cc), rng.integers(-1, 2, Cc)
    mask = rng.random((M, Cc)) > 0.4
    t = lambda v, dt=dtype: torch.from_numpy(np.ascontiguousarray(v)).to(dt)
    coef3, fwd = t(np.concatenate([a, k0, k1]), torch.float32), t(np.concatenate([fa, fb]), torch.float32)
    bits = R.pack_bits(torch.from_numpy(mask))
    assert torch.equal(R.unpack_bits(bits, M, Cc), torch.from_numpy(mask))
    assert int(bits[0]) == sum(int(mask[0, j]) << j for j in range(8))
    for mode, keep in ((0, np.ones_like(mask)), (2, zi * fa + fb >= 1), (3, mask)):
        want = a * (gi * keep) + k1 * zi + k0
        got = R.pro_bn_bwd(t(gi), t(zi), coef3, mode, dtype, fwd, bits)
        assert got.dtype == torch.float64 and np.array_equal(got.numpy(), want.astype(np.float64)), mode
    want = np.maximum(gi * fa + fb, 0)
    assert np.array_equal(R.pro_affine_relu(t(gi), fwd, dtype).numpy(), want.astype(np.float64))


@pytest.mark.parametrize("dtype", DTYPES)
def test_prologue_restatements_round_once_to_the_element_type(dtype):
    "Real coefficients: the result is a value of the 16-bit type, within half a unit in the last place of the float64 expression."
    gen = torch.Generator().manual_seed(9)
    M, Cc = 50, 64
    g, z = torch.randn((M, Cc), generator=gen).to(dtype), torch.randn((M, Cc), generator=gen).to(dtype)
    coef3 = torch.cat([torch.rand(Cc, generator=gen) + 0.5, torch.randn(Cc, generator=gen) * 0.05, torch.randn(Cc, generator=gen) * 0.05])
    fwd = torch.cat([torch.rand(Cc, generator=gen) + 0.5, torch.randn(Cc, generator=gen) * 0.3])
    got = R.pro_bn_bwd(g, z, coef3, 2, dtype, fwd)
    assert torch.equal(got, got.to(dtype).double())
    keep = (z.double() * fwd[:Cc].double() + fwd[Cc:].double()) > 0
    want = coef3[:Cc].double() * (g.double() * keep) + coef3[2 * Cc:].double() * z.double() + coef3[Cc:2 * Cc].double()
    # (half an ulp of the rounding + the two fp32 roundings before it)
    assert bool(((got - want).abs() <= R.half_ulp(want, dtype) * (1 + 2.0 ** -10)).all())
    got = R.pro_affine_relu(g, fwd, dtype)
    want = torch.clamp(g.double() * fwd[:Cc].double() + fwd[Cc:].double(), min=0)
    assert torch.equal(got, got.to(dtype).double()) and bool((got >= 0).all())
    assert bool(((got - want).abs() <= R.half_ulp(want, dtype) * (1 + 2.0 ** -10)).all())


def test_half_ulp():
    one = torch.tensor([1.0, 1.5, 0.75, 3.0, 0.0], dtype=torch.float64)
    assert R.half_ulp(one, torch.bfloat16).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -9, 2.0 ** -7, 2.0 ** -134]
    assert R.half_ulp(one, torch.float16).tolist() == [2.0 ** -11, 2.0 ** -11, 2.0 ** -12, 2.0 ** -10, 2.0 ** -25]


def test_case_table_is_consistent_and_covers_what_it_claims():
    "The S / KT columns (256 CUs) against launch_of; between them the cases reach every tile, both grid forms, S % 8 == 0 and != 0 on the XCD map, KT 2 and >= 3, a ragged last tile and a short last split."
    names = [c.name for c in R.CASES]
    assert len(set(names)) == len(names)
    seen = []
    for c in R.CASES:
        L = R.launch_of(c, c.S)
        assert L.tile == c.tile and L.KT == c.KT >= c.depth >= 2 and L.xcd == c.xcd, (c.name, L)
        assert (L.S - 1) * L.KT < L.ktiles <= L.S * L.KT, (c.name, L)              # S is what ceil(ktiles / KT) gives back
        if c.s_mod8_zero is not None:
            assert c.xcd and (L.S % 8 == 0) == c.s_mod8_zero, (c.name, L)
        if c.short_last is not None:
            assert (L.last_tiles < L.KT) == c.short_last, (c.name, L)
        assert 9 * c.M < 2 ** 24 and c.M % 64 != 0
        seen.append(L)
    assert {L.tile for L in seen} == {(128, 128), (256, 64), (128, 64), (64, 256), (64, 128), (64, 64)}
    assert {L.xcd for L in seen} == {True, False}
    assert {L.S % 8 == 0 for L in seen if L.xcd} == {True, False}
    assert any(L.KT == 2 for L in seen) and any(L.KT >= 3 and L.xcd for L in seen) and any(L.KT >= 3 and not L.xcd for L in seen)
    assert any(L.last_tiles < L.KT and L.ragged for L in seen) and any(L.last_tiles == L.KT and L.ragged for L in seen)
    assert any(L.gy == 1 for L in seen) and any(L.gy > 64 for L in seen)
    # the two prologue pairs the trunk reaches (pwconv._BottleneckFn.backward: conv3's weight gradient at mid widths 64 and 128)
    assert {(c.tile, c.gpro, c.xpro) for c in R.CASES if c.gpro is not None and c.xpro} == {((128, 64), 3, True), ((128, 128), 3, True)}
    assert {c.gpro for c in R.CASES} == {None, 0, 2, 3}


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_integer_operands_are_exact_in_both_types_and_sums_stay_below_2_to_24(case):
    ops = {dt: R.operands(case, dt, integer=True) for dt in DTYPES}
    a, b = ops[torch.bfloat16], ops[torch.float16]
    assert a.g.shape == (case.M, case.N) and a.x.shape == (case.geo.rows, case.Cin)
    for u, v in zip(a, b):                  # the same numbers in both types
        assert (u is None) == (v is None)
        if u is not None:
            assert torch.equal(u.double(), v.double())
    for dt in DTYPES:
        gt, xt = R.transformed(case, ops[dt], dt)
        for t, peak in ((gt, 10 if case.gpro is not None else 3), (xt, 7 if case.xpro else 3)):
            assert torch.equal(t, t.round()) and float(t.abs().max()) <= peak
            assert torch.equal(t.to(torch.bfloat16).double(), t) and torch.equal(t.to(torch.float16).double(), t)
        assert R.operand_peak(case, gt, xt) < 2 ** 24
        if case.xpro:
            assert bool((xt >= 0).all()) and bool((xt == 0).any()) and bool((xt > 0).any())
    if case.gpro == 3:                      # the mask is neither all open nor all shut
        frac = float(R.unpack_bits(a.bits, case.M, case.N).float().mean())
        assert 0.5 < frac < 0.7
    if case.gpro == 2:
        keep = R._fma32(a.z.float(), a.fwd[:case.N], a.fwd[case.N:]) > R.ALIVE[torch.bfloat16]
        assert 0.2 < float(keep.float().mean()) < 0.8
