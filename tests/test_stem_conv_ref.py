"""CPU: ``stem_conv_ref.py`` on its own -- the float64 references against torch's float64 convolution and its weight gradient on every
geometry the GPU cases use (the shapes derived for 256 CUs), the restated schedules of csrc/stem.hip worked by hand for 256 and 304 CUs
(every tile and every stage owned exactly once), and the operand generators' promises that let ``test_stem_conv_exact_gpu.py`` ask the
kernels for equality."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stem_conv_ref as R


def _geometries():
    g = {(1, 1, 1), (1, 7, 7), (2, 2, 3), (1, 8, 36), (3, 5, 1)}
    g |= {R.forward_shape(c, 256) for c in R.FCASES + [R.REAL_FWD]}
    g |= {R.wgrad_shape(c, 256) for c in R.WCASES + [R.REAL_WGRAD]}
    return sorted(g)


@pytest.mark.parametrize("B,H,W", _geometries())
def test_references_equal_the_float64_convolution_and_its_weight_gradient(B, H, W):
    Cout = 5
    gen = torch.Generator().manual_seed(7 * B + 3 * H + W)
    x = torch.randn((B, 3, H, W), dtype=torch.float64, generator=gen)
    w = torch.randn((Cout, 3, 7, 7), dtype=torch.float64, generator=gen)
    Ho, Wo = R.out_hw(H, W)
    g = torch.randn((B, Cout, Ho, Wo), dtype=torch.float64, generator=gen)
    y = F.conv2d(x, w, None, 2, 3)
    assert tuple(y.shape) == (B, Cout, Ho, Wo)
    dw = torch.ops.aten.convolution_backward(g, x, w, None, [2, 2], [3, 3], [1, 1], False, [0, 0], 1, [False, True, False])[1]
    xl, gl, wl = (t.permute(0, 2, 3, 1).contiguous().numpy() for t in (x, g, w))
    tol = lambda t: 1e-12 * max(float(t.abs().max()), 1e-300)
    got = torch.from_numpy(R.conv_ref(xl, wl)).permute(0, 3, 1, 2)
    assert float((got - y).abs().max()) <= tol(y)
    got = torch.from_numpy(R.wgrad_ref(gl, xl)).permute(0, 3, 1, 2)
    assert float((got - dw).abs().max()) <= tol(dw)
    # the sums of magnitudes the rounding bounds are built from: the same contractions of |.|
    ya = F.conv2d(x.abs(), w.abs(), None, 2, 3)
    assert float((torch.from_numpy(R.abs_conv_ref(xl, wl)).permute(0, 3, 1, 2) - ya).abs().max()) <= tol(ya)
    wa = torch.ops.aten.convolution_backward(g.abs(), x.abs(), w, None, [2, 2], [3, 3], [1, 1], False, [0, 0], 1, [False, True, False])[1]
    assert float((torch.from_numpy(R.abs_wgrad_ref(gl, xl)).permute(0, 3, 1, 2) - wa).abs().max()) <= tol(wa)
    # a cut into ranges of tiles: each range is its slice of the whole; a cut into ranges of stages adds up to the whole
    s = R.fwd_schedule(B, H, W, 256)
    T = s.total_tiles
    cuts = sorted({0, T // 3, (2 * T) // 3, T - 1, T})
    flat = R.conv_ref(xl, wl).reshape(-1, Cout)
    at = 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        part = R.conv_ref(xl, wl, tiles=(a, b))
        assert R.tile_pixel_start(a, B, H, W) == at and part.shape == flat[at:at + len(part)].shape
        assert np.allclose(part, flat[at:at + len(part)], rtol=0, atol=tol(y))       # (another blocking of the same matmul: equal to rounding)
        at += len(part)
    assert at == B * Ho * Wo == R.tile_pixel_start(T, B, H, W)
    q = R.wgrad_schedule(B, H, W, 256)
    S = q.total_stages
    cuts = sorted({0, S // 3, (2 * S) // 3, S - 1, S})
    parts = R.wgrad_ref_ranges(gl, xl, list(zip(cuts[:-1], cuts[1:])))
    assert np.allclose(parts.sum(0), R.wgrad_ref(gl, xl), rtol=0, atol=1e-11 * float(wa.max()))
    # the last stage by hand: the pixels from its first one to the end of the last row
    x0 = (q.tiles_x - 1) * R.WG_STAGE
    want = np.zeros((Cout, 7, 7, 3))
    for xo in range(x0, Wo):
        for r in range(7):
            for px in range(7):
                yy, xx = 2 * (Ho - 1) + r - 3, 2 * xo + px - 3
                if 0 <= yy < H and 0 <= xx < W:
                    want[:, r, px, :] += np.outer(gl[B - 1, Ho - 1, xo], xl[B - 1, yy, xx])
    assert np.allclose(R.wgrad_ref(gl, xl, (S - 1, S)), want, rtol=0, atol=1e-12 * max(float(np.abs(want).max()), 1e-300))


def test_schedules_by_hand_for_256_and_304_cus():
    # the bench shape [8, 3, 800, 1344]: 400 x 672 outputs, 42 tiles and 10.5 stages per row
    assert R.fwd_schedule(8, 800, 1344, 256) == (400, 672, 42, 134400, 510, 264)        # 134400 / 512 = 262.5 -> 263 -> 264
    assert R.fwd_schedule(8, 800, 1344, 304) == (400, 672, 42, 134400, 600, 224)        # 134400 / 608 = 221.05 -> 222 -> 224
    assert R.wgrad_schedule(8, 800, 1344, 256) == (11, 35200, 511, 69)                  # 35200 / 512 = 68.75
    assert R.wgrad_schedule(8, 800, 1344, 304) == (11, 35200, 607, 58)                  # 35200 / 608 = 57.9
    # the widest of the older direct tests: one tile per wave
    assert R.fwd_schedule(3, 32, 1000, 256) == (16, 500, 32, 1536, 384, 4)
    assert R.wgrad_schedule(2, 30, 600, 256) == (5, 150, 150, 1)
    assert R.fwd_schedule(1, 7, 7, 256) == (4, 4, 1, 4, 1, 4) and R.wgrad_schedule(1, 7, 7, 304) == (1, 4, 4, 1)
    # a wave owns more than one tile from 2 CUs x 4 + 1 tiles on
    for cus in (256, 304):
        H = 2 * (8 * cus) - 1
        assert R.fwd_schedule(1, H, 30, cus)[3:] == (8 * cus, 2 * cus, 4) and R.fwd_schedule(1, H + 2, 30, cus)[3:] == (8 * cus + 1, cus + 1, 8)
        assert R.wgrad_schedule(1, 4 * cus - 1, 66, cus) == (1, 2 * cus, 2 * cus, 1) and R.wgrad_schedule(1, 4 * cus + 1, 66, cus) == (1, 2 * cus + 1, cus + 1, 2)
    # tiles of a wave, coordinates, ring steps
    s = R.fwd_schedule(2, 2049, 30, 256)                                                 # Ho 1025, one tile per row: 2050 tiles, 8 per workgroup
    assert s == (1025, 15, 1, 2050, 257, 8) and R.fwd_ring_steps(s) == 2
    assert R.fwd_tiles_of(128, 0, s) == [1024, 1028] and R.fwd_tiles_of(128, 3, s) == [1027, 1031] and R.fwd_tiles_of(256, 1, s) == [2049]
    assert R.fwd_tiles_of(256, 2, s) == [] and R.fwd_last_wg_tiles(s) == 2
    assert R.tile_coords(1024, s) == (0, 1024, 0) and R.tile_coords(1028, s) == (1, 3, 0)      # one advance: four rows and the image boundary
    assert R.fwd_boundary_inside_a_walk(2, s)
    s = R.fwd_schedule(1, 3, 131, 256)
    assert s[:4] == (2, 66, 5, 10) and R.tile_coords(7, s) == (0, 1, 2)
    assert R.tile_pixel_start(7, 1, 3, 131) == 66 + 32 and R.tile_pixel_start(4, 1, 3, 131) == 64 and R.tile_pixel_start(10, 1, 3, 131) == 132
    assert [R.fwd_ring_steps(R.FwdSchedule(1, 1, 1, 1, 1, t)) for t in (4, 8, 12, 20)] == [2, 2, 4, 6]
    q = R.wgrad_schedule(2, 513, 130, 256)                                               # Ho 257, 65 = 64 + 1 outputs per row
    assert q == (2, 1028, 343, 3) and R.wgrad_stages_of(171, q) == (513, 516) and R.wgrad_stages_of(342, q) == (1026, 1028)
    assert R.wgrad_boundary_inside_a_range(2, 257, q) and R.wgrad_ranges_straddle_rows(q) and R.workspace_bytes(q) == 343 * 64 * 7 * 32 * 4
    assert R.tile_pixel_start(513, 2, 513, 130, R.WG_STAGE) == 256 * 65 + 64
    assert R.padded_width(33) == 40 and R.padded_width(30) == 36 and R.padded_bytes(1, 7, 7) == ((13 + 2) * 14 + 160) * 8


@pytest.mark.parametrize("cus", [256, 304, 64])
@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (1, 7, 7), (3, 32, 1000), (2, 2049, 30), (1, 2053, 33), (1, 600, 131), (2, 513, 130), (1, 341, 258), (8, 800, 1344)])
def test_every_tile_and_every_stage_is_owned_exactly_once(B, H, W, cus):
    s = R.fwd_schedule(B, H, W, cus)
    assert s.tiles_per_wg % 4 == 0 and s.wgs <= 2 * cus and (s.wgs - 1) * s.tiles_per_wg < s.total_tiles <= s.wgs * s.tiles_per_wg
    owned = [t for wg in range(s.wgs) for v in range(4) for t in R.fwd_tiles_of(wg, v, s)]
    assert sorted(owned) == list(range(s.total_tiles))
    assert all(len(R.fwd_tiles_of(wg, v, s)) <= R.fwd_ring_steps(s) for wg in (0, s.wgs - 1) for v in range(4))
    coords = [R.tile_coords(t, s) for t in (0, s.total_tiles - 1)]
    assert coords == [(0, 0, 0), (B - 1, s.Ho - 1, s.tiles_x - 1)]
    q = R.wgrad_schedule(B, H, W, cus)
    assert q.wgs <= 2 * cus
    ranges = [R.wgrad_stages_of(wg, q) for wg in range(q.wgs)]
    assert ranges[0][0] == 0 and ranges[-1][1] == q.total_stages and all(a[1] == b[0] for a, b in zip(ranges[:-1], ranges[1:]))
    assert all(0 < b - a <= q.stages_per_wg for a, b in ranges)


@pytest.mark.parametrize("cus", [256, 304])
def test_every_case_reaches_its_depth_and_the_file_reaches_every_path(cus):
    names = [c.name for c in R.FCASES + R.WCASES]
    assert len(set(names)) == len(names)
    seen = set()
    for c in R.FCASES + [R.REAL_FWD]:
        B, H, W = R.forward_shape(c, cus)
        s = R.fwd_schedule(B, H, W, cus)
        assert s.tiles_per_wg == c.target and s.tiles_x == c.W and B == c.B and s.Wo % 16 != 0
        assert R.forward_shape(c, cus) == R.forward_case(c.target, c.W, c.B, cus, c.want)
        if H > 1:                                                       # the smallest: one row less misses the depth or a property
            p = R.fwd_schedule(B, H - 1, W, cus)
            assert p.tiles_per_wg != c.target or not all(R._fwd_has(w, B, p) for w in c.want)
        last = [len(R.fwd_tiles_of(s.wgs - 1, v, s)) for v in range(4)]
        if "short_tail" in c.want:
            assert 0 in last and R.fwd_last_wg_tiles(s) < 4
        if "uneven_tail" in c.want:
            assert len(set(last)) == 2 and min(last) >= 1
        if "image_boundary" in c.want:
            assert B == 2 and R.fwd_boundary_inside_a_walk(B, s)
        assert B * s.Ho * s.Wo <= 170000 and s.total_tiles <= 12500    # the CPU reference stays small
        seen |= {("depth", c.target), ("tiles_x", s.tiles_x)} | {("want", w) for w in c.want}
    assert seen >= {("depth", 8), ("depth", 12), ("depth", 20)} | {("tiles_x", k) for k in (1, 2, 3, 5)} | {("want", w) for w in ("short_tail", "uneven_tail", "image_boundary")}
    assert R.REAL_FWD.target >= 12
    seen = set()
    for c in R.WCASES + [R.REAL_WGRAD]:
        B, H, W = R.wgrad_shape(c, cus)
        q = R.wgrad_schedule(B, H, W, cus)
        Ho, Wo = R.out_hw(H, W)
        assert q.stages_per_wg == c.target and W == c.W and B == c.B and Wo % 64 != 0
        if "last_one" in c.want:
            a, b = R.wgrad_stages_of(q.wgs - 1, q)
            assert b - a == 1
        if "image_boundary" in c.want:
            assert B == 2 and any(a < Ho * q.tiles_x < b for a, b in (R.wgrad_stages_of(wg, q) for wg in range(q.wgs)))
        if "rows" in c.want:
            assert R.wgrad_ranges_straddle_rows(q)
        assert B * Ho * Wo <= 85000 and q.total_stages <= 3200
        seen |= {("depth", c.target)} | {("want", w) for w in c.want}
    assert seen >= {("depth", 2), ("depth", 3), ("depth", 5)} | {("want", w) for w in ("last_one", "image_boundary", "rows")}
    assert R.REAL_WGRAD.target >= 3
    with pytest.raises(AssertionError):
        R.forward_case(20, 1, 1, 100000)                                # out of reach below the height limit: an error, never a skip
    with pytest.raises(AssertionError):
        R.wgrad_case(5, 66, 1, 100000)


def test_integer_forward_operands_stay_within_their_caps():
    w = R.stem_weights()
    nz = w != 0
    assert int(nz.reshape(64, -1).sum(1).max()) == 49 and bool((nz.reshape(64, 7, 21).sum(2) == 7).all())
    assert int(nz.reshape(64, 147).sum(0).min()) >= 21 and bool(nz.reshape(64, 49, 3).any(1).all())     # every channel reads all three colours
    for c in R.FCASES:
        B, H, W = R.forward_shape(c, 256)
        if B * H * W > 70000:
            H = 257                                                     # (the generator does not depend on the height: a shorter image of the same width)
        x, w = R.forward_operands(B, H, W)
        R.assert_forward_exact(x, w, c.target)
        assert set(np.unique(x)) == {-2, -1, 0, 1, 2}
        y = R.conv_ref(x, w)
        assert float(np.abs(y).max()) <= R.Y_CAP and R.exact_in_16_bits(y) and float(np.abs(y).max()) >= 16
        s = R.fwd_schedule(B, H, W, 256)
        flat = y.reshape(-1, 64)
        for wg in (0, s.wgs - 1):
            a, b = (R.tile_pixel_start(t, B, H, W) for t in R.fwd_wg_tiles(wg, s))
            assert float((flat[a:b] ** 2).sum(0).max()) < 2 ** 24
        for dt in (torch.bfloat16, torch.float16):                      # the same numbers in both element types
            for t in (x, w, y):
                assert np.array_equal(R.round_to(t, dt).astype(np.float64), np.asarray(t, np.float64))
    x, w = R.forward_operands(1, 9, 9)
    with pytest.raises(AssertionError):
        R.assert_forward_exact(x * 2, w, 8)
    with pytest.raises(AssertionError):
        R.assert_forward_exact(x, np.abs(w) + 1, 8)
    with pytest.raises(AssertionError):
        R.assert_forward_exact(x, w, 64)
    w0 = w.copy()
    w0[3, 2] = 0
    with pytest.raises(AssertionError):
        R.assert_forward_exact(x, w0, 8)                                # a channel without a weight in kernel row 2
    w0 = np.zeros_like(w)
    w0[:3] = w[:3]
    with pytest.raises(AssertionError):
        R.assert_forward_exact(x, w0, 8)                                # taps that fewer than four channels see


@pytest.mark.parametrize("case", R.WCASES, ids=lambda c: c.name)
def test_integer_weight_gradient_operands_stay_within_their_caps(case):
    B, H, W = R.wgrad_shape(case, 256)
    g, x = R.wgrad_operands(B, H, W)
    total = R.wgrad_ref(g, x)
    R.assert_wgrad_exact(g, x, total)
    assert float(np.abs(total).max()) >= 64
    z, coef3, fwd = R.bn_operands(B, H, W)
    for dt in (torch.bfloat16, torch.float16):
        dz = R.bn_grad_ref(g, z, coef3, fwd, dt)
        R.assert_bn_exact(z, coef3, fwd, dz)
        # the rule by hand: alive where z > 0
        ba, bk0, bk1 = coef3
        assert np.array_equal(dz, ba * np.where(z > 0, g, 0) + bk1 * z + bk0) and float(np.abs(dz).max()) == R.DZ_CAP
        R.assert_wgrad_exact(dz, x, R.wgrad_ref(dz, x), R.DZ_CAP)
    with pytest.raises(AssertionError):
        R.assert_wgrad_exact(g * 0.5, x, total)
    with pytest.raises(AssertionError):
        R.assert_wgrad_exact(g, x, total + 70000)
    with pytest.raises(AssertionError):
        R.assert_bn_exact(z, coef3 * np.array([[1], [0], [1]], np.float32), fwd, dz)
    with pytest.raises(AssertionError):
        R.assert_bn_exact(np.abs(z), coef3, fwd, dz)


def test_bn_gradient_rule_on_real_values():
    "bn_grad_ref on fractional operands: the threshold is strict and type-dependent, the result is rounded to the element type once."
    g = np.array([1.5, 1.5, 1.5, -0.75], np.float32).reshape(1, 1, 1, 4)
    z = np.array([2.0 ** -25, 2.0 ** -24, -1.0, 0.5], np.float32).reshape(1, 1, 1, 4)
    coef3 = np.array([[2, 2, 2, 3], [0.25, 0.25, 0.25, 1.0 / 3], [0, 0, 1, 1]], np.float32)
    fwd = np.array([[1, 1, 1, 1], [0, 0, 0, 0]], np.float32)
    f16 = R.bn_grad_ref(g, z, coef3, fwd, torch.float16).reshape(-1)
    b16 = R.bn_grad_ref(g, z, coef3, fwd, torch.bfloat16).reshape(-1)
    assert f16[0] == 0.25 and b16[0] == 3.25                            # 2^-25 is not above fp16's threshold, and above bf16's
    assert f16[1] == 3.25 and b16[1] == 3.25 and f16[2] == -0.75 and b16[2] == -0.75
    want = np.float32(3) * np.float32(-0.75) + (np.float32(0.5) + np.float32(1.0 / 3))
    assert f16[3] == R.round_to(np.array([want]), torch.float16)[0] and b16[3] == R.round_to(np.array([want]), torch.bfloat16)[0] and f16[3] != b16[3]
    assert R.relu_alive(torch.float16) == 2.0 ** -25 and 0 < R.relu_alive(torch.bfloat16) < 1e-40
    assert R.half_ulp(np.array([1.0, 3.0, 0.0]), True).tolist() == [2.0 ** -8, 2.0 ** -7, 2.0 ** -134] and R.half_ulp(np.array([1.0]), False)[0] == 2.0 ** -11
