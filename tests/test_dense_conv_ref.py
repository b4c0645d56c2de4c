"""CPU: ``dense_conv_ref.py`` on its own -- the float64 references against torch's float64 convolution and its autograd on every geometry
the GPU cases use, the restated schedules of the dense 3x3 family worked by hand for 256 and 304 CUs (every K-tile and every position
owned exactly once), and the operand generators' promises that let ``test_dense_conv_exact_gpu.py`` ask the kernels for equality."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dense_conv_ref as R


def _geometries():
    "Every (N, h, w) of the GPU cases (the run-time shapes at 256 CUs), and the degenerate ones by name."
    g = {(1, 1, 1), (1, 1, 7), (1, 7, 1), (1, 2, 2), (3, 2, 2)}
    for c in R.FCASES + R.DCASES + [R.REAL_DENSE, R.REAL_DGRAD]:
        g |= {(c.N, h, w) for h, w in c.hw}
    for c in R.BCASES + R.SCASES + [R.REAL_BAND, R.REAL_SPLITK]:
        g.add((c.N, c.H, c.W))
    for kind in WKINDS:
        N, hw = R.wgrad_case_shapes(kind, 256)
        g |= {(N, h, w) for h, w in hw}
    g |= {(R.REAL_WGRAD[0], h, w) for h, w in R.REAL_WGRAD[1]}
    g.add(R.splitk_shape(3, 256, 256))
    return sorted(g)


WKINDS = R.WKINDS


@pytest.mark.parametrize("N,H,W", _geometries())
def test_references_equal_the_float64_convolution_and_its_autograd(N, H, W):
    Cout, Cin = 5, 3
    gen = torch.Generator().manual_seed(7 * N + 3 * H + W)
    x = torch.randn((N, Cin, H, W), dtype=torch.float64, generator=gen, requires_grad=True)
    w = torch.randn((Cout, Cin, 3, 3), dtype=torch.float64, generator=gen, requires_grad=True)
    g = torch.randn((N, Cout, H, W), dtype=torch.float64, generator=gen)
    bias = torch.randn(Cout, dtype=torch.float64, generator=gen)
    y = F.conv2d(x, w, None, 1, 1)
    y.backward(g)
    xl, gl, wl = (t.detach().permute(0, 2, 3, 1).contiguous().numpy() for t in (x, g, w))
    tol = lambda t: 1e-12 * max(float(t.abs().max()), 1e-300)
    got = torch.from_numpy(R.conv_ref(xl, wl)).permute(0, 3, 1, 2)
    assert float((got - y.detach()).abs().max()) <= tol(y.detach())
    for relu in (False, True):
        want = y.detach() + bias[None, :, None, None]
        want = F.relu(want) if relu else want
        got = torch.from_numpy(R.conv_ref(xl, wl, bias.numpy(), relu)).permute(0, 3, 1, 2)
        assert float((got - want).abs().max()) <= tol(want)
    dw = torch.from_numpy(R.wgrad_ref(gl, xl)).permute(0, 3, 1, 2)
    assert float((dw - w.grad).abs().max()) <= tol(w.grad)
    # the input gradient is the same convolution of g with the flipped, transposed weights
    dx = torch.from_numpy(R.conv_ref(gl, R.dgrad_weights(wl))).permute(0, 3, 1, 2)
    assert float((dx - x.grad).abs().max()) <= tol(x.grad)
    # the sums of magnitudes the rounding bounds are built from: the same contractions of |.|
    assert np.allclose(R.abs_conv_ref(xl, wl), R.conv_ref(np.abs(xl), np.abs(wl)), rtol=0, atol=0)
    ya = F.conv2d(x.detach().abs(), w.detach().abs(), None, 1, 1)
    assert float((torch.from_numpy(R.abs_conv_ref(xl, wl)).permute(0, 3, 1, 2) - ya).abs().max()) <= tol(ya)
    wa = torch.zeros_like(w, requires_grad=True)
    F.conv2d(x.detach().abs(), wa, None, 1, 1).backward(g.abs())
    assert float((torch.from_numpy(R.abs_wgrad_ref(gl, xl)).permute(0, 3, 1, 2) - wa.grad).abs().max()) <= tol(wa.grad)
    # a range of positions: the ranges of any cut add up to the whole, and one range by hand
    M = N * H * W
    cuts = sorted({0, M // 3, (2 * M) // 3, M})
    parts = [R.wgrad_ref(gl, xl, (a, b)) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.allclose(sum(parts), R.wgrad_ref(gl, xl), rtol=0, atol=1e-12 * float(w.grad.abs().max()))
    m = M - 1
    n, h, w_ = m // (H * W), (m // W) % H, m % W
    want = np.zeros((Cout, 3, 3, Cin))
    for kh in range(3):
        for kw in range(3):
            hh, ww = h + kh - 1, w_ + kw - 1
            if 0 <= hh < H and 0 <= ww < W:
                want[:, kh, kw, :] = np.outer(gl[n, h, w_], xl[n, hh, ww])
    assert np.allclose(R.wgrad_ref(gl, xl, (m, M)), want, rtol=0, atol=1e-13 * max(float(np.abs(want).max()), 1e-300))


def test_k_ranges_of_the_reference_add_up_and_follow_the_walk():
    x, w, _ = R.forward_operands(2, 3, 5, 192, 256)
    full = R.conv_ref(x, w)
    for S in (2, 3):
        assert np.array_equal(sum(R.conv_ref(x, w, ktiles=r) for r in R.ksplit_ranges(192, S)), full)
    # K-tile kt = 9 * chunk + tap: tile 13 is chunk 1, tap 4 (the centre): y = x[.., 64:128] @ w[:, 1, 1, 64:128]^T
    want = x.reshape(-1, 192)[:, 64:128].astype(np.float64) @ w[:, 1, 1, 64:128].astype(np.float64).T
    assert np.array_equal(R.conv_ref(x, w, ktiles=(13, 14)).reshape(-1, 256), want)


def test_schedules_by_hand_for_256_and_304_cus():
    # MODE_DENSE grid
    g = R.dense_grid([1, 255, 256, 4], 64, 256)
    assert g.tile_beg == [0, 1, 2, 3, 4] and g.col_tiles == 1 and g.ktiles == 9
    g = R.dense_grid([257, 513, 4], 128, 512)
    assert g.tile_beg == [0, 2, 5, 6] and g.col_tiles == 2 and g.ktiles == 18
    assert R.row_tiles(1) == 1 and R.row_tiles(256) == 1 and R.row_tiles(257) == 2 and R.row_tiles(513) == 3
    assert R.straddling_tiles(3, 9, 30) == 2 and R.straddling_tiles(1, 19, 27) == 0 and R.straddling_tiles(3, 16, 16) == 0
    # band walk
    b = R.band_walk(1, 1, 1, 64, 128)
    assert (b.tiles, b.col_tiles, b.NB, b.last_rows) == (1, 1, 3, 1) and b.bands == [(0, 0, 0), (0, 1, 1), (0, 2, 0)]
    b = R.band_walk(3, 9, 30, 192, 384)
    assert (b.tiles, b.col_tiles, b.NB, b.last_rows) == (4, 3, 9, 42)
    assert b.bands[2:5] == [(0, 2, 0), (1, 0, 1), (1, 1, 0)]          # an odd band count per chunk: chunk 1 starts on the other buffer
    assert R.band_walk(1, 1, 515, 512, 128).NB == 24 and R.band_walk(1, 1, 515, 512, 128).last_rows == 3
    # split-K: S = cus / workgroups, 3 -> 2 -> 1
    for cus, last3, last2 in ((256, 85, 128), (304, 101, 152)):
        f = lambda wgs: R.dense_ksplit(wgs * 256, 256, cus)
        assert (f(1), f(last3), f(last3 + 1), f(last2), f(last2 + 1)) == (3, 3, 2, 2, 1)
        assert R.dense_ksplit(last3 * 256 + 1, 256, cus) == 2 and R.dense_ksplit((last3 // 2) * 256, 512, cus) == 3
    assert R.dense_ksplit(8 * 25 * 42, 512, 256) == 3 and R.dense_ksplit(8 * 50 * 84, 256, 256) == 1      # conv2 of layer4 / layer3 at 800 x 1333
    assert R.ksplit_ranges(64, 3) == [(0, 3), (3, 6), (6, 9)]         # one kernel row each
    assert R.ksplit_ranges(64, 2) == [(0, 4), (4, 9)]                 # inside kernel row 1
    assert R.ksplit_ranges(192, 3) == [(0, 9), (9, 18), (18, 27)]     # one chunk each
    assert R.ksplit_ranges(192, 2) == [(0, 13), (13, 27)]             # chunk 1, between taps 3 and 4
    assert R.ksplit_ranges(512, 3) == [(0, 24), (24, 48), (48, 72)]
    # weight gradient: FPN P3 / P4 / P5 of the 800 x 1333 bucket, 8 images: 525 + 132 + 35 K-tiles
    s = R.dense_splits([33600, 8400, 2184], 256)
    assert (s.budget, s.tps, s.beg) == (28, 27, [0, 20, 25, 27])      # 25 and 26 tiles per split would need 29 splits
    assert s.rows[19] == (0, 19 * 27 * 64, 33600) and s.tiles_of(19) == 12 and s.rows[26] == (2, 1728, 2184) and s.tiles_of(26) == 8
    s = R.dense_splits([33600, 8400, 2184], 304)
    assert (s.budget, s.tps, s.beg) == (33, 22, [0, 24, 30, 32])
    s = R.dense_splits([1], 256)
    assert (s.budget, s.tps, s.beg, s.rows) == (28, 1, [0, 1], [(0, 0, 1)])
    s = R.dense_splits([193, 383, 1], 256)
    assert s.tps == 1 and s.beg == [0, 4, 10, 11] and s.rows[3] == (0, 192, 193) and s.rows[9] == (1, 320, 383)
    assert R.dense_splits([1, 1, 1, 1], 27).budget == 4                # at least one split per problem


@pytest.mark.parametrize("cus", [256, 304, 64])
@pytest.mark.parametrize("Ms", [[1], [63], [64], [65], [127], [8400], [33600, 8400, 2184], [193, 383, 3650], [1, 63, 4000], [5, 5, 5, 5], [100000, 1]])
def test_split_tables_cover_every_k_tile_exactly_once(Ms, cus):
    s = R.dense_splits(Ms, cus)
    assert s.total == len(s.rows) <= s.budget and s.beg[0] == 0 and len(s.beg) == len(Ms) + 1
    for p, M in enumerate(Ms):
        mine = s.rows[s.beg[p]:s.beg[p + 1]]
        assert mine and all(q == p for q, _, _ in mine)
        assert mine[0][1] == 0 and mine[-1][2] == M and all(a[2] == b[1] for a, b in zip(mine[:-1], mine[1:]))
        assert all(m1 - m0 == s.tps * R.WG_POS for _, m0, m1 in mine[:-1]) and 0 < mine[-1][2] - mine[-1][1] <= s.tps * R.WG_POS
    assert sum(s.tiles_of(i) for i in range(s.total)) == sum(-(-M // R.WG_POS) for M in Ms)
    if s.tps > 1:                                                       # the smallest depth that fits the budget
        kt = [-(-M // R.WG_POS) for M in Ms]
        assert sum(-(-k // (s.tps - 1)) for k in kt) > s.budget
    for Cin in (64, 128, 192, 512):
        for S in (1, 2, 3):
            r = R.ksplit_ranges(Cin, S)
            assert r[0][0] == 0 and r[-1][1] == 9 * Cin // 64 and all(a[1] == b[0] and a[0] < a[1] for a, b in zip(r, r[1:] + [(r[-1][1], 0)]))


def test_gpu_case_tables_reach_what_they_are_for_on_256_and_304_cus():
    names = [c.name for c in R.FCASES + R.DCASES + R.BCASES + R.SCASES]
    assert len(set(names)) == len(names)
    # MODE_DENSE forward
    assert {len(c.hw) for c in R.FCASES} == {1, 2, 3, 4}
    assert {1, 255, 256, 257, 513} <= {M for c in R.FCASES for M in c.Ms}
    assert {(1, 1), (2, 2)} <= {hw for c in R.FCASES for hw in c.hw}
    assert any(h == 1 and w > 1 for c in R.FCASES for h, w in c.hw) and any(w == 1 and h > 1 for c in R.FCASES for h, w in c.hw)
    assert any(c.N == 3 and R.straddling_tiles(c.N, *c.hw[0]) > 0 for c in R.FCASES)
    assert {c.Cin for c in R.FCASES} == {64, 128, 512} and {c.Cout for c in R.FCASES} == {256, 512}
    assert all(c.Cin % 256 == 0 and c.Cout % 64 == 0 for c in R.DCASES)             # the launch's Cout is the convolution's Cin
    # band kernel
    assert {c.Cin for c in R.BCASES} == {64, 128, 192, 512} and {c.Cout for c in R.BCASES} == {128, 256, 384}
    assert {1, 255, 256, 257, 258, 259, 515} <= {c.M for c in R.BCASES}
    assert {1, 2, 3, 256, 257, 300} <= {c.W for c in R.BCASES} and {c.H for c in R.BCASES} >= {1, 2} and {c.N for c in R.BCASES} == {1, 3}
    assert any(c.W > R.BAND_POS and c.H > 1 for c in R.BCASES)
    assert {R.band_walk(c.N, c.H, c.W, c.Cin, c.Cout).NB for c in R.BCASES} == {3, 6, 9, 24}
    assert any(c.M % 256 and R.straddling_tiles(c.N, c.H, c.W) for c in R.SCASES) and any(c.Cout > 128 for c in R.SCASES)
    for cus in (256, 304):
        # split-K
        for Cin in (64, 192):
            N, H, W = R.splitk_shape(3, 512, cus)
            assert R.dense_ksplit(N * H * W, 512, cus) == 3 and R.row_tiles(N * H * W) == 3 and (N * H * W) % 256
            N, H, W = R.splitk_shape(2, 256, cus)
            assert R.dense_ksplit(N * H * W, 256, cus) == 2 and (N * H * W) % 256 and N * H * W * 256 * 2 * 4 < 64 << 20
        # weight gradient
        tps3 = []
        for kind in WKINDS:
            N, hw = R.wgrad_case_shapes(kind, cus)
            Ms = [N * h * w for h, w in hw]
            s = R.dense_splits(Ms, cus)
            assert s.tps == (3 if kind.startswith("p3") else 1) and max(Ms) < 6000, (kind, s.tps, Ms)
            if kind.startswith("p3"):
                tps3 += Ms[:2]
            if kind == "p3_tps3_tails":
                assert Ms[0] == 64 * s.tps + 1 and Ms[1] == 64 * 2 * s.tps - 1
                assert [s.tiles_of(i) for i in range(s.beg[0], s.beg[2])] == [3, 1, 3, 3] and s.rows[1] == (0, 192, 193) and s.rows[3] == (1, 192, 383)
        assert sorted(tps3) == [1, 63, 64, 65, 193, 383]
        N, hw = R.REAL_WGRAD
        assert R.dense_splits([N * h * w for h, w in hw], cus).total >= 3


@pytest.mark.parametrize("case", R.FCASES + R.DCASES, ids=lambda c: c.name)
def test_integer_forward_cases_stay_within_their_cap(case):
    dgrad = case in R.DCASES
    for p, (h, w) in enumerate(case.hw):
        if dgrad:                                                       # g [N][h][w][Cout] against the flipped weights [Cin][3][3][Cout]
            g, wt, wf = R.dgrad_operands(case.N, h, w, case.Cin, case.Cout, seed=p)
            assert wt.shape == (case.Cout, 3, 3, case.Cin) and wf.shape == (case.Cin, 3, 3, case.Cout)
            y = R.conv_ref(g, wf)
            R.assert_forward_exact(g, wf, None, y, None)
            assert float(np.abs(y).max()) <= 27 * case.Cout // 64
            continue
        x, wt, bias = R.forward_operands(case.N, h, w, case.Cin, case.Cout, seed=p)
        y, yb = R.conv_ref(x, wt), R.conv_ref(x, wt, bias)
        R.assert_forward_exact(x, wt, bias, y, yb)
        assert float(np.abs(y).max()) <= 27 * case.Cin // 64 and float(np.abs(bias).max()) == 40
        assert bool((yb < 0).any()) and bool((yb > 0).any())           # the ReLU has something to do ...
        if case.Cin == 64:                                              # ... and where |conv| <= 27 it empties the columns whose bias is below -27
            neg = bias < -27
            assert int(neg.sum()) >= 2 and not R.conv_ref(x, wt, bias, True)[..., neg].any() and R.conv_ref(x, wt, bias, True)[..., bias > 27].all()
        for dt in (torch.bfloat16, torch.float16):                      # the same numbers in both element types
            for t in (x, wt, y, yb):
                assert np.array_equal(torch.from_numpy(np.asarray(t, np.float32)).to(dt).double().numpy(), np.asarray(t, np.float64))


def test_forward_weights_touch_every_k_tile_and_every_channel_lane():
    w = R.forward_weights(256, 192)
    nz = w.reshape(256, 9, 3, 64) != 0
    assert bool((nz.sum(3) == 1).all())                                 # one per (output channel, tap, chunk)
    assert bool(nz.any(axis=0).all())                                   # over the output channels: every lane of every (tap, chunk)
    assert int(np.argmax(nz[3, 4, 2])) == (7 * 3 + 5 * 4 + 3 * 2) % 64
    wf = R.dgrad_weights(w)                                             # flipped: [Cin][3][3][Cout], still at most one per (row, tap, chunk of 64)
    assert wf.shape == (192, 3, 3, 256) and wf[5, 2, 0, 7] == w[7, 0, 2, 5]
    assert int((wf != 0).reshape(192, 9, 4, 64).sum(3).max()) == 1
    x = np.zeros((1, 1, 1, 192), np.float32)
    with pytest.raises(AssertionError):
        R.assert_forward_exact(x, w * 2, None, np.zeros(1), None)
    with pytest.raises(AssertionError):
        R.assert_forward_exact(x, w, None, np.full(1, 257.0), None)
    with pytest.raises(AssertionError):
        R.assert_forward_exact(x, w, None, np.full(1, 129.0), None, cap=R.STATS_CAP)
    with pytest.raises(AssertionError):
        R.assert_forward_exact(x + 0.5, w, None, np.zeros(1), None)


@pytest.mark.parametrize("case", R.BCASES + R.SCASES, ids=lambda c: c.name)
def test_integer_band_cases_stay_within_their_cap(case):
    x, w, _ = R.forward_operands(case.N, case.H, case.W, case.Cin, case.Cout)
    y = R.conv_ref(x, w)
    stats = case in R.SCASES
    R.assert_forward_exact(x, w, None, y, None, cap=R.STATS_CAP if stats else R.Y_CAP)
    if stats:                                                           # every tile's sums are exact in fp32
        for t in range(R.row_tiles(case.M)):
            rows = y.reshape(case.M, -1)[t * 256:(t + 1) * 256]
            assert float((rows ** 2).sum(0).max()) <= 2 ** 22 and float(np.abs(rows).sum(0).max()) < 2 ** 24


@pytest.mark.parametrize("kind,cus", [(k, 256) for k in WKINDS] + [(k, 304) for k in WKINDS if k.startswith("p3")])      # (only the P = 3 shapes follow the CU count)
def test_integer_weight_gradient_cases_stay_within_their_cap(kind, cus):
    N, hw = R.wgrad_case_shapes(kind, cus)
    for p, (h, w) in enumerate(hw):
        g, x = R.wgrad_operands(N, h, w, 256, 256, seed=p)
        ref = R.wgrad_ref(g, x)
        R.assert_wgrad_exact(g, x, ref, R.abs_wgrad_ref(g, x))
        assert float(np.abs(ref).max()) >= 1
    with pytest.raises(AssertionError):
        R.assert_wgrad_exact(g, x, ref + 300, R.abs_wgrad_ref(g, x))
    with pytest.raises(AssertionError):
        R.assert_wgrad_exact(g * 0.5, x, ref, R.abs_wgrad_ref(g, x))
