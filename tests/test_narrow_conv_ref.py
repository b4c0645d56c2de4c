"""CPU: ``narrow_conv_ref.py`` on its own -- the two float64 references against torch's float64 convolution and its autograd, the
restated schedules of ``wgrad3x3_kernel`` and ``conv3x3_narrow64_kernel`` (every tile / row walked exactly once), the case tables
worked through for 256 CUs, and the operand generators' promises that let ``test_narrow_conv_gpu.py`` ask the kernels for equality."""
import pytest
import torch
import torch.nn.functional as F

import narrow_conv_ref as R

DTYPES = [torch.bfloat16, torch.float16]


@pytest.mark.parametrize("N,H,W,Cout,Cin", [(1, 1, 1, 3, 2), (2, 3, 5, 4, 6), (3, 4, 2, 5, 3)])
def test_references_equal_the_float64_convolution_and_its_autograd(N, H, W, Cout, Cin):
    gen = torch.Generator().manual_seed(7 * N + H)
    x = torch.randn((N, Cin, H, W), dtype=torch.float64, generator=gen, requires_grad=True)
    w = torch.randn((Cout, Cin, 3, 3), dtype=torch.float64, generator=gen, requires_grad=True)
    g = torch.randn((N, Cout, H, W), dtype=torch.float64, generator=gen)
    bias = torch.randn(Cout, dtype=torch.float64, generator=gen)
    y = F.conv2d(x, w, None, 1, 1)
    y.backward(g)
    xl, gl, wl = x.detach().permute(0, 2, 3, 1), g.permute(0, 2, 3, 1), w.detach().permute(0, 2, 3, 1)
    got = R.forward_ref(xl, wl).permute(0, 3, 1, 2)
    assert float((got - y.detach()).abs().max()) <= 1e-12 * float(y.detach().abs().max())
    for relu in (False, True):
        want = y.detach() + bias[None, :, None, None]
        want = F.relu(want) if relu else want
        assert float((R.forward_ref(xl, wl, bias, relu).permute(0, 3, 1, 2) - want).abs().max()) <= 1e-12 * float(want.abs().max())
    dw = R.wgrad_ref(gl, xl).view(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
    assert float((dw - w.grad).abs().max()) <= 1e-12 * float(w.grad.abs().max())
    # the sum of magnitudes the rounding bound is built from: the same gather on |g|, |x|
    xa = x.detach().abs().requires_grad_(False)
    wa = torch.zeros_like(w, requires_grad=True)
    F.conv2d(xa, wa, None, 1, 1).backward(g.abs())
    got_abs = R.abs_terms_sum(gl, xl).view(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
    assert float((got_abs - wa.grad).abs().max()) <= 1e-12 * float(wa.grad.abs().max())


SCHEDULE_SHAPES = [
    # N, H, W, Cout, Cin, wgs_per_sub
    (1, 3, 1, 64, 64, 4), (2, 5, 32, 64, 64, 4), (1, 7, 33, 64, 64, 2), (3, 3, 64, 64, 64, 4), (2, 3, 65, 64, 64, 3),
    (1, 5, 96, 64, 64, 4), (2, 5, 97, 64, 64, 1), (1, 4, 128, 128, 64, 2), (2, 3, 129, 64, 128, 2), (1, 9, 130, 128, 128, 4),
    (1, 1, 1, 64, 64, 256),            # one tile, 511 teams without one
    (1, 3, 30, 64, 64, 256),           # the smallest existing case: three tiles on 512 teams
    (1, 19, 1, 512, 512, 4),           # ragged: seven working teams, the last holds one tile
    (1, 17, 33, 512, 512, 4),          # six working teams, a whole workgroup idle
    (2, 5, 70, 512, 512, 4), (9, 3, 64, 512, 512, 4), (11, 3, 97, 512, 512, 4),
    (1, 1027, 33, 64, 64, 256), (103, 5, 96, 64, 64, 256), (257, 7, 33, 64, 128, 128),
    (2, 3, 200, 64, 64, 5),            # four tiles per row, a workgroup count that divides nothing
]


@pytest.mark.parametrize("N,H,W,Cout,Cin,wps", SCHEDULE_SHAPES)
def test_wgrad_schedule_walks_every_tile_once_and_every_pixel_once(N, H, W, Cout, Cin, wps):
    s = R.wgrad_schedule(N, H, W, Cout, Cin, wps)
    assert s.tiles_x == -(-W // 64) and s.tiles == N * H * s.tiles_x == len(s.tile_map)
    assert s.subs == (Cout // 64) * (Cin // 64) and len(s.ranges) == s.subs * wps
    assert (s.tiles_per_team - 1) * 2 * wps < s.tiles <= s.tiles_per_team * 2 * wps
    seen_px = torch.zeros((N, H, W), dtype=torch.int32)
    for wg in range(wps):                                   # the first sub-problem; the others repeat it
        for b, e in s.ranges[wg]:
            assert 0 <= b <= e <= s.tiles and e - b <= s.tiles_per_team
            for t in range(b, e):
                img, y, x0, ks = s.tile_map[t]
                assert x0 % 64 == 0 and x0 < W and ks == (2 if W - x0 > 32 else 1)
                seen_px[img, y, x0:min(x0 + 64, W)] += 1
        (b0, e0), (b1, e1) = s.ranges[wg]
        assert s.pixel_start(b0) <= s.pixel_start(max(e0, e1)) <= N * H * W
    assert bool((seen_px == 1).all())
    for wg in range(len(s.ranges)):
        assert s.ranges[wg] == s.ranges[wg % wps]
        assert s.block(wg) == ((wg // wps) // (Cin // 64) * 64, (wg // wps) % (Cin // 64) * 64)
    assert sorted({s.block(wg) for wg in range(len(s.ranges))}) == [(n, c) for n in range(0, Cout, 64) for c in range(0, Cin, 64)]
    sizes = s.team_sizes()
    assert len(sizes) == 2 * wps and sum(sizes) == s.tiles


def test_wgrad_schedule_shapes_include_idle_teams_and_every_row_length():
    ws = {sh[2] for sh in SCHEDULE_SHAPES}
    assert {1, 32, 33, 64, 65, 96, 97, 128, 129, 130} <= ws
    idle = [R.wgrad_schedule(*sh).team_sizes().count(0) for sh in SCHEDULE_SHAPES]
    assert sum(1 for v in idle if v) >= 5 and 511 in idle
    s = R.wgrad_schedule(1, 19, 1, 512, 512, 4)
    assert s.team_sizes() == [3, 3, 3, 3, 3, 3, 1, 0] and s.ranges[3] == ((18, 19), (19, 19)) and s.ranges[255] == s.ranges[3]


@pytest.mark.parametrize("N,H,W,Cout,Cin,wps", [(2, 3, 70, 64, 64, 2), (1, 7, 33, 128, 64, 3), (3, 3, 5, 64, 128, 4), (1, 2, 1, 64, 64, 4)])
def test_partials_of_the_schedule_sum_to_the_reference(N, H, W, Cout, Cin, wps):
    g, x = R.wgrad_operands(N, H, W, Cout, Cin, torch.bfloat16, integer=True)
    s = R.wgrad_schedule(N, H, W, Cout, Cin, wps)
    part = R.wgrad_partials_ref(g, x, s)
    assert part.shape == (s.subs * wps, 64, 9, 64)
    ref = R.wgrad_ref(g, x)
    assert torch.equal(R.total_from_partials(part, s, Cout, Cin), ref)
    assert torch.equal(R.reduce_ref(part.float(), s, Cout, Cin, torch.float32).double(), ref)
    # one workgroup by hand: its teams' tiles, pixel by pixel
    wg = len(s.ranges) - 1
    n0, c0 = s.block(wg)
    want = torch.zeros((64, 9, 64), dtype=torch.float64)
    for b, e in s.ranges[wg]:
        for t in range(b, e):
            img, y, x0, _ = s.tile_map[t]
            for px in range(x0, min(x0 + 64, W)):
                for tap in range(9):
                    yy, xx = y + tap // 3 - 1, px + tap % 3 - 1
                    if 0 <= yy < H and 0 <= xx < W:
                        want[:, tap, :] += torch.outer(g[img, y, px, n0:n0 + 64].double(), x[img, yy, xx, c0:c0 + 64].double())
    assert torch.equal(part[wg], want)


@pytest.mark.parametrize("N,H,W,rows", [(1, 1, 1, 1), (2, 7, 129, 3), (1, 11, 130, 4), (3, 19, 145, 10), (1, 12, 33, 12), (2, 13, 257, 4),
                                        (1, 300, 128, 7), (1, 5, 384, 5)])
def test_band_schedule_walks_every_row_once(N, H, W, rows):
    s = R.band_schedule(N, H, W, rows)
    assert s.strips == -(-W // 128) and s.bands == -(-H // rows) == len(s.band_rows)
    assert [y for y0, y1 in s.band_rows for y in range(y0, y1)] == list(range(H))
    assert all(0 < y1 - y0 <= rows for y0, y1 in s.band_rows) and all(y1 - y0 == rows for y0, y1 in s.band_rows[:-1])
    assert 1 <= s.last_strip_pixels <= 128 and (s.strips - 1) * 128 + s.last_strip_pixels == W
    sc = R.store_counts(W)
    assert len(sc) == 2 * s.strips and sum(sc) == -(-W // 16) and all(0 <= v <= 4 for v in sc)


def _rows_256(N, H, W):
    "rn_conv3x3_narrow_rows_per_band worked through for 256 CUs."
    bands = max(1, min(H, 512 // (N * -(-W // 128))))
    return -(-H // bands)


def test_case_tables_cover_what_the_kernels_can_get_wrong_on_256_cus():
    assert len({c.name for c in R.WCASES}) == len(R.WCASES) and len({c.name for c in R.FCASES}) == len(R.FCASES)
    reached = {}
    for c in R.WCASES:
        subs = (c.Cout // 64) * (c.Cin // 64)
        wps = 256 // subs
        N, H, W = R.wgrad_shape(c, wps)
        s = R.wgrad_schedule(N, H, W, c.Cout, c.Cin, wps)
        R.check_wgrad_case(c, s)
        assert N * H * W * max(c.Cout, c.Cin) * 2 < 30 << 20 and 9 * N * H * W < 2 ** 24, c.name
        reached.setdefault((c.Cout, c.Cin) if c.Cout == c.Cin else "rect", []).append((c, s))
    assert set(reached) == {(64, 64), "rect", (512, 512)}
    kinds = lambda pred: {k for k, v in reached.items() if any(pred(c, s) for c, s in v)}
    for what, pred in (("full at 2", lambda c, s: c.full and s.tiles_per_team == 2), ("3", lambda c, s: s.tiles_per_team == 3 and c.last is None),
                       ("4", lambda c, s: s.tiles_per_team == 4), ("5", lambda c, s: s.tiles_per_team == 5), (">= 8", lambda c, s: s.tiles_per_team >= 8),
                       ("tail of 1", lambda c, s: c.last == 1 and c.odd_working), ("tail of 2", lambda c, s: c.last == 2),
                       ("mixed k-steps at depth >= 3", lambda c, s: c.mixed and s.tiles_per_team >= 3),
                       ("two images in one walk", lambda c, s: c.straddle), ("real operands", lambda c, s: c.real and s.tiles_per_team >= 3)):
        assert len(kinds(pred)) >= 2, what
    assert {70, 96, 97, 33, 64, 1} <= {c.W for c in R.WCASES if c.depth >= 3}
    assert any(s.team_sizes()[-2:] == [0, 0] for v in reached.values() for c, s in v if c.last is not None)       # a whole workgroup idle
    assert sum(1 for c in R.WCASES if c.wrapper) >= 1

    seen = []
    for c in R.FCASES:
        N = R.forward_images(c, _rows_256)
        s = R.check_forward_case(c, N, _rows_256(N, c.H, c.W))
        assert N * c.H * c.W * 128 < 31 << 20, c.name
        seen.append((c, s))
    assert {3, 4, 5, 6} <= {s.rows_per_band for _, s in seen} and any(s.rows_per_band >= 9 and s.bands > 1 for _, s in seen)
    assert any(s.last_band_rows == 1 and s.rows_per_band > 2 for _, s in seen)
    assert any(s.last_band_rows == s.rows_per_band - 1 and s.rows_per_band > 2 for _, s in seen)
    assert any(s.bands == 1 and s.rows_per_band == c.H > 4 for c, s in seen)
    assert {1, 2, 9, 16, 17, 48} <= {s.last_strip_pixels for _, s in seen if s.strips >= 2}
    assert {1, 2, 3, 4} <= {v for c, _ in seen for v in R.store_counts(c.W)}
    assert max(R.FCASES, key=lambda c: c.rows).probe and max((c for c in R.FCASES if c.bands > 1), key=lambda c: c.rows).probe


def test_tail_search():
    assert R.tiles_for_tail(8, 3, 1, True) == 19 and R.tiles_for_tail(8, 3, 2, False) == 17
    assert R.tiles_for_tail(512, 3, 1, True) == 1027 and R.tiles_for_tail(512, 3, 2, False) == 1025
    assert R.tiles_for_tail(2, 3, 1, True) is None            # two teams: a third tile per team needs both of them working


@pytest.mark.parametrize("shape", [(2, 9, 33, 64, 64), (1, 40, 70, 128, 64), (3, 5, 1, 64, 128)])
def test_integer_weight_gradient_operands_keep_their_promises(shape):
    ops = {dt: R.wgrad_operands(*shape, dt, integer=True) for dt in DTYPES}
    for a, b in zip(ops[torch.bfloat16], ops[torch.float16]):
        assert torch.equal(a.double(), b.double())                 # the same numbers in both types
    g, x = ops[torch.bfloat16]
    assert g.shape == shape[:3] + (shape[3],) and x.shape == shape[:3] + (shape[4],)
    assert 0.5 < float((g == 0).float().mean()) < 0.8 and float(g.abs().max()) == 3
    R.assert_wgrad_exactness(g, x, R.wgrad_ref(g, x), R.abs_terms_sum(g, x))
    # ... and the assertions do fire: a fraction, a value past 3, a sum past 2^24, a gradient past the fp16 range
    ref, abs_sum = R.wgrad_ref(g, x), R.abs_terms_sum(g, x)
    for bad in (lambda: R.assert_wgrad_exactness(g * 0.5, x, ref, abs_sum), lambda: R.assert_wgrad_exactness(g * 2, x, ref, abs_sum),
                lambda: R.assert_wgrad_exactness(g, x, ref, abs_sum + 2.0 ** 24), lambda: R.assert_wgrad_exactness(g, x, ref + 65536, abs_sum)):
        with pytest.raises(AssertionError):
            bad()
    gr, xr = R.wgrad_operands(*shape, torch.float16, integer=False)
    assert not torch.equal(gr.double(), gr.double().round()) and abs(float(gr.float().std()) - 1) < 0.1


@pytest.mark.parametrize("shape", [(2, 5, 33), (1, 3, 130)])
def test_integer_forward_operands_keep_their_promises(shape):
    ops = {dt: R.forward_operands(*shape, dt) for dt in DTYPES}
    for a, b in zip(ops[torch.bfloat16], ops[torch.float16]):
        assert torch.equal(a.double(), b.double())
    x, w, bias = ops[torch.bfloat16]
    assert x.shape == shape + (64,) and w.shape == (64, 3, 3, 64) and bias.shape == (64,) and bias.dtype == torch.float32
    y, yb = R.forward_ref(x, w), R.forward_ref(x, w, bias)
    R.assert_forward_exactness(x, w, bias, y, yb)
    assert float(y.abs().max()) > 16 and bool((yb < 0).any()) and bool((yb > 0).any())      # the ReLU has something to do
    assert torch.equal(y.permute(0, 3, 1, 2), F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), None, 1, 1))
    for bad in (lambda: R.assert_forward_exactness(x * 2, w, bias, y, yb), lambda: R.assert_forward_exactness(x, w * 2, bias, y, yb),
                lambda: R.assert_forward_exactness(x, w, bias + 0.5, y, yb), lambda: R.assert_forward_exactness(x, w, bias, y + 200, yb),
                lambda: R.assert_forward_exactness(x, w, bias, y, yb + 0.5)):
        with pytest.raises(AssertionError):
            bad()


def test_rows_per_band_export_refuses_what_the_entry_point_refuses():
    "Host logic only (no GPU call is needed for the refusals): 0 for shapes rn_conv3x3_narrow_forward returns an error for."
    from pytorch_retinanet_amd._lib import lib
    assert lib.rn_conv3x3_narrow_rows_per_band(0, 5, 5) == 0 and lib.rn_conv3x3_narrow_rows_per_band(1, 0, 5) == 0
    assert lib.rn_conv3x3_narrow_rows_per_band(1, 5, -1) == 0 and lib.rn_conv3x3_narrow_rows_per_band(1 << 11, 1 << 10, 1 << 10) == 0
