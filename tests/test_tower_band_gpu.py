"""GPU: the BAND walk of the head tile kernel (csrc/conv.hip, ``TOWER_BAND``) through the C ABI -- ``rn_conv3x3_canvas``,
``rn_conv3x3_canvas_batched_ex``, ``rn_conv3x3_canvas_dgrad_relu_batched`` and ``rn_conv3x3_canvas_sum2`` with Cout = 256 -- against
fp32 ``torch.nn.functional.conv2d`` (and its autograd input gradient) on the same 16-bit values.

Bar: the result is ONE 16-bit rounding of an f32-accumulated sum, the bar of ``tests/test_model_gpu.py`` /
``tests/test_dense_conv_gpu.py`` restated: bf16 (half an ulp = 2^-9 of the element) 2.5e-3 in L2 and 2^-8 of the tensor's largest
magnitude per element; fp16 has three more mantissa bits, so both figures divided by 8.

Shapes are the smallest at which a band can go wrong: a canvas 6 positions wide (the +-Wp kernel-row offsets are shorter than a band
and every band of the single ragged tile leaves the canvas), 259 positions (two tiles, the second nearly empty), exactly 512, and
sheets with seams (zero rows / columns of the keep mask inside a band, as between the levels of the packed canvas).

The shapes the walk does not take: Cout = 512 runs the tile walk and is checked here like the others.  Cout = 128 and Cin = 96 are
rejected by these entry points with RN_EUNSUPPORTED whatever the switch (include/retinanet_hip.h; ``tests/test_host_surface.py``
checks Cin = 96): they have no tile-walk fallback to return RN_OK from, and this file only checks that this did not change.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
RN_OK, RN_EUNSUPPORTED = 0, -4


def _api():
    from pytorch_retinanet_amd import _launch, _lib
    return _lib.lib, {torch.bfloat16: _lib.RN_BF16, torch.float16: _lib.RN_F16}, _launch.ptr_array, _launch.stream_on(torch.device(DEV))


def _one_rounding(got, ref, dtype, what):
    scale = 1.0 if dtype == torch.bfloat16 else 0.125
    got, ref = got.float(), ref.float()
    rel = float((got - ref).norm() / (ref.norm() + 1e-20))
    err, top = float((got - ref).abs().max()), float(ref.abs().max())
    print(f"{what}: rel {rel:.3e} (bar {2.5e-3 * scale:.3e})  max err {err:.3e} (bar {2.0 ** -8 * scale * top + 1e-6:.3e})")
    assert rel < 2.5e-3 * scale and err <= 2.0 ** -8 * scale * top + 1e-6, (what, rel, err, top)


def _keep_mask(Hp, Wp, seams, seed):
    "[Hp][Wp] uint8: zero border, zero seam rows / columns, a few random gaps"
    g = torch.Generator(device=DEV).manual_seed(seed)
    m = torch.zeros(Hp, Wp, dtype=torch.uint8, device=DEV)
    m[1:-1, 1:-1] = (torch.rand(Hp - 2, Wp - 2, device=DEV, generator=g) > 0.1).to(torch.uint8)
    if seams:
        m[Hp // 2, :] = 0
        m[:, Wp // 3] = 0
        m[:, Wp // 3 + 1] = 0
    return m


def _canvas(N, C, Hp, Wp, mask2d, dtype, seed, scale=1.0):
    "[N][Hp][Wp][C] (= [M][C]) 16-bit values, zero where the mask is"
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(N, Hp, Wp, C, device=DEV, generator=g) * scale
    return (x * mask2d[None, :, :, None]).to(dtype).contiguous()


def _weight(Cout, Cin, dtype, seed, scale=0.05):
    "[Cout][3][3][Cin]: the kernel's [Cout][9][Cin]"
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(Cout, 3, 3, Cin, device=DEV, generator=g) * scale).to(dtype).contiguous()


def _conv_ref(x, w, bias=None):
    "fp32 conv2d of the canvas [N][Hp][Wp][Cin] with w [Cout][3][3][Cin] -> [N][Hp][Wp][Cout]"
    y = F.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), bias, padding=1)
    return y.permute(0, 2, 3, 1).contiguous()


def _flip(w):
    "data-gradient weights: [Cin][3][3][Cout], taps reversed"
    return w.flip(1, 2).permute(3, 1, 2, 0).contiguous()


def _bits(t):
    "[.., C] bool -> [.., C / 8] uint8, bit j of byte c / 8 = t[.., c + j]"
    sh = t.shape
    b = t.reshape(*sh[:-1], sh[-1] // 8, 8).to(torch.int32)
    wts = (2 ** torch.arange(8, device=t.device, dtype=torch.int32))
    return (b * wts).sum(-1).to(torch.uint8).contiguous()


# (N, Hp, Wp, Cin, seams)
SHAPES = [(1, 20, 6, 64, False),      # 120 positions, 6 wide: one ragged tile whose bands all leave the canvas
          (1, 7, 37, 256, False),     # 259 = 256 + 3: the second tile nearly empty
          (2, 16, 16, 64, True),      # exactly 512
          (2, 14, 37, 256, True)]     # 1 036: five tiles, seams inside the bands, the sheet boundary inside a tile
_CACHE = {}


def _forward_case(shape, dtype, P):
    "inputs, the kernel's outputs and the fp32 reference of one forward case: computed once, shared, not modified"
    key = (shape, dtype, P)
    if key in _CACHE:
        return _CACHE[key]
    lib, DT, ptrs, stream = _api()
    N, Hp, Wp, Cin, seams = shape
    Cout, M = 256, N * Hp * Wp
    mask2d = _keep_mask(Hp, Wp, seams, 1)
    xs = [_canvas(N, Cin, Hp, Wp, mask2d, dtype, 10 + p) for p in range(P)]
    ws = [_weight(Cout, Cin, dtype, 20 + p) for p in range(P)]
    bs = [torch.randn(Cout, device=DEV, generator=torch.Generator(device=DEV).manual_seed(30 + p)) * 0.3 for p in range(P)]

    def run():
        ys = [torch.full((N, Hp, Wp, Cout), float("nan"), dtype=dtype, device=DEV) for _ in range(P)]
        rms = [torch.full((M, Cout // 8), 0xAA, dtype=torch.uint8, device=DEV) for _ in range(P)]
        rc = lib.rn_conv3x3_canvas_batched_ex(ptrs(xs), ptrs(ws), ptrs(bs), mask2d.data_ptr(), ptrs(ys), ptrs(rms), P, DT[dtype], M, Hp * Wp, Wp,
                                              Cin, Cout, 1, stream)
        assert rc == RN_OK, rc
        torch.cuda.synchronize()
        return ys, rms

    ys, rms = run()
    ys2, rms2 = run()
    refs = [torch.relu(_conv_ref(xs[p], ws[p], bs[p])) * mask2d[None, :, :, None].float() for p in range(P)]
    _CACHE[key] = dict(mask2d=mask2d, xs=xs, ws=ws, bs=bs, ys=ys, rms=rms, ys2=ys2, rms2=rms2, refs=refs)
    return _CACHE[key]


@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_output_bias_relu_and_mask_bits(shape, dtype, P):
    "rn_conv3x3_canvas_batched_ex: bias + ReLU + keep mask, the ReLU bits of what was stored, two calls bit-equal"
    c = _forward_case(shape, dtype, P)
    N, Hp, Wp, Cin, _ = shape
    for p in range(P):
        y = c["ys"][p]
        _one_rounding(y, c["refs"][p], dtype, f"forward {shape} {dtype} problem {p}")
        assert not y.float()[:, c["mask2d"] == 0].any()                       # border, seams and gaps are exact zeros (and no NaN is left)
        assert torch.equal(c["rms"][p].view(N, Hp, Wp, -1), _bits(y.float() > 0))
        assert torch.equal(y, c["ys2"][p]) and torch.equal(c["rms"][p], c["rms2"][p])
    if P == 2:                                                                # different weights: the problems are not each other's copies
        assert not torch.equal(c["ys"][0], c["ys"][1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1, 20, 6), (1, 7, 37), (2, 16, 16)])
def test_every_tap_alone_from_the_first_and_last_interior_position(shape, dtype):
    """x is non-zero only at the first and at the last interior position; the weight of tap t alone is the identity on the 64 input
    channels (output channel n copies input channel n % 64): the output is x shifted by the tap, EXACTLY and at every canvas
    position -- a wrong band-row offset or swizzle key moves or scrambles it."""
    lib, DT, _, stream = _api()
    N, Hp, Wp = shape
    Cin, Cout, M = 64, 256, N * Hp * Wp
    x = torch.zeros(N, Hp, Wp, Cin, dtype=dtype, device=DEV)
    x[0, 1, 1] = (torch.arange(Cin, device=DEV) % 13 + 1).to(dtype)
    x[N - 1, Hp - 2, Wp - 2] = (torch.arange(Cin, device=DEV) % 7 + 2).to(dtype)
    for t in range(9):
        w = torch.zeros(Cout, 9, Cin, dtype=dtype, device=DEV)
        w[torch.arange(Cout), t, torch.arange(Cout) % Cin] = 1.0
        y = torch.full((N, Hp, Wp, Cout), float("nan"), dtype=dtype, device=DEV)
        rc = lib.rn_conv3x3_canvas(x.data_ptr(), w.data_ptr(), 0, 0, y.data_ptr(), DT[dtype], M, Hp * Wp, Wp, Cin, Cout, 0, stream)
        assert rc == RN_OK, rc
        # no keep mask in this call, so EVERY canvas position is written, and the canvas formulation is the reference: tap (r, s) of position
        # m is position m + (r - 1) Wp + s - 1, clamped into the canvas (taps 2 and 6 move both points onto border positions, which
        # a padded conv2d would not show)
        src = (torch.arange(M, device=DEV) + (t // 3 - 1) * Wp + (t % 3 - 1)).clamp(0, M - 1)
        ref = x.view(M, Cin)[src][:, torch.arange(Cout, device=DEV) % Cin]
        assert torch.equal(y.view(M, Cout), ref), (shape, dtype, t)
        assert int((ref != 0).any(dim=1).sum()) == 2


@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_data_gradient_relu_mask_and_column_sums(shape, dtype, P):
    """rn_conv3x3_canvas_dgrad_relu_batched: flipped weights, the ReLU backward from a bit mask with dead lanes, the keep mask, and the
    column sums (the bias gradient of the layer below) against the fp32 sum; two calls bit-equal."""
    lib, DT, ptrs, stream = _api()
    N, Hp, Wp, C, seams = shape
    M = N * Hp * Wp
    Cres = 256                                     # the incoming gradient has C channels (the contraction), the result 256
    mask2d = _keep_mask(Hp, Wp, seams, 2)
    gs = [_canvas(N, C, Hp, Wp, mask2d, dtype, 40 + p) for p in range(P)]           # contraction over C channels of g
    ws = [_weight(Cres, C, dtype, 50 + p) for p in range(P)]                         # already in data-gradient layout [Cres][9][C]
    alive = [torch.rand(N, Hp, Wp, Cres, device=DEV, generator=torch.Generator(device=DEV).manual_seed(60 + p)) > 0.4 for p in range(P)]
    for a in alive:
        a[..., 5] = False                                                            # a dead channel
        a[0, 1, 1, :] = False                                                        # and a dead position
    rms = [_bits(a).view(M, Cres // 8) for a in alive]
    ws_bytes = lib.rn_conv3x3_colsum_workspace_bytes(P, M, Cres)
    assert ws_bytes > 0

    def run():
        ys = [torch.full((N, Hp, Wp, Cres), float("nan"), dtype=dtype, device=DEV) for _ in range(P)]
        dbs = [torch.full((Cres,), float("nan"), device=DEV) for _ in range(P)]
        wsp = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        rc = lib.rn_conv3x3_canvas_dgrad_relu_batched(ptrs(gs), ptrs(ws), ptrs(rms), mask2d.data_ptr(), ptrs(ys), ptrs(dbs), P, DT[dtype], M,
                                                      Hp * Wp, Wp, C, Cres, wsp.data_ptr(), ws_bytes, stream)
        assert rc == RN_OK, rc
        torch.cuda.synchronize()
        return ys, dbs

    ys, dbs = run()
    ys2, dbs2 = run()
    for p in range(P):
        ref = _conv_ref(gs[p], ws[p]) * mask2d[None, :, :, None].float() * alive[p].float()
        _one_rounding(ys[p], ref, dtype, f"data gradient {shape} {dtype} problem {p}")
        assert not ys[p].float()[~alive[p]].any() and not ys[p].float()[:, mask2d == 0].any()
        _one_rounding(dbs[p], ref.sum((0, 1, 2)), dtype, f"column sums {shape} {dtype} problem {p}")
        # and they are the sums of what was stored, to fp32 summation order
        stored = ys[p].float().sum((0, 1, 2))
        torch.testing.assert_close(dbs[p], stored, rtol=1e-4, atol=1e-4 * float(stored.abs().max()))
        assert torch.equal(ys[p], ys2[p]) and torch.equal(dbs[p], dbs2[p])


def test_data_gradient_against_autograd():
    "the same entry point with the weights flipped from a forward weight: torch's autograd input gradient of conv2d"
    lib, DT, ptrs, stream = _api()
    dtype = torch.bfloat16
    N, Hp, Wp, C = 2, 14, 37, 256
    M = N * Hp * Wp
    mask2d = _keep_mask(Hp, Wp, True, 3)
    g = _canvas(N, C, Hp, Wp, mask2d, dtype, 70)
    w = _weight(C, C, dtype, 71)                                                     # forward weight [Cout][3][3][Cin]
    x = torch.zeros(N, C, Hp, Wp, device=DEV, requires_grad=True)
    F.conv2d(x, w.float().permute(0, 3, 1, 2), padding=1).backward(g.float().permute(0, 3, 1, 2))
    ref = x.grad.permute(0, 2, 3, 1) * mask2d[None, :, :, None].float()
    wt = _flip(w)
    ones = torch.full((M, C // 8), 0xFF, dtype=torch.uint8, device=DEV)
    y = torch.empty(N, Hp, Wp, C, dtype=dtype, device=DEV)
    db = torch.empty(C, device=DEV)
    nb = lib.rn_conv3x3_colsum_workspace_bytes(1, M, C)
    wsp = torch.empty(nb, dtype=torch.uint8, device=DEV)
    rc = lib.rn_conv3x3_canvas_dgrad_relu_batched(ptrs([g]), ptrs([wt]), ptrs([ones]), mask2d.data_ptr(), ptrs([y]), ptrs([db]), 1, DT[dtype], M,
                                                  Hp * Wp, Wp, C, C, wsp.data_ptr(), nb, stream)
    assert rc == RN_OK, rc
    _one_rounding(y, ref, dtype, "data gradient vs autograd")
    _one_rounding(db, ref.sum((0, 1, 2)), dtype, "bias gradient vs autograd")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1, 20, 6, 64), (1, 7, 37, 256), (2, 14, 37, 256)])
def test_two_source_data_gradient(shape, dtype):
    "rn_conv3x3_canvas_sum2 = conv(g0, w[.., :C]) + conv(g1, w[.., C:]) in one accumulator: fp32 reference, and the sum of two single-source calls"
    lib, DT, _, stream = _api()
    N, Hp, Wp, C = shape
    Cout, M = 256, N * Hp * Wp
    mask2d = _keep_mask(Hp, Wp, True, 4)
    g0, g1 = _canvas(N, C, Hp, Wp, mask2d, dtype, 80), _canvas(N, C, Hp, Wp, mask2d, dtype, 81)
    w0, w1 = _weight(Cout, C, dtype, 82), _weight(Cout, C, dtype, 83)
    wcat = torch.cat([w0, w1], dim=3).contiguous()                                   # [Cout][3][3][2 C]
    y = torch.full((N, Hp, Wp, Cout), float("nan"), dtype=dtype, device=DEV)
    y_again = torch.empty_like(y)
    for out in (y, y_again):
        rc = lib.rn_conv3x3_canvas_sum2(g0.data_ptr(), g1.data_ptr(), wcat.data_ptr(), mask2d.data_ptr(), out.data_ptr(), DT[dtype], M, Hp * Wp, Wp,
                                        C, Cout, stream)
        assert rc == RN_OK, rc
    ref = (_conv_ref(g0, w0) + _conv_ref(g1, w1)) * mask2d[None, :, :, None].float()
    _one_rounding(y, ref, dtype, f"sum2 {shape} {dtype}")
    assert torch.equal(y, y_again)
    # against the sum of two single-source calls.  On random data that sum carries two 16-bit roundings of its own (measured: 1.02 of
    # the per-element bar at bf16, 1.4 at fp16, while sum2 itself is inside it against fp32 above), so the comparison is made where the
    # single-source results are EXACT: operands in {-1, 0, 1}, sparse weights, every sum an integer of at most 128 -- representable in
    # both formats -- and then sum2 must equal the sum of the two calls bit for bit.
    gen = torch.Generator(device=DEV).manual_seed(84)
    tri = lambda sh, density: ((torch.rand(sh, device=DEV, generator=gen) < density).float() * (torch.randint(0, 2, sh, device=DEV, generator=gen) * 2 - 1))
    gi = [(tri((N, Hp, Wp, C), 0.6) * mask2d[None, :, :, None]).to(dtype).contiguous() for _ in range(2)]
    wi = [tri((Cout, 3, 3, C), 8.0 / C).to(dtype).contiguous() for _ in range(2)]
    exact = [_conv_ref(g, w) * mask2d[None, :, :, None].float() for g, w in zip(gi, wi)]
    assert max(float(e.abs().max()) for e in exact) <= 64 and min(float(e.abs().max()) for e in exact) >= 4
    yi = torch.full_like(y, float("nan"))
    rc = lib.rn_conv3x3_canvas_sum2(gi[0].data_ptr(), gi[1].data_ptr(), torch.cat(wi, dim=3).contiguous().data_ptr(), mask2d.data_ptr(), yi.data_ptr(),
                                    DT[dtype], M, Hp * Wp, Wp, C, Cout, stream)
    assert rc == RN_OK, rc
    singles = []
    for g, w, e in zip(gi, wi, exact):
        s = torch.empty_like(y)
        rc = lib.rn_conv3x3_canvas(g.data_ptr(), w.data_ptr(), 0, mask2d.data_ptr(), s.data_ptr(), DT[dtype], M, Hp * Wp, Wp, C, Cout, 0, stream)
        assert rc == RN_OK, rc
        assert torch.equal(s.float(), e)
        singles.append(s.float())
    assert torch.equal(yi.float(), singles[0] + singles[1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_shapes_the_band_walk_does_not_take(dtype):
    "Cout = 512 keeps the tile walk: RN_OK and the same bar; Cout = 128 and Cin = 96 stay RN_EUNSUPPORTED"
    lib, DT, _, stream = _api()
    N, Hp, Wp, Cin, Cout = 1, 7, 37, 64, 512
    M = N * Hp * Wp
    mask2d = _keep_mask(Hp, Wp, False, 5)
    x, w = _canvas(N, Cin, Hp, Wp, mask2d, dtype, 90), _weight(Cout, Cin, dtype, 91)
    b = torch.randn(Cout, device=DEV, generator=torch.Generator(device=DEV).manual_seed(92)) * 0.3
    y = torch.full((N, Hp, Wp, Cout), float("nan"), dtype=dtype, device=DEV)
    rc = lib.rn_conv3x3_canvas(x.data_ptr(), w.data_ptr(), b.data_ptr(), mask2d.data_ptr(), y.data_ptr(), DT[dtype], M, Hp * Wp, Wp, Cin, Cout, 1, stream)
    assert rc == RN_OK, rc
    _one_rounding(y, torch.relu(_conv_ref(x, w, b)) * mask2d[None, :, :, None].float(), dtype, f"tile-walk fallback {dtype}")
    p = x.data_ptr()
    assert lib.rn_conv3x3_canvas(p, p, 0, 0, p, DT[dtype], M, Hp * Wp, Wp, 64, 128, 0, stream) == RN_EUNSUPPORTED
    assert lib.rn_conv3x3_canvas(p, p, 0, 0, p, DT[dtype], M, Hp * Wp, Wp, 96, 256, 0, stream) == RN_EUNSUPPORTED
