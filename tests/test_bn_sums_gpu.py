"""GPU: every row enters every fused BatchNorm sum exactly once, and the finalizers / the variance scheme against float64.

The BatchNorm statistics of the training step come out of fused kernels (GEMM / conv epilogues, the pooling backward) as
per-row-tile ``partial`` arrays f32 [rows][2][C] which ``rn_bn_stats_finalize`` / ``rn_bn_bwd_finalize`` combine in double.

1. Row census.  Operands are 0 / 1 (or small integers) with a period over the row index, so that the stored output is exactly
   0.0 / 1.0 and a column sum is a COUNT of rows: the sums are integers below 2^24 and every assertion is exact.  Expected
   values are the same operation on the host in float64.  Two coprime periods (7 and 8): a dropped row paired with a doubled
   one cannot cancel in both.  Where a producer reads ReLU bit rows [M][C / 8], a second census has all-ones data and the bits
   set on the rows with ``i % 3 == 0``: reading a neighbour's bit row changes the count.  Row counts: 1, 127, 128, 129,
   3 * 128 + 1 and, per walker kernel, the first row count with more row tiles than walkers (read from the ``*_walkers()``
   exports at run time) plus one more tile.  This judges the epilogues' row bookkeeping, not the matrix arithmetic.
2. The two finalizers alone on synthetic partials against float64 (numpy long double sums of the same fp32 partials).
3. The variance scheme (fp32 block sums, ``q / M - mean^2`` in double) against float64 when |mean| / std is 0, 4 and 32, with
   two yardsticks measured on the same input: torch's fp32 batch norm and a numpy restatement of the documented scheme.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H16 = [torch.bfloat16, torch.float16]
PERIODS = (7, 8)
ROWS = [1, 127, 128, 129, 3 * 128 + 1]
BIG = ["cap+1", "cap+129"]           # the first row count with more row tiles than walkers, and one tile more


# ---------------------------------------------------------------------------------------------------------------- helpers
def _rn(dtype):
    from pytorch_retinanet_amd._lib import RN_BF16, RN_F16, RN_F32
    return {torch.float32: RN_F32, torch.bfloat16: RN_BF16, torch.float16: RN_F16}[dtype]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _rows(M, Cc, P, dtype):
    "x[i, c] = [c == (i mod P) mod min(P, C)]: one 1 per row, period P over the row index."
    i = torch.arange(M, device=DEV)
    x = torch.zeros((M, Cc), dtype=dtype, device=DEV)
    x[i, (i % P) % min(P, Cc)] = 1
    return x


def _rows_all(M, Cc, P, dtype):
    "x[i, c] = [c mod P == i mod P]: the same period in every channel group (for the kernels that do not contract over c)."
    i, c = torch.arange(M, device=DEV)[:, None], torch.arange(Cc, device=DEV)[None, :]
    return ((c % P) == (i % P)).to(dtype).contiguous()


def _sel(N, Cc, P, dtype, k=1):
    "w[n, c, centre tap] = [c == n mod min(P, C)], so (x . w^T)[i, n] = [(i mod P) mod k == n mod k] -- exactly 0 or 1."
    w = torch.zeros((N, Cc, k, k), dtype=dtype, device=DEV)
    n = torch.arange(N, device=DEV)
    w[n, n % min(P, Cc), k // 2, k // 2] = 1
    return w.contiguous(memory_format=torch.channels_last)


def _img(rows, Nimg, H, W):
    "[M, C] rows -> the channels-last [Nimg, C, H, W] tensor with the same memory."
    return rows.view(Nimg, H, W, rows.shape[1]).permute(0, 3, 1, 2)


def _flat(t):
    "channels-last [Nimg, C, H, W] -> [M, C] float64 on the host."
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).double().cpu()


def _rowbits(alive_rows, Cc):
    "ReLU bit rows u8 [M][C / 8]: every bit of row i set iff alive_rows[i]."
    return (alive_rows.to(torch.uint8) * 255)[:, None].expand(-1, Cc // 8).contiguous().view(-1)


def _pack(mask):
    M, Cc = mask.shape
    return (mask.view(M, Cc // 8, 8).to(torch.int32) * (2 ** torch.arange(8, device=mask.device, dtype=torch.int32))).sum(-1).to(torch.uint8).view(-1)


def _unit(Cc):
    "f32 [ones(C) | zeros(C)] and the two pointers: a = 1, b = 0 (also invstd = 1, mean = 0)."
    t = torch.cat([torch.ones(Cc, device=DEV), torch.zeros(Cc, device=DEV)])
    return t, t.data_ptr(), t.data_ptr() + 4 * Cc


def _nan(n):
    return torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)


def _sums(partial, nb, Cc):
    return partial.view(nb, 2, Cc).double().sum(0).cpu()


def _same(got, want, what):
    got, want = got.double().cpu(), want.double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (got != want) | torch.isnan(got)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} differ, first at {bad.nonzero()[0].tolist()}: " \
                                f"got {got[bad][0].item()} want {want[bad][0].item()}"


def _cap(walkers):
    "Largest number of 128-row tiles that still gets a walker each (the export's cu_count()-dependent cap)."
    lo, hi = 1, 1 << 20
    assert walkers(128 * lo) >= lo
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if walkers(128 * mid) >= mid:
            lo = mid
        else:
            hi = mid - 1
    return lo


def _M(rows, walkers):
    if isinstance(rows, int):
        return rows
    cap = _cap(walkers)
    M = cap * 128 + (1 if rows == "cap+1" else 129)
    assert walkers(M) < (M + 127) // 128, "the shape does not reach the multi-round regime"
    return M


# ------------------------------------------------------------------------------------------ 1. census: forward producers
@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("rows,N", [(r, 64) for r in ROWS + BIG] + [(r, 128) for r in ROWS])
def test_census_pw_conv_forward_statistics(rows, N, dtype):
    "rn_pw_conv_forward + RN_PW_EPI_STATS, 1x1: plain and with the relu(x * 1 + 0) prologue; both column-tile widths (64, 128)."
    from pytorch_retinanet_amd import pwconv
    from pytorch_retinanet_amd._lib import lib
    M = _M(rows, lib.rn_pw_walkers)
    print(f"rn_pw_walkers({M}) = {lib.rn_pw_walkers(M)} for {(M + 127) // 128} row tiles")
    coef, _, _ = _unit(64)
    for P in PERIODS:
        xr, w = _rows(M, 64, P, dtype), _sel(N, 64, P, dtype)
        want = xr.double().cpu() @ w.view(N, 64).double().cpu().t()
        for pro in (None, pwconv.affine_relu(coef)):
            epi, partial, nb = pwconv.stats_epilogue(M, N, torch.device(DEV))
            partial.fill_(float("nan"))
            y = pwconv.pw_forward(_img(xr, 1, 1, M), w, pro=pro, epi=epi)
            what = f"M={M} N={N} period {P} prologue {'none' if pro is None else 'affine_relu'}"
            _same(_flat(y), want, "output, " + what)
            s = _sums(partial, nb, N)
            _same(s[0], want.sum(0), "column sums, " + what)
            _same(s[1], want.sum(0), "column sums of squares, " + what)


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("k,stride,H,W", [(1, 2, 1, 7), (1, 2, 19, 23), (3, 1, 19, 23), (3, 2, 19, 23), (3, 2, 1, 7), (3, 1, 1, 1)])
def test_census_pw_conv_forward_statistics_strided_and_3x3(k, stride, H, W, dtype):
    "The same through the position walk of the strided / 3 x 3 forms (weight on the centre tap; odd H and W)."
    from pytorch_retinanet_amd import pwconv
    Nimg = 2
    for P in PERIODS:
        x = _img(_rows(Nimg * H * W, 64, P, dtype), Nimg, H, W)
        w = _sel(64, 64, P, dtype, k)
        ref = F.conv2d(x.double().cpu(), w.double().cpu(), None, stride, k // 2)
        want = _flat(ref)
        M = want.shape[0]
        epi, partial, nb = pwconv.stats_epilogue(M, 64, torch.device(DEV))
        partial.fill_(float("nan"))
        y = pwconv.pw_forward(x, w, stride=stride, epi=epi)
        what = f"{k}x{k} stride {stride} {H}x{W} period {P}"
        assert tuple(y.shape) == tuple(ref.shape)
        _same(_flat(y), want, "output, " + what)
        s = _sums(partial, nb, 64)
        _same(s[0], want.sum(0), "column sums, " + what)
        _same(s[1], want.sum(0), "column sums of squares, " + what)


def _chain_call(M, c4, cn, dtype, z3, res, w1, ra):
    from pytorch_retinanet_amd._lib import lib
    nb = lib.rn_pw_block_out_conv1_walkers(M, c4, cn)
    assert nb > 0
    unit, one, zero = _unit(c4)
    y = torch.full((M, c4), float("nan"), dtype=dtype, device=DEV)
    bits = torch.zeros((M * c4 // 8,), dtype=torch.uint8, device=DEV)
    z1 = torch.full((M, cn), float("nan"), dtype=dtype, device=DEV)
    part = _nan(nb * 2 * cn)
    rc = lib.rn_pw_block_out_conv1(M, c4, cn, _rn(dtype), z3.data_ptr(), res.data_ptr(), one if ra else 0, zero if ra else 0, one, zero,
                                   w1.data_ptr(), y.data_ptr(), bits.data_ptr(), z1.data_ptr(), part.data_ptr(), _st())
    assert rc == 0
    torch.cuda.synchronize()
    return y, bits, z1, part, nb


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("rows,c4,cn", [(r, 256, 64) for r in ROWS + BIG] + [(r, c4, cn) for r in (1, 129, 385) for c4, cn in ((256, 128), (512, 128))])
def test_census_block_out_conv1(rows, c4, cn, dtype):
    "rn_pw_block_out_conv1: block output y, its ReLU bits, the next conv1's z1 and z1's column sums."
    from pytorch_retinanet_amd._lib import lib
    M = _M(rows, lambda m: lib.rn_pw_block_out_conv1_walkers(m, c4, cn))
    print(f"rn_pw_block_out_conv1_walkers({M}, {c4}, {cn}) = {lib.rn_pw_block_out_conv1_walkers(M, c4, cn)} for {(M + 127) // 128} row tiles")
    for P in PERIODS:
        # y = relu(z3 * 1 + 0 + resid): the pattern comes half from z3 and half from the residual (even / odd rows)
        pat = _rows(M, c4, P, dtype)
        even = (torch.arange(M, device=DEV) % 2 == 0)[:, None]
        z3, res = pat * even, pat * ~even
        w1 = _sel(cn, c4, P, dtype)
        want = pat.double().cpu() @ w1.view(cn, c4).double().cpu().t()
        for ra in ((False, True) if isinstance(rows, int) else (False,)):
            y, bits, z1, part, nb = _chain_call(M, c4, cn, dtype, z3, res, w1, ra)
            what = f"M={M} ({c4}, {cn}) period {P} res_affine {ra}"
            _same(y, pat, "block output, " + what)
            assert torch.equal(bits, _pack(pat > 0)), "ReLU bits, " + what
            _same(z1, want, "z1, " + what)
            s = _sums(part, nb, cn)
            _same(s[0], want.sum(0), "column sums, " + what)
            _same(s[1], want.sum(0), "column sums of squares, " + what)


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("rows,cm,c4", [(r, 64, 256) for r in ROWS + BIG] + [(r, cm, c4) for r in (1, 129, 385) for cm, c4 in ((128, 512), (64, 128))])
def test_census_conv3_forward(rows, cm, c4, dtype):
    "rn_pw_conv3_forward: z3 = relu(z2 * 1 + 0) . w3^T and its column sums."
    from pytorch_retinanet_amd._lib import lib
    M = _M(rows, lambda m: lib.rn_pw_conv3_forward_walkers(m, cm, c4))
    nb = lib.rn_pw_conv3_forward_walkers(M, cm, c4)
    print(f"rn_pw_conv3_forward_walkers({M}, {cm}, {c4}) = {nb} for {(M + 127) // 128} row tiles")
    assert nb > 0
    coef, _, _ = _unit(cm)
    for P in PERIODS:
        z2, w3 = _rows(M, cm, P, dtype), _sel(c4, cm, P, dtype)
        want = z2.double().cpu() @ w3.view(c4, cm).double().cpu().t()
        z3 = torch.full((M, c4), float("nan"), dtype=dtype, device=DEV)
        part = _nan(nb * 2 * c4)
        assert lib.rn_pw_conv3_forward(M, cm, c4, _rn(dtype), z2.data_ptr(), coef.data_ptr(), w3.data_ptr(), z3.data_ptr(), part.data_ptr(), _st()) == 0
        what = f"M={M} ({cm}, {c4}) period {P}"
        _same(z3, want, "z3, " + what)
        s = _sums(part, nb, c4)
        _same(s[0], want.sum(0), "column sums, " + what)
        _same(s[1], want.sum(0), "column sums of squares, " + what)


def _stem_call(x, w, dtype):
    from pytorch_retinanet_amd._lib import check, lib
    B, _, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = torch.empty((lib.rn_stem_padded_bytes(B, H, W),), dtype=torch.uint8, device=DEV)
    wk = torch.empty((64 * 7 * 32,), dtype=dtype, device=DEV)
    z = torch.full((B, 64, Ho, Wo), float("nan"), dtype=dtype, device=DEV).contiguous(memory_format=torch.channels_last)
    nb = lib.rn_stem_partial_rows(B, H, W)
    part = _nan(nb * 2 * 64)
    check(lib.rn_stem_conv_forward(x.data_ptr(), w.data_ptr(), xp.data_ptr(), wk.data_ptr(), z.data_ptr(), part.data_ptr(), _rn(dtype), B, H, W, _st()),
          "rn_stem_conv_forward")
    return z, part, nb


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("B,H,W", [(1, 7, 7), (2, 37, 53), (1, 3, 161)])
def test_census_stem_conv_forward(B, H, W, dtype):
    """rn_stem_conv_forward (7x7 / stride 2): weight on the centre tap, so the output is the image at the even positions.
    (1, 3, 161): 6 column tiles per output row against 4 tiles per workgroup -- one output row spans two workgroups."""
    for P in PERIODS:
        x = _img(_rows(B * H * W, 3, P, dtype), B, H, W)
        w = _sel(64, 3, P, dtype, 7)
        ref = F.conv2d(x.double().cpu(), w.double().cpu(), None, 2, 3)
        want = _flat(ref)
        z, part, nb = _stem_call(x, w, dtype)
        what = f"({B}, {H}, {W}) period {P}, {nb} partial rows"
        assert tuple(z.shape) == tuple(ref.shape)
        _same(_flat(z), want, "output, " + what)
        s = _sums(part, nb, 64)
        _same(s[0], want.sum(0), "column sums, " + what)
        _same(s[1], want.sum(0), "column sums of squares, " + what)


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("N,h,wd", [(1, 16, 16), (1, 1, 257), (2, 13, 23)])
def test_census_dense_band_statistics(N, h, wd, dtype):
    "rn_conv3x3_dense_band_stats (256-position row tiles): one full tile, the first shape with two tiles (257 positions), a ragged one."
    from pytorch_retinanet_amd import biasact
    for P in PERIODS:
        x = _img(_rows(N * h * wd, 64, P, dtype), N, h, wd)
        w = _sel(128, 64, P, dtype, 3)
        want = _flat(F.conv2d(x.double().cpu(), w.double().cpu(), None, 1, 1))
        y, partial, tiles = biasact.conv3x3_dense_band_stats(x, w)
        assert tiles == (N * h * wd + 255) // 256
        what = f"({N}, {h}, {wd}) period {P}, {tiles} tiles"
        _same(_flat(y), want, "output, " + what)
        s = _sums(partial, tiles, 128)
        _same(s[0], want.sum(0), "column sums, " + what)
        _same(s[1], want.sum(0), "column sums of squares, " + what)


@pytest.mark.parametrize("dtype", [torch.float32] + H16)
@pytest.mark.parametrize("Cc", [8, 2056])
@pytest.mark.parametrize("M", [1, 9, 1031])
def test_census_bn_stats(M, Cc, dtype):
    """rn_bn_stats keeps its partials in its workspace, so the census reads what the finalizer makes of them: with exact
    integer sums s = q = count, mean = s / M is the correctly rounded quotient (exact comparison) and invstd follows in double."""
    from pytorch_retinanet_amd import norm
    from pytorch_retinanet_amd._lib import check, lib
    eps = 1e-5
    for P in PERIODS:
        x = _rows_all(M, Cc, P, dtype)
        count = x.double().sum(0).cpu().numpy()
        out = torch.full((4 * Cc,), float("nan"), dtype=torch.float32, device=DEV)
        rm, rv = torch.zeros(Cc, device=DEV), torch.zeros(Cc, device=DEV)
        wp, wn = norm._workspace(torch.device(DEV), _st(), Cc)
        sp = out.data_ptr()
        check(lib.rn_bn_stats(x.data_ptr(), _rn(dtype), M, Cc, 0, 0, rm.data_ptr(), rv.data_ptr(), 0, 1.0, eps, sp, sp + 4 * Cc, sp + 8 * Cc, wp, wn, _st()),
              "rn_bn_stats")
        got = out.cpu().numpy()
        mean = count / M
        var = np.maximum(count / M - mean * mean, 0.0)
        what = f"M={M} C={Cc} period {P}"
        assert np.array_equal(got[:Cc], mean.astype(np.float32)), "mean (= count / M), " + what
        assert np.array_equal(rm.cpu().numpy(), mean.astype(np.float32)), "running mean at momentum 1, " + what
        inv = 1.0 / np.sqrt(var + np.float64(np.float32(eps)))
        ulp = np.spacing(inv.astype(np.float32))
        assert np.all(np.abs(got[Cc:2 * Cc].astype(np.float64) - inv) <= ulp), "invstd (sum of squares = count), " + what


# ----------------------------------------------------------------------------------------- 1. census: backward producers
def _relu_bwd_epilogue(M, N, zprev):
    "RN_PW_EPI_RELU_BWD with ea = 1, eb = 0, emean = 0, einv = 1: mask = [zprev > 0], xhat = zprev."
    from pytorch_retinanet_amd._lib import RN_PW_EPI_RELU_BWD, RnPwEpilogue, lib
    nb = lib.rn_pw_walkers(M)
    part = _nan(nb * 2 * N)
    unit, one, zero = _unit(N)
    return RnPwEpilogue(RN_PW_EPI_RELU_BWD, part.data_ptr(), 0, 0, zprev.data_ptr(), one, zero, zero, one), part, nb, unit


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("rows,N", [(r, 64) for r in ROWS + BIG] + [(r, 128) for r in (1, 129, 385)])
def test_census_pw_conv_forward_relu_backward_epilogue(rows, N, dtype):
    """rn_pw_conv_forward + RN_PW_PRO_BN_BWD (a = 1, k0 = k1 = 0) + RN_PW_EPI_RELU_BWD with zprev = 2 (alive, xhat = 2):
    sum g' = count, sum g' xhat = 2 * count.  Row census through relu_mode 0; bit-row censuses: relu_mode 3 (bits), relu_mode 2
    (mask recomputed from x2 = the row pattern) and the epilogue's own mask (zprev = 2 on the rows i % 3 == 0, else 0)."""
    from pytorch_retinanet_amd import pwconv
    from pytorch_retinanet_amd._lib import lib
    M = _M(rows, lib.rn_pw_walkers)
    Cin = 64
    coef3 = torch.cat([torch.ones(Cin, device=DEV), torch.zeros(2 * Cin, device=DEV)])
    fwd, _, _ = _unit(Cin)
    zero_x2 = torch.zeros((M, Cin), dtype=dtype, device=DEV)
    third = torch.arange(M, device=DEV) % 3 == 0
    two = torch.full((M, N), 2.0, dtype=dtype, device=DEV)

    def run(x, w, pro, zprev, want, what):
        epi, part, nb, keep = _relu_bwd_epilogue(M, N, zprev)
        y = pwconv.pw_forward(_img(x, 1, 1, M), w, pro=pro, epi=epi)
        _same(_flat(y), want, "output, " + what)
        s = _sums(part, nb, N)
        _same(s[0], want.sum(0), "sum g', " + what)
        _same(s[1], 2 * want.sum(0), "sum g' xhat, " + what)

    for P in PERIODS:
        xr, w = _rows(M, Cin, P, dtype), _sel(N, Cin, P, dtype)
        want = xr.double().cpu() @ w.view(N, Cin).double().cpu().t()
        run(xr, w, pwconv.bn_bwd(coef3, zero_x2, 0), two, want, f"row census M={M} N={N} period {P}")
    ones, w = torch.ones((M, Cin), dtype=dtype, device=DEV), _sel(N, Cin, 8, dtype)
    want = third.double().cpu()[:, None].expand(M, N).contiguous()
    bits = _rowbits(third, Cin)
    run(ones, w, pwconv.bn_bwd(coef3, zero_x2, 3, bits=bits), two, want, f"bit rows (relu_mode 3) M={M} N={N}")
    x2 = third[:, None].expand(M, Cin).to(dtype).contiguous()
    run(ones, w, pwconv.bn_bwd(coef3, x2, 2, fwd_coef=fwd), two, want, f"mask from x2 (relu_mode 2) M={M} N={N}")
    run(ones, w, pwconv.bn_bwd(coef3, zero_x2, 0), two * third[:, None], want, f"epilogue mask rows (zprev) M={M} N={N}")


def _dgrad_call(M, cm, c4, dtype, dz1, w1t, resid, rbits, rs, H, W, pz3, pbits):
    from pytorch_retinanet_amd._lib import lib
    nb = lib.rn_pw_dgrad_resid_sums_walkers(M, cm, c4)
    assert nb > 0
    unit, one, zero = _unit(c4)
    dx = torch.full((M, c4), float("nan"), dtype=dtype, device=DEV)
    part = _nan(nb * 2 * c4)
    rc = lib.rn_pw_dgrad_resid_sums(M, cm, c4, _rn(dtype), dz1.data_ptr(), w1t.data_ptr(), resid.data_ptr(), rbits.data_ptr() if rbits is not None else 0,
                                    rs, H, W, pz3.data_ptr(), pbits.data_ptr(), zero, one, dx.data_ptr(), part.data_ptr(), _st())
    assert rc == 0
    torch.cuda.synchronize()
    return dx, part, nb


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("rows,cm,c4", [(r, 64, 256) for r in ROWS + BIG] + [(r, 128, 512) for r in (1, 129, 385)])
def test_census_dgrad_resid_sums(rows, cm, c4, dtype):
    """rn_pw_dgrad_resid_sums: dx = dz1 . w1t^T + resid * rbits and the previous block's (sum g', sum g' xhat), g' = dx * prev_bits,
    with prev_z3 = 2, mean 0, invstd 1 (xhat = 2).  Row census: the pattern through the GEMM (resid = 0).  Bit rows: all-ones data
    through the residual with rbits on the rows i % 3 == 0; all-ones dx with prev_bits on those rows."""
    from pytorch_retinanet_amd._lib import lib
    M = _M(rows, lambda m: lib.rn_pw_dgrad_resid_sums_walkers(m, cm, c4))
    print(f"rn_pw_dgrad_resid_sums_walkers({M}, {cm}, {c4}) = {lib.rn_pw_dgrad_resid_sums_walkers(M, cm, c4)} for {(M + 127) // 128} row tiles")
    third = torch.arange(M, device=DEV) % 3 == 0
    all_rows = torch.ones(M, dtype=torch.bool, device=DEV)
    pz3 = torch.full((M, c4), 2.0, dtype=dtype, device=DEV)
    zeros_r, ones_r = torch.zeros((M, c4), dtype=dtype, device=DEV), torch.ones((M, c4), dtype=dtype, device=DEV)
    zeros_g = torch.zeros((M, cm), dtype=dtype, device=DEV)

    def check(dx, part, nb, want_dx, want_g, what):
        _same(dx, want_dx, "dx, " + what)
        s = _sums(part, nb, c4)
        _same(s[0], want_g.sum(0), "sum g', " + what)
        _same(s[1], 2 * want_g.sum(0), "sum g' xhat, " + what)

    for P in PERIODS:
        dz1, w1t = _rows(M, cm, P, dtype), _sel(c4, cm, P, dtype)
        want = dz1.double().cpu() @ w1t.view(c4, cm).double().cpu().t()
        dx, part, nb = _dgrad_call(M, cm, c4, dtype, dz1, w1t, zeros_r, _rowbits(all_rows, c4), 1, 0, 0, pz3, _rowbits(all_rows, c4))
        check(dx, part, nb, want, want, f"row census M={M} ({cm}, {c4}) period {P}")
    w1t = _sel(c4, cm, 8, dtype)
    rows3 = third.double().cpu()[:, None].expand(M, c4).contiguous()
    dx, part, nb = _dgrad_call(M, cm, c4, dtype, zeros_g, w1t, ones_r, _rowbits(third, c4), 1, 0, 0, pz3, _rowbits(all_rows, c4))
    check(dx, part, nb, rows3, rows3, f"rbits rows M={M} ({cm}, {c4})")
    dx, part, nb = _dgrad_call(M, cm, c4, dtype, zeros_g, w1t, ones_r, _rowbits(all_rows, c4), 1, 0, 0, pz3, _rowbits(third, c4))
    check(dx, part, nb, torch.ones(M, c4, dtype=torch.float64), rows3, f"prev_bits rows M={M} ({cm}, {c4})")


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("H,W", [(1, 7), (19, 23)])
def test_census_dgrad_resid_sums_stride2_join(H, W, dtype):
    "The same with the stride-2 downsample gradient joining at the even (y, x) of an odd-sized grid: dx in {0, 1, 2}, sums exact."
    cm, c4, Nimg = 64, 256, 2
    M = Nimg * H * W
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    all_rows = torch.ones(M, dtype=torch.bool, device=DEV)
    pz3 = torch.full((M, c4), 2.0, dtype=dtype, device=DEV)
    for P in PERIODS:
        dz1, w1t = _rows(M, cm, P, dtype), _sel(c4, cm, P, dtype)
        resid = _rows_all(Nimg * Hc * Wc, c4, P, dtype)
        full = torch.zeros((Nimg, H, W, c4), dtype=torch.float64)
        full[:, ::2, ::2] = resid.double().cpu().view(Nimg, Hc, Wc, c4)
        want = dz1.double().cpu() @ w1t.view(c4, cm).double().cpu().t() + full.view(M, c4)
        dx, part, nb = _dgrad_call(M, cm, c4, dtype, dz1, w1t, resid, None, 2, H, W, pz3, _rowbits(all_rows, c4))
        what = f"stride-2 join {H}x{W} period {P}"
        _same(dx, want, "dx, " + what)
        s = _sums(part, nb, c4)
        _same(s[0], want.sum(0), "sum g', " + what)
        _same(s[1], 2 * want.sum(0), "sum g' xhat, " + what)


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("rows,cm,c4", [(r, cm, c4) for cm, c4 in ((64, 256), (128, 512)) for r in ROWS + BIG])
def test_census_conv3_backward(rows, cm, c4, dtype):
    """rn_pw_conv3_backward: dy2 = (g * bits) . w3t^T masked by relu(z2) with z2 = 2 (alive, xhat = 2), and bn2's backward sums.
    The partial rows start as NaN: with Cm = 128 the walker count is rounded up to a multiple of 8 and the idle ones must write
    zeros.  Bit rows: all-ones g with the bits on the rows i % 3 == 0."""
    from pytorch_retinanet_amd._lib import lib
    M = _M(rows, lambda m: lib.rn_pw_conv3_backward_walkers(m, cm, c4))
    nb = lib.rn_pw_conv3_backward_walkers(M, cm, c4)
    print(f"rn_pw_conv3_backward_walkers({M}, {cm}, {c4}) = {nb} for {(M + 127) // 128} row tiles")
    assert nb > 0
    coef3 = torch.cat([torch.ones(c4, device=DEV), torch.zeros(2 * c4, device=DEV)])
    unit, one, zero = _unit(cm)
    z3 = torch.zeros((M, c4), dtype=dtype, device=DEV)
    z2 = torch.full((M, cm), 2.0, dtype=dtype, device=DEV)
    ws = torch.empty((lib.rn_pw_conv3_backward_workspace_bytes(M, cm, c4),), dtype=torch.uint8, device=DEV)
    third = torch.arange(M, device=DEV) % 3 == 0
    all_rows = torch.ones(M, dtype=torch.bool, device=DEV)

    def run(g, w3t, bits, want, what):
        part = _nan(nb * 2 * cm)
        dy2 = torch.full((M, cm), float("nan"), dtype=dtype, device=DEV)
        S = C.c_int(0)
        p3 = coef3.data_ptr()
        rc = lib.rn_pw_conv3_backward(M, cm, c4, _rn(dtype), g.data_ptr(), z3.data_ptr(), bits.data_ptr(), p3, p3 + 4 * c4, p3 + 8 * c4, w3t.data_ptr(),
                                      z2.data_ptr(), one, zero, zero, one, dy2.data_ptr(), part.data_ptr(), ws.data_ptr(), ws.numel(), C.byref(S), _st())
        assert rc == 0 and S.value == nb
        _same(dy2, want, "dy2, " + what)
        s = _sums(part, nb, cm)
        _same(s[0], want.sum(0), "sum g', " + what)
        _same(s[1], 2 * want.sum(0), "sum g' xhat, " + what)

    for P in PERIODS:
        g, w3t = _rows(M, c4, P, dtype), _sel(cm, c4, P, dtype)
        want = g.double().cpu() @ w3t.view(cm, c4).double().cpu().t()
        run(g, w3t, _rowbits(all_rows, c4), want, f"row census M={M} ({cm}, {c4}) period {P}")
    # all-ones g: every one of the C4 inputs of an output column would add up, so the weight picks ONE input channel per column
    w3t = _sel(cm, c4, c4, dtype)
    want = third.double().cpu()[:, None].expand(M, cm).contiguous()
    run(torch.ones((M, c4), dtype=dtype, device=DEV), w3t, _rowbits(third, c4), want, f"bit rows M={M} ({cm}, {c4})")


@pytest.mark.parametrize("dtype", [torch.float32] + H16)
@pytest.mark.parametrize("Cc", [8, 2056])
@pytest.mark.parametrize("M", [1, 9, 1031])
def test_census_bn_bwd_reduce(M, Cc, dtype):
    """rn_bn_bwd_reduce with x = 2, mean 0, invstd 1 (xhat = 2): dbeta = count and dgamma = 2 * count exactly, in every ReLU mode
    (none / mask from y / recomputed from x / bit rows)."""
    from pytorch_retinanet_amd import norm
    from pytorch_retinanet_amd._lib import check, lib
    unit, one, zero = _unit(Cc)
    x = torch.full((M, Cc), 2.0, dtype=dtype, device=DEV)
    third = torch.arange(M, device=DEV) % 3 == 0
    wp, wn = norm._workspace(torch.device(DEV), _st(), Cc)

    def run(dy, y, relu, want, what):
        out = torch.full((5 * Cc,), float("nan"), dtype=torch.float32, device=DEV)       # dgamma | dbeta | coef3
        gp = out.data_ptr()
        check(lib.rn_bn_bwd_reduce(dy.data_ptr(), y.data_ptr() if y is not None else 0, x.data_ptr(), _rn(dtype), M, Cc, 0, zero, one, one, 1, relu,
                                   gp, gp + 4 * Cc, gp + 8 * Cc, wp, wn, _st()), "rn_bn_bwd_reduce")
        got = out.double().cpu()
        _same(got[Cc:2 * Cc], want, "dbeta = sum g', " + what)
        _same(got[:Cc], 2 * want, "dgamma = sum g' xhat, " + what)

    for P in PERIODS:
        dy = _rows_all(M, Cc, P, dtype)
        count = dy.double().sum(0).cpu()
        what = f"M={M} C={Cc} period {P}"
        run(dy, None, 0, count, "no ReLU, " + what)
        run(dy, torch.ones_like(dy), 1, count, "mask from y, " + what)
        run(dy, None, 1, count, "mask recomputed from x, " + what)
        run(dy, _rowbits(torch.ones(M, dtype=torch.bool, device=DEV), Cc), 2, count, "bit rows all set, " + what)
    ones = torch.ones((M, Cc), dtype=dtype, device=DEV)
    n3 = torch.full((Cc,), float(int(third.sum())), dtype=torch.float64)
    run(ones, _rowbits(third, Cc), 2, n3, f"bit rows i % 3 == 0, M={M} C={Cc}")
    run(ones, third[:, None].expand(M, Cc).to(dtype).contiguous(), 1, n3, f"y rows i % 3 == 0, M={M} C={Cc}")


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("N,H,W", [(1, 1, 1), (2, 7, 9), (1, 38, 54), (1, 363, 363)])
def test_census_maxpool_backward_bn(N, H, W, dtype):
    """rn_maxpool3x3s2_backward_bn with z = 2, forward coefficients (1, 0), mean 0, invstd 1 (alive, xhat = 2).  Arg-max codes of a
    random tensor (decoded on the host: code = 3 * row + column inside the window at (2 oy - 1, 2 ox - 1)), pooled gradient = the
    row pattern: dx is a sum of at most four 0 / 1 values.  (1, 363, 363): more 2 x 2 blocks than the 1024 partial rows take in
    one round of the grid-stride loop."""
    from pytorch_retinanet_amd._lib import check, lib
    Cc = 64
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    g = torch.Generator(device=DEV).manual_seed(1)
    src = torch.randn((N, H, W, Cc), device=DEV, generator=g).to(dtype).permute(0, 3, 1, 2)
    pooled = torch.empty((N, Cc, OH, OW), dtype=dtype, device=DEV).contiguous(memory_format=torch.channels_last)
    arg = torch.empty((N, Cc, OH, OW), dtype=torch.uint8, device=DEV).contiguous(memory_format=torch.channels_last)
    check(lib.rn_maxpool3x3s2_forward(src.data_ptr(), pooled.data_ptr(), arg.data_ptr(), _rn(dtype), N, H, W, Cc, _st()), "rn_maxpool3x3s2_forward")
    code = arg.permute(0, 2, 3, 1).long().cpu()                                        # [N, OH, OW, C]
    oy, ox = torch.arange(OH).view(1, OH, 1, 1), torch.arange(OW).view(1, 1, OW, 1)
    iy, ix = 2 * oy - 1 + code // 3, 2 * ox - 1 + code % 3
    assert bool(((code < 9) & (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)).all()), "arg-max codes outside their image"
    n_i = torch.arange(N).view(N, 1, 1, 1).expand_as(code)
    c_i = torch.arange(Cc).view(1, 1, 1, Cc).expand_as(code)
    rows = lib.rn_maxpool3x3s2_backward_bn_rows(N, H, W, Cc)
    print(f"rn_maxpool3x3s2_backward_bn_rows({N}, {H}, {W}, {Cc}) = {rows} for {N * ((H + 1) // 2) * ((W + 1) // 2) * Cc // 8} threads of work")
    assert rows > 0
    unit, one, zero = _unit(Cc)
    z = torch.full((N * H * W, Cc), 2.0, dtype=dtype, device=DEV)
    for P in PERIODS:
        dy = _rows_all(N * OH * OW, Cc, P, dtype)
        want = torch.zeros((N, H, W, Cc), dtype=torch.float64)
        want.index_put_((n_i, iy.expand_as(code), ix.expand_as(code), c_i), dy.double().cpu().view(N, OH, OW, Cc), accumulate=True)
        want = want.view(-1, Cc)
        dx = torch.full((N * H * W, Cc), float("nan"), dtype=dtype, device=DEV)
        part = _nan(rows * 2 * Cc)
        check(lib.rn_maxpool3x3s2_backward_bn(arg.data_ptr(), dy.data_ptr(), z.data_ptr(), unit.data_ptr(), zero, one, dx.data_ptr(), part.data_ptr(),
                                              _rn(dtype), N, H, W, Cc, _st()), "rn_maxpool3x3s2_backward_bn")
        what = f"({N}, {H}, {W}) period {P}"
        _same(dx, want, "dx, " + what)
        s = _sums(part, rows, Cc)
        _same(s[0], want.sum(0), "sum g', " + what)
        _same(s[1], 2 * want.sum(0), "sum g' xhat, " + what)


# ------------------------------------------------------------------------------------------ 2. the finalizers against float64
NBLOCKS = [1, 2, 3, 4, 5, 127, 128, 129, 511, 512, 513]


def _ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def _synthetic_partials(nb, M, Cc, big, seed):
    "Plausible per-block (sum, sum of squares) of `M / nb` rows of N(mu_c, sigma_c) data, f32; `big`: block nb // 2 is 10^6 times larger."
    rng = np.random.default_rng(seed)
    mu, sigma = rng.normal(0.0, 1.0, Cc), rng.uniform(0.5, 1.5, Cc)
    r = M / nb
    s = r * (mu + sigma * rng.normal(0.0, 1.0, (nb, Cc)) / np.sqrt(r))
    q = r * (mu * mu + sigma * sigma) * (1.0 + 0.1 * rng.uniform(-1.0, 1.0, (nb, Cc)))
    if big:
        s[nb // 2] *= 1e6
        q[nb // 2] *= 1e6
    s[:, 0], q[:, 0] = r * 3.0, r * 1e-3    # column 0: mean 3 with q / M = 1e-3 -- the variance is negative before the clamp
    return np.stack([s, q], 1).astype(np.float32)                                     # [nb][2][C]


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("Cc", [8, 64, 2056])
def test_stats_finalizer_against_float64(Cc, big):
    """rn_bn_stats_finalize on synthetic partials, every nblocks around the 128-lane split and its 4-way unrolled loop; M = 1 takes
    the unbiased-variance branch.  The kernel sums in double, so: save_mean is the rounded double quotient (1 fp32 ulp for the
    summation order), invstd and the running variance 2 ulp; coef a is ONE fp32 product of the stored invstd (exact) and coef b one
    fp32 multiply-subtract of stored values (2 ulp of its larger term: half an ulp for the product, half an ulp of a result of up to twice
    that size; less when fused).  Momentum 0.25, so that (1 - momentum) and the products by the momentum are exact and the running
    statistics carry three roundings at most."""
    from pytorch_retinanet_amd._lib import check, lib
    eps, mom = np.float32(1e-5), np.float32(0.25)
    rng = np.random.default_rng(7)
    gamma, beta = rng.uniform(0.5, 1.5, Cc).astype(np.float32), rng.normal(0, 0.2, Cc).astype(np.float32)
    rm0, rv0 = rng.normal(0, 1, Cc).astype(np.float32), rng.uniform(0.5, 1.5, Cc).astype(np.float32)
    for nb in NBLOCKS:
        for M in ((1, 100003) if nb == 1 else (nb * 131 + 5,)):
            part = _synthetic_partials(nb, M, Cc, big, 100 + nb)
            t = lambda a: torch.from_numpy(a.copy()).to(DEV)
            p, g_, b_, rm, rv = t(part), t(gamma), t(beta), t(rm0), t(rv0)
            nbt = torch.tensor([41], dtype=torch.int64, device=DEV)
            out = torch.full((4 * Cc,), float("nan"), dtype=torch.float32, device=DEV)
            sp = out.data_ptr()
            check(lib.rn_bn_stats_finalize(p.data_ptr(), nb, M, Cc, g_.data_ptr(), b_.data_ptr(), rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(), float(mom),
                                           float(eps), sp, sp + 4 * Cc, sp + 8 * Cc, _st()), "rn_bn_stats_finalize")
            got = out.cpu().numpy().astype(np.float64)
            mean_g, inv_g, a_g, b_g = got[:Cc], got[Cc:2 * Cc], got[2 * Cc:3 * Cc], got[3 * Cc:]
            tot = part.astype(np.longdouble).sum(0)
            mean = (tot[0] / M).astype(np.float64)
            var_raw = (tot[1] / M - (tot[0] / M) ** 2).astype(np.float64)
            var = np.maximum(var_raw, 0.0)
            assert var_raw[0] < 0.0, "column 0 was meant to have a negative variance before the clamp"
            inv = 1.0 / np.sqrt(var + np.float64(eps))
            what = f"nblocks={nb} M={M} C={Cc} big={big}"
            assert int(nbt) == 42, what
            assert np.all(np.abs(mean_g - mean) <= _ulp32(mean)), "save_mean, " + what
            assert np.all(np.abs(inv_g - inv) <= 2 * _ulp32(inv)), "save_invstd, " + what
            assert np.array_equal(a_g.astype(np.float32), gamma * inv_g.astype(np.float32)), "coef a = gamma * invstd, " + what
            bb = beta.astype(np.float64) - mean_g * a_g
            assert np.all(np.abs(b_g - bb) <= 2 * _ulp32(np.maximum(np.abs(beta), np.abs(mean_g * a_g)))), "coef b, " + what
            unb = var * M / (M - 1) if M > 1 else var
            keep = 1.0 - np.float64(mom)
            for name, got_r, A, B in (("running_mean", rm, keep * rm0, np.float64(mom) * mean_g), ("running_var", rv, keep * rv0, np.float64(mom) * unb)):
                tol = 2 * _ulp32(np.maximum(np.maximum(np.abs(A), np.abs(B)), np.abs(A + B)))
                assert np.all(np.abs(got_r.cpu().numpy().astype(np.float64) - (A + B)) <= tol), f"{name}, {what}"


@pytest.mark.parametrize("training", [0, 1])
@pytest.mark.parametrize("Cc", [8, 64, 2056])
def test_bwd_finalizer_against_float64(Cc, training):
    """rn_bn_bwd_finalize on synthetic partials: dbeta = s, dgamma = q (rounded doubles: 1 ulp), a = gamma * invstd (one fp32 product:
    exact) and, training, the BatchNorm backward  dx = a (g - mean(g) - xhat mean(g xhat))  written  dx = a g + k1 x + k0:
    k1 = -a q / M * invstd, k0 = -a s / M + a q / M * mean * invstd, formed in double from the fp32 inputs (1 ulp; k0 is a
    difference, so + 1e-13 of its two terms for the double arithmetic).  Frozen statistics: k0 = k1 = 0."""
    from pytorch_retinanet_amd._lib import check, lib
    rng = np.random.default_rng(11)
    gamma = rng.uniform(0.5, 1.5, Cc).astype(np.float32)
    mean, inv = rng.normal(0, 1, Cc).astype(np.float32), rng.uniform(0.5, 2.0, Cc).astype(np.float32)
    for nb in NBLOCKS:
        M = nb * 131 + 5
        part = (rng.normal(0, 1, (nb, 2, Cc)) * 100).astype(np.float32)
        part[nb // 2] *= 1e6 if nb % 2 else 1.0
        t = lambda a: torch.from_numpy(a.copy()).to(DEV)
        p, g_, m_, i_ = t(part), t(gamma), t(mean), t(inv)
        out = torch.full((5 * Cc,), float("nan"), dtype=torch.float32, device=DEV)
        gp = out.data_ptr()
        check(lib.rn_bn_bwd_finalize(p.data_ptr(), nb, M, Cc, g_.data_ptr(), m_.data_ptr(), i_.data_ptr(), training, gp, gp + 4 * Cc, gp + 8 * Cc, _st()),
              "rn_bn_bwd_finalize")
        got = out.cpu().numpy().astype(np.float64)
        dgamma, dbeta, a_g, k0_g, k1_g = (got[i * Cc:(i + 1) * Cc] for i in range(5))
        tot = part.astype(np.longdouble).sum(0).astype(np.float64)
        s, q = tot[0], tot[1]
        what = f"nblocks={nb} M={M} C={Cc} training={training}"
        assert np.all(np.abs(dbeta - s) <= _ulp32(s)), "dbeta, " + what
        assert np.all(np.abs(dgamma - q) <= _ulp32(q)), "dgamma, " + what
        a = (gamma * inv).astype(np.float64)
        assert np.array_equal(a_g, a), "coef a, " + what
        if training:
            c1, c2 = -a * s / M, -a * q / M
            k1 = c2 * inv
            t2 = c2 * mean.astype(np.float64) * inv
            assert np.all(np.abs(k1_g - k1) <= _ulp32(k1)), "k1, " + what
            assert np.all(np.abs(k0_g - (c1 - t2)) <= _ulp32(c1 - t2) + 1e-13 * (np.abs(c1) + np.abs(t2))), "k0, " + what
        else:
            assert not k0_g.any() and not k1_g.any(), "frozen statistics: k0 = k1 = 0, " + what


# -------------------------------------------------------------------------- 3. the variance scheme when the mean dominates
FLOOR = 4 * 2.0 ** -23            # 4 fp32 ulp, relative
BLOCK = 128                       # rows per block of the restated scheme (one GEMM row tile)


def _draw(M, Cc, ratio, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    std = torch.rand(Cc, device=DEV, generator=g) + 0.5
    sign = torch.where(torch.arange(Cc, device=DEV) % 2 == 0, 1.0, -1.0)
    x = torch.randn((M, Cc), device=DEV, generator=g) * std + ratio * std * sign
    return x.to(dtype).contiguous()


def _block_sums32(v):
    "fp32 sums over contiguous blocks of BLOCK rows (sequential, like a thread's running sum), combined in float64."
    M = v.shape[0]
    tot = np.zeros(v.shape[1], np.float64)
    for r0 in range(0, M, BLOCK):
        tot += np.cumsum(v[r0:r0 + BLOCK], axis=0, dtype=np.float32)[-1].astype(np.float64)
    return tot


def _restated_scheme(x32, dy32, gamma32, eps, store):
    """The scheme as csrc/norm.hip documents it, written from that description: per-block fp32 sums of x and x^2 (and, backward,
    of g and g * xhat), one partial per block, combined in double per channel; var = q / M - mean^2; dx = a g + k1 x + k0 in fp32,
    stored in the activation's type (``store``)."""
    M = x32.shape[0]
    s, q = _block_sums32(x32), _block_sums32(x32 * x32)
    mean = s / M
    var = np.maximum(q / M - mean * mean, 0.0)
    inv = (1.0 / np.sqrt(var + eps)).astype(np.float32)
    unb = (var * M / (M - 1)).astype(np.float32)
    out = {"invstd": inv.astype(np.float64), "running_var": unb.astype(np.float64)}
    if dy32 is not None:
        mean32 = mean.astype(np.float32)
        xhat = (x32 - mean32) * inv
        sg, sq = _block_sums32(dy32), _block_sums32(dy32 * xhat)
        a = gamma32 * inv
        c1, c2 = -a.astype(np.float64) * sg / M, -a.astype(np.float64) * sq / M
        k1 = (c2 * inv).astype(np.float32)
        k0 = (c1 - c2 * mean32.astype(np.float64) * inv).astype(np.float32)
        dx = a * dy32 + (k1 * x32 + k0)
        out["dx"] = store(dx)
    return out


def _float64_truth(x64, dy64, gamma64, eps):
    M = x64.shape[0]
    mean = x64.mean(0)
    var = ((x64 - mean) ** 2).mean(0)
    inv = 1.0 / np.sqrt(var + eps)
    out = {"invstd": inv, "running_var": var * M / (M - 1)}
    if dy64 is not None:
        xhat = (x64 - mean) * inv
        out["dx"] = gamma64 * inv * (dy64 - dy64.mean(0) - xhat * (dy64 * xhat).mean(0))
    return out


def _errors(res, truth):
    e = {k: float(np.max(np.abs(res[k] - truth[k]) / np.abs(truth[k]))) for k in ("invstd", "running_var")}
    if "dx" in truth:
        e["dx"] = float(np.max(np.abs(res["dx"] - truth["dx"])) / np.max(np.abs(truth["dx"])))
    return e


def _torch_fp32(x, dy, gamma, eps):
    "torch's own batch norm on the fp32 copy of the same stored values (statistics, running variance at momentum 1, autograd dx)."
    Cc = x.shape[1]
    xf = x.float().view(1, -1, 1, Cc).permute(0, 3, 1, 2).requires_grad_(dy is not None)
    rm, rv = torch.zeros(Cc, device=DEV), torch.zeros(Cc, device=DEV)
    y, _, inv = torch.native_batch_norm(xf, gamma, torch.zeros_like(gamma), rm, rv, True, 1.0, eps)
    out = {"invstd": inv.double().cpu().numpy(), "running_var": rv.double().cpu().numpy()}
    if dy is not None:
        y.backward(dy.float().view(1, -1, 1, Cc).permute(0, 3, 1, 2))
        out["dx"] = xf.grad.permute(0, 2, 3, 1).reshape(-1, Cc).double().cpu().numpy()
    return out


def _judge(kernel, torch32, restated, what, assert_it):
    print(f"VARIANCE {what}: " + "; ".join(f"{k} kernel {kernel[k]:.3e} torch-fp32 {torch32[k]:.3e} restated {restated[k]:.3e}" for k in kernel))
    if assert_it:
        for k in kernel:
            bar = max(4 * max(torch32[k], restated[k]), FLOOR)
            assert kernel[k] <= bar, f"{what}: {k} error {kernel[k]:.3e} against float64 > {bar:.3e} (torch fp32 {torch32[k]:.3e}, restated scheme {restated[k]:.3e})"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M", [1031, 67601])
@pytest.mark.parametrize("ratio", [0, 4, 32])
def test_variance_scheme_fused_batchnorm_against_float64(ratio, M, dtype):
    """``FusedBatchNorm2d`` forward + backward at |mean| / std = ratio (signs mixed over the channels): relative error of invstd
    and of the running variance, max error of dx over max |dx|, all against float64 on the same stored values -- within 4 x the
    larger of two yardsticks measured on the same input (torch's fp32 batch norm; the numpy restatement of the documented
    scheme, dx rounded to the activation's type as the kernel stores it), floor 4 fp32 ulp.  The factor 4 covers another block
    split and summation order.  Measured figures: CHANGELOG.md."""
    from pytorch_retinanet_amd.norm import FusedBatchNorm2d
    Cc, eps = 64, 1e-5
    x, dy = _draw(M, Cc, ratio, dtype, 3), _draw(M, Cc, 0, dtype, 4)
    bn = FusedBatchNorm2d(Cc, eps=eps, momentum=1.0).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(Cc, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)) + 0.5)
    xin = x.view(1, M, 1, Cc).permute(0, 3, 1, 2).requires_grad_(True)
    assert bn._fusable(xin, None)
    y = bn(xin)
    stats = y.grad_fn.saved_tensors[3]                      # save_mean | save_invstd | coef a | coef b
    y.backward(dy.view(1, M, 1, Cc).permute(0, 3, 1, 2))
    kernel = {"invstd": stats[Cc:2 * Cc].double().cpu().numpy(), "running_var": bn.running_var.double().cpu().numpy(),
              "dx": xin.grad.permute(0, 2, 3, 1).reshape(M, Cc).double().cpu().numpy()}
    gamma = bn.weight.detach()
    x64, dy64, g64 = x.double().cpu().numpy(), dy.double().cpu().numpy(), gamma.double().cpu().numpy()
    truth = _float64_truth(x64, dy64, g64, eps)
    store = lambda a: torch.from_numpy(a).to(dtype).double().numpy()
    restated = _restated_scheme(x64.astype(np.float32), dy64.astype(np.float32), g64.astype(np.float32), eps, store)
    _judge(_errors(kernel, truth), _errors(_torch_fp32(x, dy, gamma, eps), truth), _errors(restated, truth),
           f"FusedBatchNorm2d ratio={ratio} M={M} {str(dtype)[6:]}", True)


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("M", [1031, 67601])
@pytest.mark.parametrize("ratio", [0, 4, 32])
def test_variance_scheme_gemm_epilogue_against_float64(ratio, M, dtype):
    """The same for ``pw_forward`` + statistics epilogue + ``bn_finalize``: identity weight, so the stored output IS the drawn tensor.
    Ratio 32 is measured and printed, not asserted: at (bf16, M = 67601) the kernel's invstd is 9.6e-6 / its running variance 1.9e-5
    from float64 against 5.4e-8 / 5.6e-8 for the restated scheme and 1.2e-7 / 2.7e-7 for torch -- cancellation alone (q / M is
    ~1000 x the variance, so one fp32 rounding of a partial is 6e-5 of it): bf16 values near 32 sigma are multiples of 1/8 .. 1/4, whose
    squares sum EXACTLY in fp32 over the restatement's 128-row blocks and no longer over the kernel's two row tiles per walker; the
    fp16 case of the same shape has the kernel at 1.6e-5 and the restatement at 1.9e-4 ("Variance when the mean dominates")."""
    from pytorch_retinanet_amd import pwconv
    Cc, eps = 64, 1e-5
    x = _draw(M, Cc, ratio, dtype, 5)
    w = torch.eye(Cc, device=DEV).to(dtype).view(Cc, Cc, 1, 1).contiguous(memory_format=torch.channels_last)
    epi, partial, nb = pwconv.stats_epilogue(M, Cc, torch.device(DEV))
    y = pwconv.pw_forward(_img(x, 1, 1, M), w, epi=epi)
    assert torch.equal(y.permute(0, 2, 3, 1).reshape(M, Cc), x)
    bn = torch.nn.BatchNorm2d(Cc, eps=eps, momentum=1.0).to(DEV)
    stats = pwconv.bn_finalize(partial, nb, M, bn)
    kernel = {"invstd": stats[Cc:2 * Cc].double().cpu().numpy(), "running_var": bn.running_var.double().cpu().numpy()}
    x64 = x.double().cpu().numpy()
    truth = _float64_truth(x64, None, None, eps)
    restated = _restated_scheme(x64.astype(np.float32), None, None, eps, None)
    _judge(_errors(kernel, truth), _errors(_torch_fp32(x, None, bn.weight.detach(), eps), truth), _errors(restated, truth),
           f"pw_forward + finalize ratio={ratio} M={M} {str(dtype)[6:]}", ratio != 32)
