"""GPU: ``pw_gemm_kernel`` (csrc/pw.hip, through ``rn_pw_conv_forward``) against the float64 reference of ``pw_gemm_ref.py`` at row counts
where a workgroup walks MORE THAN ONE 128-row tile: the one staging register set shared by a tile's later K-tiles and the next tile's
first, the f32 epilogue tile that overlays both LDS stages, the next tile's row decode under the current epilogue, the late epilogue
loads of the widest variant, the early return of the XCD-mapped grid and the column sums carried in registers across a walker's tiles --
1x1 and 3x3, stride 1 and 2, every prologue and epilogue and the pairs the fused bottleneck launches, bf16 and fp16.

Integer operands: every product, accumulator and partial sum is an integer below 2^24 (``test_pw_gemm_ref.py``), so fp32 arithmetic is
exact in any order and the kernel must EQUAL the once-rounded reference, element for element and partial row for partial row.
N(0, 1) operands: each element within the order-independent rounding bound of an fp32 sum plus half a unit of the output type.

Every case first asserts, from the walker count the library reports, that it still reaches the depth it exists for.
"""
import ctypes as C
import time

import pytest
import torch

import pw_gemm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
GUARD = 4096            # bytes of pattern behind Y and the partial sums that the kernel must not touch
PAD_ROWS = 130          # NaN rows (0xFF bits) behind every operand the kernel gathers by row: more than a row tile


def _padded(t: torch.Tensor, rows: int, fill) -> torch.Tensor:
    "``t`` (on the device, ``rows`` rows) as the leading part of a larger allocation whose PAD_ROWS further rows are ``fill``."
    buf = torch.empty((rows + PAD_ROWS, t.numel() // rows), dtype=t.dtype, device=DEV)
    buf[rows:] = fill
    buf[:rows] = t.view(rows, -1)
    return buf[:rows].view(t.shape)


def _assert_depth(case, wk, gx_lib):
    "Hard failure, not a skip: a changed work split must not quietly turn these into single-tile tests."
    why = (f"{case.name}: the library now runs M = {case.M} on {gx_lib} walkers -- the work split changed and this shape no longer covers what "
           f"it is here for; choose a new shape in tests/pw_gemm_ref.py (CASES, EXPECT_WALK)")
    assert gx_lib == wk.gx and (wk.MT, wk.rounds, wk.gx, wk.ragged) == R.EXPECT_WALK[case.M], why
    assert wk.depth == wk.rounds >= 2 and wk.ragged[1] >= 1, why
    assert case.KT == case.taps * case.Cin // 64 and case.ny == case.N // case.BN, why


class _Problem:
    "One case on the device: operands inside NaN-tailed allocations, the descriptors of the C ABI, guarded outputs, the float64 reference."

    def __init__(self, case, dtype, integer):
        from pytorch_retinanet_amd import pwconv
        from pytorch_retinanet_amd._lib import (RN_BF16, RN_F16, RN_PW_EPI_BIAS, RN_PW_EPI_RELU_BWD, RN_PW_EPI_RESID, RN_PW_EPI_STATS, RnPwConv,
                                                RnPwEpilogue, lib)
        self.case, self.dtype, geo = case, dtype, case.geo
        nan = float("nan")
        op = R.operands(case, dtype, integer, device=DEV)
        xr = geo.rows
        op = op._replace(x=_padded(op.x, xr, nan),
                         z=_padded(op.z, xr, nan) if op.z is not None else None,
                         xbits=_padded(op.xbits, xr, 0xFF) if op.xbits is not None else None,
                         R=_padded(op.R, op.R.shape[0], nan) if op.R is not None else None,
                         rbits=_padded(op.rbits, case.M, 0xFF) if op.rbits is not None else None,
                         zp=_padded(op.zp, case.M, nan) if op.zp is not None else None)
        self.op = op
        self.wk = R.walk(case.M)
        _assert_depth(case, self.wk, int(lib.rn_pw_walkers(case.M)))
        self.d = RnPwConv(case.M, case.Cin, case.N, case.taps, case.stride, case.pad, geo.Ho, geo.Wo, geo.H, geo.W,
                          RN_F16 if dtype == torch.float16 else RN_BF16)
        self.pro = None
        if case.pro == "aff":
            self.pro = pwconv.affine_relu(op.xcoef)
        elif case.pro is not None:
            self.pro = pwconv.bn_bwd(op.coef3, op.z, case.pro, fwd_coef=op.fwd, bits=op.xbits)
        self.y = torch.full((case.M * case.N + GUARD // 2,), 0x7B7B, dtype=torch.int16, device=DEV)
        self.partial = None
        self.n_partial = self.wk.gx * 2 * case.N                    # exactly the rows the library's walker count asks for
        if case.epi in ("stats", "relu_bwd"):
            self.partial = torch.full((self.n_partial * 4 + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)      # f32 0xFFFFFFFF = NaN
        pp = self.partial.data_ptr() if self.partial is not None else 0
        N = case.N
        if case.epi == "":
            self.epi = None
        elif case.epi == "stats":
            self.epi = RnPwEpilogue(RN_PW_EPI_STATS, pp, 0, 0, 0, 0, 0, 0, 0)
        elif case.epi in ("resid", "resid_bits"):
            self.epi = RnPwEpilogue(RN_PW_EPI_RESID, 0, op.R.data_ptr(), op.rbits.data_ptr() if op.rbits is not None else 0, 0, 0, 0, 0, 0)
        elif case.epi == "resid_s2":
            self.epi = RnPwEpilogue(RN_PW_EPI_RESID, 0, op.R.data_ptr(), 0, 0, 0, 0, 0, 0, 2, *case.res_hw)
        elif case.epi == "relu_bwd":
            p = op.est.data_ptr()                                   # emean | einv | ea | eb
            self.epi = RnPwEpilogue(RN_PW_EPI_RELU_BWD, pp, 0, 0, op.zp.data_ptr(), p + 8 * N, p + 12 * N, p, p + 4 * N)
        elif case.epi in ("bias", "bias_resid_relu"):
            self.epi = pwconv.bias_act_epilogue(op.bias, case.epi == "bias_resid_relu", op.R)
            assert self.epi.kind == RN_PW_EPI_BIAS | (RN_PW_EPI_RESID if op.R is not None else 0)
        else:
            raise AssertionError(case.epi)
        self.ex = R.expected(case, op, dtype)

    def run(self):
        "(Y as float64 [M][N], the partial sums as float64 [gx][2][N] or None), after checking the guards behind both."
        from pytorch_retinanet_amd._lib import lib
        case = self.case
        rc = lib.rn_pw_conv_forward(C.byref(self.d), self.op.x.data_ptr(), self.op.w.data_ptr(), self.y.data_ptr(),
                                    C.byref(self.pro) if self.pro is not None else None, C.byref(self.epi) if self.epi is not None else None,
                                    torch.cuda.current_stream().cuda_stream)
        assert rc == 0, (rc, lib.rn_status_string(rc))
        torch.cuda.synchronize()
        n = case.M * case.N
        assert bool((self.y[n:] == 0x7B7B).all()), "the kernel wrote behind Y"
        part = None
        if self.partial is not None:
            assert bool((self.partial[self.n_partial * 4:] == 0xFF).all()), "the kernel wrote behind its gx partial rows"
            part = self.partial[:self.n_partial * 4].view(torch.float32).view(self.wk.gx, 2, case.N).double()
        return self.y[:n].view(self.dtype).view(case.M, case.N).double(), part


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_integer_operands_give_the_exact_output(case, dtype):
    t0 = time.perf_counter()
    p = _Problem(case, dtype, integer=True)
    ex, wk = p.ex, p.wk
    assert torch.equal(ex.acc, ex.acc.round()) and float(ex.acc.abs().max()) < 2 ** 24 and (ex.keep is None or bool(ex.keep.all()))
    got, part = p.run()
    print(f"pw_gemm {case.name} {dtype}: M {case.M} = {wk.MT} tiles on {wk.gx} walkers ({wk.rounds} rounds), KT {case.KT}, BN {case.BN} x {case.ny} "
          f"({'XCD map' if case.ny >= 2 else '2-D grid'}), last tile: walker {wk.ragged[0]}'s tile {wk.ragged[1]} with {wk.ragged[2]} rows")
    assert bool(torch.isfinite(got).all()), "a row >= M, an invalid tap or an operand's NaN tail reached the output"
    bad = got != ex.y
    if bool(bad.any()):
        m, n = bad.nonzero()[0].tolist()
        tiles = sorted(set((bad.any(1).nonzero().view(-1) // 128).tolist()))
        raise AssertionError(f"{int(bad.sum())} of {bad.numel()} elements differ from the once-rounded reference, first at [m, n] = [{m}, {n}]: "
                             f"{float(got[m, n])} != {float(ex.y[m, n])}; row tiles {tiles[:8]}{'...' if len(tiles) > 8 else ''} "
                             f"(tiles >= {wk.gx} are later tiles of their walkers)")
    terms = R.partial_terms(case, ex, ex.y)
    if terms is not None:
        assert bool(torch.isfinite(part).all()), "a walker's partial row was left unwritten"
        for which, t in enumerate(terms):
            want = R.walker_sums(t, wk)
            bad = part[:, which] != want
            assert not bool(bad.any()), (f"partial sum {which}: {int(bad.sum())} of {bad.numel()} entries differ from the sums over each walker's own "
                                         f"tiles, first at [walker, n] = {bad.nonzero()[0].tolist()}")
    torch.cuda.synchronize()
    print(f"pw_gemm {case.name} {dtype}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", [c for c in R.CASES if c.real], ids=lambda c: c.name)
def test_real_operands_stay_inside_the_summation_bound(case, dtype):
    """|got - ref64| <= (T - 1) 2^-24 sum |terms| + half_ulp(|ref64| + that bound): T = K products (taps * Cin) plus the epilogue's addends
    (bias, residual: each one more fp32 addition of one more term).  The bound is derived, not fitted: one rounding per addition in any
    order, one rounding to the element type."""
    p = _Problem(case, dtype, integer=False)
    ex, wk = p.ex, p.wk
    got, part = p.run()
    assert bool(torch.isfinite(got).all())
    xt = R.transformed(case, p.op, dtype)
    mag = R.abs_terms(xt, p.op.w, case.taps, case.stride, case.pad, case.geo)
    if ex.extra_abs is not None:
        mag = mag + ex.extra_abs
    bound = R.sum_bound(case.taps * case.Cin + ex.extra_terms, mag)
    tol = bound + R.half_ulp(ex.pre.abs() + bound, dtype)
    if case.epi == "relu_bwd":
        left_out = float(ex.keep.logical_not().double().mean())
        assert left_out <= 1e-4, left_out
        dead = ex.keep & ~ex.alive
        assert float(got[dead].abs().max()) == 0.0, "an element whose ReLU was shut is not zero"
        sel = ex.keep & ex.alive
        err, tol = (got - ex.pre)[sel].abs(), tol[sel]
    else:
        err = (got - ex.pre).abs()
    ratio = float((err / tol).max())
    print(f"pw_gemm {case.name} {dtype}: {wk.rounds} rounds KT {case.KT} max err / bound = {ratio:.3e}")
    assert bool((err <= tol).all()), f"max err / bound = {ratio}"
    # the column sums: float64 sums of the STORED output over each walker's own rows, within the bound of an fp32 sum of that many terms
    terms = R.partial_terms(case, ex, got)
    if terms is not None:
        assert bool(torch.isfinite(part).all())
        rows = torch.tensor(R.walker_rows(wk), dtype=torch.float64, device=DEV)[:, None]
        for which, t in enumerate(terms):
            serr = (part[:, which] - R.walker_sums(t, wk)).abs()
            sbound = (rows - 1) * 2.0 ** -24 * R.walker_sums(t.abs(), wk)                 # R.sum_bound with each walker's own row count
            sratio = float((serr[sbound > 0] / sbound[sbound > 0]).max())
            print(f"pw_gemm {case.name} {dtype}: partial sum {which} max err / bound = {sratio:.3e}")
            assert bool((serr <= sbound).all()), f"partial sum {which}: max err / bound = {sratio}"
