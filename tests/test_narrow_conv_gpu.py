"""GPU: ``wgrad3x3_kernel`` + ``wgrad3x3_reduce_kernel`` (csrc/wgrad3x3.hip) and ``conv3x3_narrow64_kernel`` (csrc/narrow3x3.hip) against
the float64 references of ``narrow_conv_ref.py`` at shapes where their pipelines run past the prologue: a team that walks 2, 3, 4, 5 and
>= 8 tiles (the refill branch, both buffer parities, the steady state), ragged tails with idle teams, one- and two-k-step tiles in one
walk, walks across an image boundary; bands of 3, 4, 5, 6 and >= 9 rows (the four-row ring before, at and after its wrap), short last
bands, a single band, last strips of 1, 2, 9, 16, 17 and 48 pixels -- in bf16 and fp16.

Integer operands: every product and every partial sum is an integer below 2^24, so fp32 accumulation is exact in any order and the
kernels must EQUAL the reference -- the weight gradient workgroup by workgroup, each partial against the reference restricted to the
tiles the restated schedule gives that workgroup.  N(0, 1) operands: each element within the order-independent rounding bound.

The depth of both walks follows the CU count, so the shapes are derived at run time from what the library reports and every case first
asserts, as a hard failure, that it reaches what it is here for.
"""
import ctypes as C
import functools

import pytest
import torch

import narrow_conv_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
GUARD = 4096            # bytes of pattern behind a buffer the kernels must not touch
PAD_PIXELS = 200        # NaN pixels behind g / x: three tiles' worth

# Factor on the summation bound of the real-valued cases: (M - 1) 2^-24 sum |g x| holds for one rounding per addition in any order; what
# the matrix unit's adder does inside an instruction is not documented.  1: the bound as derived (test_pw_wgrad_gpu.py takes the same).
# Measured on the MI355X (256 CUs), the largest err / bound of the summed partials over all real-valued cases is 9.0e-4 (c512_d3_w70,
# fp16; bf16 8.9e-4) -- the cases with few pixels, where the bound is tightest; at 49 000-59 000 pixels it is 1e-6.  dW against half a unit
# in the last place + the bound: 0.95 at most (c512_d3_w70, bf16), nearly all of it the rounding to the element type.
BOUND_SCALE = 1.0


def _dt(dtype):
    from pytorch_retinanet_amd._lib import RN_BF16, RN_F16
    return RN_F16 if dtype == torch.float16 else RN_BF16


def _padded(t: torch.Tensor, fill, rows: int) -> torch.Tensor:
    "``t`` [rows_of_t][C] as the leading slice of a larger allocation whose tail is ``fill``."
    buf = torch.empty((t.shape[0] + rows,) + tuple(t.shape[1:]), dtype=t.dtype, device=DEV)
    buf[t.shape[0]:] = fill
    buf[:t.shape[0]] = t.to(DEV)
    return buf[:t.shape[0]]


def _wgs_per_sub(Cout: int, Cin: int) -> int:
    from pytorch_retinanet_amd._lib import lib
    subs = (Cout // 64) * (Cin // 64)
    need = int(lib.rn_conv3x3_wgrad_narrow_workspace_bytes(Cout, Cin))
    assert need > 0 and need % (subs * R.W3_OUT * 4) == 0
    return need // (subs * R.W3_OUT * 4)


class _Wgrad:
    "One weight-gradient case on the device: operands inside NaN-tailed allocations, the restated schedule, the float64 references."

    def __init__(self, case: R.WCase, dtype, integer: bool):
        self.case, self.dtype = case, dtype
        self.wps = _wgs_per_sub(case.Cout, case.Cin)
        self.N, self.H, self.W = R.wgrad_shape(case, self.wps)
        self.s = R.wgrad_schedule(self.N, self.H, self.W, case.Cout, case.Cin, self.wps)
        R.check_wgrad_case(case, self.s)
        g, x = R.wgrad_operands(self.N, self.H, self.W, case.Cout, case.Cin, dtype, integer)
        M = self.N * self.H * self.W
        self.M = M
        self.g = _padded(g.view(M, case.Cout), float("nan"), PAD_PIXELS).view(self.N, self.H, self.W, case.Cout)
        self.x = _padded(x.view(M, case.Cin), float("nan"), PAD_PIXELS).view(self.N, self.H, self.W, case.Cin)
        self.n_elems = case.Cout * 9 * case.Cin

    def run(self):
        """rn_conv3x3_wgrad_narrow into a NaN-patterned workspace of exactly the size the library asks for and a dW with a patterned tail:
        (partials f32 [workgroups][64][9][64], dw [Cout][9][Cin])."""
        from pytorch_retinanet_amd import biasact
        from pytorch_retinanet_amd._lib import lib
        c = self.case
        need = int(lib.rn_conv3x3_wgrad_narrow_workspace_bytes(c.Cout, c.Cin))
        ws = torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)                # f32 0xFFFFFFFF = NaN
        out = torch.full((self.n_elems + GUARD // 2,), 0x7B7B, dtype=torch.int16, device=DEV)
        zero = biasact._zero_page(torch.device(DEV))
        rc = lib.rn_conv3x3_wgrad_narrow(self.g.data_ptr(), self.x.data_ptr(), out.data_ptr(), _dt(self.dtype), self.N, self.H, self.W, c.Cout, c.Cin,
                                         zero.data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert bool((ws[need:] == 0xFF).all()), "the kernel wrote behind its workspace"
        assert bool((out[self.n_elems:] == 0x7B7B).all()), "the reduction wrote behind dW"
        assert bool((zero == 0).all()), "the zero page was written"
        part = ws[:need].view(torch.float32).view(self.s.subs * self.wps, 64, 9, 64)
        return part, out[:self.n_elems].view(self.dtype).view(c.Cout, 9, c.Cin)


def _first_difference(p: _Wgrad, got: torch.Tensor, want: torch.Tensor) -> str:
    bad = (got != want).flatten(1).any(1).nonzero().flatten().tolist()
    wg = bad[0]
    (b0, e0), (b1, e1) = p.s.ranges[wg]
    n, tap, c = (got[wg] != want[wg]).nonzero()[0].tolist()
    n0, c0 = p.s.block(wg)
    return (f"{len(bad)} of {got.shape[0]} workgroups differ from the reference over their own tiles (first ten: {bad[:10]}); workgroup {wg} "
            f"(block n0 {n0} c0 {c0}; team 0 tiles [{b0}, {e0}), team 1 tiles [{b1}, {e1}); tile = (image, row, x0, ksteps): "
            f"{[p.s.tile_map[t] for t in list(range(b0, e0))[:6]]} / {[p.s.tile_map[t] for t in list(range(b1, e1))[:6]]}): first at "
            f"(n, tap, c) = ({n}, {tap}, {c}): {float(got[wg, n, tap, c])} != {float(want[wg, n, tap, c])}; "
            f"{int((got[wg] != want[wg]).sum())} elements of this partial differ")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", R.WCASES, ids=lambda c: c.name)
def test_integer_operands_give_the_exact_weight_gradient_workgroup_by_workgroup(case, dtype):
    p = _Wgrad(case, dtype, integer=True)
    print(f"wgrad3x3 {case.name} {dtype}: N {p.N} H {p.H} W {p.W} wgs_per_sub {p.wps} {p.s.describe()}")
    want = R.wgrad_partials_ref(p.g, p.x, p.s)
    ref = R.total_from_partials(want, p.s, case.Cout, case.Cin)
    R.assert_wgrad_exactness(p.g, p.x, ref, R.abs_terms_sum(p.g, p.x))
    part, dw = p.run()
    assert not bool(torch.isnan(part).any()), f"{int(torch.isnan(part).flatten(1).any(1).sum())} workgroups left part of their partial unwritten"
    got = part.double()
    assert torch.equal(got, want), _first_difference(p, got, want)
    exact = ref.float().to(dtype)                # (an integer below 2^24: exact in fp32, then ONE rounding)
    assert torch.equal(dw, exact), f"dW differs from the once-rounded exact total in {int((dw != exact).sum())} elements"
    if case.wrapper:                             # the layout biasact hands to autograd: [Cout, Cin, 3, 3], channels-last = [Cout][3][3][Cin]
        from pytorch_retinanet_amd import biasact
        w = torch.empty((case.Cout, case.Cin, 3, 3), dtype=dtype, device=DEV).contiguous(memory_format=torch.channels_last)
        gl, xl = p.g.permute(0, 3, 1, 2), p.x.permute(0, 3, 1, 2)
        assert biasact.wgrad_narrow_ok(w, (1, 1), xl)
        dw2 = biasact.conv3x3_wgrad_narrow(gl, xl, w)
        assert dw2.shape == w.shape and dw2.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(dw2.permute(0, 2, 3, 1).reshape(case.Cout, 9, case.Cin), exact)
        assert torch.equal(dw2, exact.view(case.Cout, 3, 3, case.Cin).permute(0, 3, 1, 2))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", [c for c in R.WCASES if c.real], ids=lambda c: c.name)
def test_real_operands_stay_inside_the_summation_bound(case, dtype):
    p = _Wgrad(case, dtype, integer=False)
    assert p.s.tiles_per_team >= 3
    part, dw = p.run()
    assert bool(torch.isfinite(part).all())
    ref = R.wgrad_ref(p.g, p.x)
    bound = R.sum_bound(p.M, R.abs_terms_sum(p.g, p.x))
    total = R.total_from_partials(part.double(), p.s, case.Cout, case.Cin)
    err = (total - ref).abs()
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    derr = (dw.double() - ref).abs()
    dbound = R.half_ulp(ref, dtype) + BOUND_SCALE * bound
    print(f"wgrad3x3 {case.name} {dtype}: M {p.M} {p.s.describe()} max err / bound = {ratio:.3e} (partials), {float((derr / dbound).max()):.3e} (dW, with half an ulp)")
    assert bool((err <= BOUND_SCALE * bound).all()), f"max err / bound = {ratio}"
    # dW: the same partials reduced in the documented order, bit for bit -- within half a unit in the last place of the reference, plus the bound
    assert torch.equal(dw, R.reduce_ref(part, p.s, case.Cout, case.Cin, dtype))
    assert bool((derr <= dbound).all()), f"max dW err / (half ulp + bound) = {float((derr / dbound).max())}"


# ---- the forward product ---------------------------------------------------------------------------------------------------------

def _rows_per_band(N, H, W):
    from pytorch_retinanet_amd._lib import lib
    return int(lib.rn_conv3x3_narrow_rows_per_band(N, H, W))


@functools.lru_cache(maxsize=1)
def _forward_problem(name: str):
    "Shape, operands (fp32 integers on the device) and float64 references of a case, computed once for both element types."
    case = next(c for c in R.FCASES if c.name == name)
    N = R.forward_images(case, _rows_per_band)
    s = R.check_forward_case(case, N, _rows_per_band(N, case.H, case.W) if N else 0)
    x, w, bias = R.forward_operands(N, case.H, case.W, torch.float32)
    x, w, bias = x.to(DEV), w.to(DEV), bias.to(DEV)
    y = R.forward_ref(x, w)
    yb = R.forward_ref(x, w, bias)
    R.assert_forward_exactness(x, w, bias, y, yb)
    return case, N, s, x, w, bias, y, yb


def _forward(x, w, bias, relu, dtype):
    "rn_conv3x3_narrow_forward through the C ABI: x behind a NaN tail, y in front of a patterned one."
    from pytorch_retinanet_amd import biasact
    from pytorch_retinanet_amd._lib import lib
    N, H, W, _ = x.shape
    M = N * H * W
    xd = _padded(x.to(dtype).view(M, 64), float("nan"), PAD_PIXELS)
    out = torch.full((M * 64 + GUARD // 2,), 0x7B7B, dtype=torch.int16, device=DEV)
    wd = w.to(dtype).contiguous()
    rc = lib.rn_conv3x3_narrow_forward(xd.data_ptr(), wd.data_ptr(), bias.data_ptr() if bias is not None else None, out.data_ptr(), _dt(dtype), N, H, W, 64,
                                       int(relu), biasact._zero_page(torch.device(DEV)).data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((out[M * 64:] == 0x7B7B).all()), "the kernel wrote behind y"
    return out[:M * 64].view(dtype).view(N, H, W, 64)


def _assert_same(y: torch.Tensor, want: torch.Tensor, s: R.BandSchedule, what: str):
    bad = y.double() != want
    if bool(bad.any()):
        n, h, w_, c = bad.nonzero()[0].tolist()
        rows = sorted(set(bad.nonzero()[:, 1].tolist()))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outputs differ, in rows {rows[:20]} (bands of {s.rows_per_band} rows, {s.bands} per strip); first at "
                             f"(n, h, w, c) = ({n}, {h}, {w_}, {c}): row {h % s.rows_per_band} of band {h // s.rows_per_band}, pixel {w_ % 128} of strip {w_ // 128}: "
                             f"{float(y[n, h, w_, c])} != {float(want[n, h, w_, c])}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("name", [c.name for c in R.FCASES])
def test_integer_operands_give_the_exact_forward_product(name, dtype):
    case, N, s, x, w, bias, y, yb = _forward_problem(name)
    print(f"narrow3x3 {name} {dtype}: N {N} H {case.H} W {case.W} rows_per_band {s.rows_per_band} bands {s.bands} (last {s.last_band_rows} rows) "
          f"strips {s.strips} (last {s.last_strip_pixels} pixels) stores per wave {R.store_counts(case.W)}")
    _assert_same(_forward(x, w, None, False, dtype), y, s, "plain")
    _assert_same(_forward(x, w, bias, False, dtype), yb, s, "with bias")
    _assert_same(_forward(x, w, bias, True, dtype), torch.clamp(yb, min=0), s, "with bias and ReLU")
    if case.probe:
        # a different weight per output channel and per tap: a transposed or mirrored tap order cannot pass
        w2 = torch.zeros_like(w)
        w2[5, 0, 2, 9] = 1.0                                   # [co][kh][kw][ci]: y[:, h, w, 5] = x[:, h - 1, w + 1, 9]
        want = torch.zeros_like(y)
        want[:, 1:, :-1, 5] = x[:, :-1, 1:, 9].double()
        _assert_same(_forward(x, w2, None, False, dtype), want, s, "tap probe")
