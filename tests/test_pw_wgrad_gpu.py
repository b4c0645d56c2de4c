"""GPU: ``pw_wgrad_kernel`` and the two split reductions of csrc/pw.hip against the float64 reference of ``pw_wgrad_ref.py``, at shapes
where a workgroup walks MORE THAN ONE 64-position K-tile (the register prefetch of tile kt + 1 under the MFMAs of tile kt, the second
pass through the staging, a last split with fewer tiles than the others) -- on all six (TN, TK) tiles, both grid forms, bf16 and fp16.

Integer operands: every product and every partial sum is an integer below 2^24, so fp32 accumulation is exact in any order and the
kernel must EQUAL the reference.  N(0, 1) operands: each element within the order-independent rounding bound of an fp32 sum.  The
reductions over the splits: bit for bit against their documented order restated with fp32 adds.

Every case first asserts, from the split count the library reports, that it still reaches the depth it exists for.
"""
import ctypes as C

import pytest
import torch

import pw_wgrad_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
GUARD = 4096            # bytes of pattern behind a buffer the kernels must not touch
PAD_ROWS = 130          # NaN rows behind G / z / X: two K-tiles' worth

# Factor on the summation bound of the real-valued cases.  (M - 1) 2^-24 sum |g x| holds for one rounding per addition; what the matrix
# unit's adder does inside an instruction is not documented.  1: the bound as derived -- measured on the MI355X, the largest err / bound
# over all real-valued cases is 5.1e-4 without a prologue (t128x128_m1050, fp16) and 4.4e-2 with one (bn2_2048x64, fp16, where the compiler
# may round multiply-add and conversion once and the restatement rounds twice); bf16 stays below 4e-4 everywhere.
BOUND_SCALE = 1.0


def _padded(t: torch.Tensor, fill) -> torch.Tensor:
    "``t`` as the leading slice of a larger allocation whose tail is ``fill``."
    buf = torch.empty((t.shape[0] + PAD_ROWS,) + tuple(t.shape[1:]), dtype=t.dtype, device=DEV)
    buf[t.shape[0]:] = fill
    buf[:t.shape[0]] = t.to(DEV)
    return buf[:t.shape[0]]


class _Problem:
    "One case on the device: operands inside NaN-tailed allocations, the descriptor and prologues of the C ABI, the float64 reference."

    def __init__(self, case, dtype, integer):
        from pytorch_retinanet_amd import pwconv
        from pytorch_retinanet_amd._lib import RN_BF16, RN_F16, RnPwConv
        op = R.operands(case, dtype, integer)
        self.case, self.dtype, geo = case, dtype, case.geo
        self.g, self.x = _padded(op.g, float("nan")), _padded(op.x, float("nan"))
        self.keep = [self.g, self.x]
        self.gpro = self.xpro = None
        dev = {}
        if case.gpro is not None:
            dev["z"], dev["coef3"] = _padded(op.z, float("nan")), op.coef3.to(DEV)
            dev["fwd"] = op.fwd.to(DEV) if op.fwd is not None else None
            dev["bits"] = _padded(op.bits, 0xFF) if op.bits is not None else None
            self.gpro = pwconv.bn_bwd(dev["coef3"], dev["z"], case.gpro, fwd_coef=dev["fwd"], bits=dev["bits"])
        if case.xpro:
            dev["xcoef"] = op.xcoef.to(DEV)
            self.xpro = pwconv.affine_relu(dev["xcoef"])
        self.keep.append(dev)
        self.d = RnPwConv(case.M, case.Cin, case.N, case.taps, case.stride, case.pad, geo.Ho, geo.Wo, geo.H, geo.W,
                          RN_F16 if dtype == torch.float16 else RN_BF16)
        gt = self.g.double() if case.gpro is None else R.pro_bn_bwd(self.g, dev["z"], dev["coef3"], case.gpro, dtype, dev["fwd"], dev["bits"])
        xt = R.pro_affine_relu(self.x, dev["xcoef"], dtype) if case.xpro else self.x.double()
        self.gt, self.xt = gt, xt
        self.ref = R.wgrad_ref(gt, xt, case.taps, case.stride, case.pad, geo)          # [N][taps][Cin] float64
        self.n_elems = case.N * case.taps * case.Cin

    def _ws(self):
        from pytorch_retinanet_amd._lib import lib
        need = int(lib.rn_pw_wgrad_workspace_bytes(C.byref(self.d)))
        assert need > 0 and need % 16 == 0
        return torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device=DEV), need       # f32 0xFFFFFFFF = NaN

    def _pro(self, p):
        return C.byref(p) if p is not None else None

    def partials(self):
        "rn_pw_conv_wgrad_partial into a NaN-patterned workspace of exactly the size the library asks for: (f32 [S][N][taps * Cin], launch)."
        from pytorch_retinanet_amd._lib import lib
        ws, need = self._ws()
        S = C.c_int(0)
        rc = lib.rn_pw_conv_wgrad_partial(C.byref(self.d), self.g.data_ptr(), self.x.data_ptr(), self._pro(self.gpro), self._pro(self.xpro),
                                          ws.data_ptr(), need, C.byref(S), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        S = int(S.value)
        assert 1 <= S and S * self.n_elems * 4 <= need
        assert bool((ws[need:] == 0xFF).all()), "the kernel wrote behind its workspace"
        return ws[:S * self.n_elems * 4].view(torch.float32).view(S, self.case.N, self.case.taps, self.case.Cin), R.launch_of(self.case, S)

    def full(self):
        "rn_pw_conv_wgrad: (dw [N][taps][Cin] in the element type, the workspace's f32 contents afterwards)."
        from pytorch_retinanet_amd._lib import lib
        ws, need = self._ws()
        out = torch.full((self.n_elems + GUARD // 2,), 0x7B7B, dtype=torch.int16, device=DEV)
        rc = lib.rn_pw_conv_wgrad(C.byref(self.d), self.g.data_ptr(), self.x.data_ptr(), out.data_ptr(), self._pro(self.gpro), self._pro(self.xpro),
                                  ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert bool((ws[need:] == 0xFF).all()), "the kernels wrote behind their workspace"
        assert bool((out[self.n_elems:] == 0x7B7B).all()), "the reduction wrote behind dW"
        return out[:self.n_elems].view(self.dtype).view(self.case.N, self.case.taps, self.case.Cin), ws[:need].view(torch.float32)


def _assert_depth(case, L):
    "Hard failure, not a skip: a change of wgrad_splits / wgrad_tile must not quietly turn these into single-tile tests."
    why = (f"{case.name}: the library now runs {L} -- the split heuristic or the tile choice changed and this shape no longer covers what it "
           f"is here for; choose a new shape in tests/pw_wgrad_ref.py (CASES)")
    assert L.KT >= case.depth, why
    assert L.tile == case.tile and L.xcd == case.xcd, why
    assert L.ragged != 0, why
    if case.s_mod8_zero is not None:
        assert (L.S % 8 == 0) == case.s_mod8_zero, why
    if case.short_last is not None:
        assert (L.last_tiles < L.KT) == case.short_last, why


def _reduce_ref(partial: torch.Tensor, dtype) -> torch.Tensor:
    """The order of pw_wgrad_reduce_kernel / pw_wgrad_reduce_many_kernel on partial f32 [S][n]: slice l = 0..7 adds splits l, l + 8, ...
    in sequence, starting from zero; the eight sums are added 0..7; one rounding to the element type."""
    S = partial.shape[0]
    sums = []
    for l in range(8):
        s = torch.zeros_like(partial[0])
        for sp in range(l, S, 8):
            s = s + partial[sp]
        sums.append(s)
    t = sums[0]
    for l in range(1, 8):
        t = t + sums[l]
    return t.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_integer_operands_give_the_exact_weight_gradient(case, dtype):
    p = _Problem(case, dtype, integer=True)
    assert R.operand_peak(case, p.gt, p.xt) < 2 ** 24 and torch.equal(p.ref, p.ref.round())
    part, L = p.partials()
    print(f"pw_wgrad {case.name} {dtype}: M {case.M} tile {L.tile} gy {L.gy} ktiles {L.ktiles} S {L.S} KT {L.KT} "
          f"{'XCD map' if L.xcd else '2-D grid'} last split {L.last_tiles} tiles, last tile {L.ragged} rows")
    _assert_depth(case, L)
    assert bool(torch.isfinite(part).all()), "a partial was left unwritten, or a row >= M / an invalid tap contributed"
    assert torch.equal(part, part.round()), "a partial of integer products is not an integer"
    got = part.double().sum(0)
    bad = got != p.ref
    assert not bool(bad.any()), (f"{int(bad.sum())} of {bad.numel()} elements differ, first at [n, tap, c] = {bad.nonzero()[0].tolist()}: "
                                 f"{float(got[bad][0])} != {float(p.ref[bad][0])}")
    dw, _ = p.full()
    want = p.ref.float().to(dtype)              # (the reference is an integer below 2^24: exact in fp32, then ONE rounding)
    assert torch.equal(dw, want), f"dW differs from the once-rounded reference in {int((dw != want).sum())} elements"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", [c for c in R.CASES if c.real], ids=lambda c: c.name)
def test_real_operands_stay_inside_the_summation_bound(case, dtype):
    p = _Problem(case, dtype, integer=False)
    part, L = p.partials()
    _assert_depth(case, L)
    assert bool(torch.isfinite(part).all())
    bound = R.sum_bound(case.M, R.abs_terms_sum(p.gt, p.xt, case.taps, case.stride, case.pad, case.geo))
    err = (part.double().sum(0) - p.ref).abs()
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"pw_wgrad {case.name} {dtype}: S {L.S} KT {L.KT} max err / bound = {ratio:.3e}")
    assert bool((err <= BOUND_SCALE * bound).all()), f"max err / bound = {ratio}"
    # rn_pw_conv_wgrad: the same partials (the kernel is deterministic), reduced in the documented order -- bit for bit -- which puts dW
    # within half a unit in the last place of the reference, plus the bound
    dw, ws = p.full()
    assert torch.equal(ws[:part.numel()].view_as(part), part)
    assert torch.equal(dw.view(-1), _reduce_ref(part.view(L.S, -1), dtype))
    derr = (dw.double() - p.ref).abs()
    assert bool((derr <= R.half_ulp(p.ref, dtype) + BOUND_SCALE * bound).all())


# ---- the reductions over the splits, alone ------------------------------------------------------------------------------------

def _reduce_many(problems, dtype, misalign=None, n_override=None):
    "problems: [(S, n_elems)] with random, non-integer partials.  Returns (status, partials, outputs with their guard behind them)."
    from pytorch_retinanet_amd._lib import RN_BF16, RN_F16, lib
    gen = torch.Generator(device=DEV).manual_seed(17)
    parts, outs = [], []
    for S, n in problems:
        parts.append(torch.randn((S, n), device=DEV, generator=gen) * 3.0)
        outs.append(torch.full((n + GUARD // 2,), 0x7B7B, dtype=torch.int16, device=DEV))
    k = len(problems)
    pp = [t.data_ptr() + (4 if misalign == "partial" else 0) for t in parts]
    po = [t.data_ptr() + (2 if misalign == "dw" else 0) for t in outs]
    rc = lib.rn_pw_wgrad_reduce_many_dt((C.c_void_p * k)(*pp), (C.c_int * k)(*[s for s, _ in problems]), (C.c_int64 * k)(*[n for _, n in problems]),
                                        (C.c_void_p * k)(*po), k if n_override is None else n_override, RN_F16 if dtype == torch.float16 else RN_BF16,
                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, parts, outs


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_reduce_many_eight_problems_of_very_different_sizes(dtype):
    """One launch: S of 1, 7, 8, 9, 17 and 64; n / 4 not a multiple of 32 (a block's last float4s idle); n > 2048 * 128 (the grid-stride
    loop runs twice in the first blocks) next to problems of one and two float4s, whose other 2047 blocks have nothing to do."""
    problems = [(1, 4), (7, 132), (8, 4 * 1000), (9, 2048 * 128 + 4 * 37), (17, 1028), (64, 5000), (3, 64 * 64), (2, 8)]
    rc, parts, outs = _reduce_many(problems, dtype)
    assert rc == 0
    for (S, n), part, out in zip(problems, parts, outs):
        assert bool((out[n:] == 0x7B7B).all()), (S, n)
        got, want = out[:n].view(dtype), _reduce_ref(part, dtype)
        assert torch.equal(got, want), f"S {S}, n {n}: {int((got != want).sum())} elements differ from the documented order"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("S,n", [(1, 36), (7, 4), (8, 132), (9, 64 * 64), (17, 2048 * 128 + 4), (64, 1028)])
def test_reduce_many_single_problem(S, n, dtype):
    rc, parts, outs = _reduce_many([(S, n)], dtype)
    assert rc == 0
    assert bool((outs[0][n:] == 0x7B7B).all())
    assert torch.equal(outs[0][:n].view(dtype), _reduce_ref(parts[0], dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_reduce_many_refusals_leave_the_outputs_alone(dtype):
    from pytorch_retinanet_amd._lib import lib
    RN_EINVAL, RN_EALIGN = -1, -2
    for what, want, kw, problems in (("nine problems", RN_EINVAL, {}, [(2, 64)] * 9),
                                     ("n_elems % 4 != 0", RN_EINVAL, {}, [(2, 64), (3, 66)]),
                                     ("partials not 16-byte aligned", RN_EALIGN, {"misalign": "partial"}, [(2, 64), (3, 128)]),
                                     ("dW not 8-byte aligned", RN_EALIGN, {"misalign": "dw"}, [(2, 64), (3, 128)]),
                                     ("no problems", RN_EINVAL, {"n_override": 0}, [(2, 64)])):
        rc, _, outs = _reduce_many(problems, dtype, **kw)
        assert rc == want, f"{what}: status {rc} ({lib.rn_status_string(rc)})"
        for out in outs:
            assert bool((out == 0x7B7B).all()), f"{what}: refused, but an output was written"
