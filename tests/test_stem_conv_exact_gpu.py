"""GPU: the stem kernels of csrc/stem.hip -- ``rn_stem_conv_forward`` (7x7 / stride 2 / pad 3 with bn1's statistics partials),
``rn_stem_conv_wgrad`` and ``rn_stem_conv_wgrad_bn`` -- against the float64 references of ``stem_conv_ref.py``, in bf16 and fp16, at the
depths where a wave walks several tiles and a workgroup several stages.

Integer operands: every product and every partial sum is an integer below 2^24 and every result one the element type holds, so fp32
accumulation is exact in any order and the kernels must EQUAL the reference -- the outputs, the statistics partials workgroup by workgroup,
the f32 weight-gradient workspace workgroup by workgroup, the weight gradient.  A tile computed from the other ring slot, a row wrap or an
image boundary missed by the walk, a stage read from the buffer being refilled or a masked pixel that picked up bk0 changes an integer.
N(0, 1) operands: each element within half a unit in the last place plus the order-independent summation bound.

Every buffer the kernels write is followed by a guard pattern that must come back untouched; the image, the gradient and the conv output
are the leading slices of allocations whose tails are NaN; the padded image and the packed weights start as NaNs.  The heights follow the
CU count: every case first asserts, as a hard failure, that the library's grids are the restated ones and that it reaches the depth it
is here for, and prints what it reached.
"""
import functools

import numpy as np
import pytest
import torch

import stem_conv_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "f16"]
GUARD = 4096            # bytes of pattern behind a buffer the kernels must not touch
PAD = 8192              # NaN elements behind an operand tensor

# Factor on the summation bound of the real-valued cases: (K - 1) 2^-24 sum |a b| holds for one rounding per addition in any order; what
# the matrix unit's adder does inside an instruction is not documented.  1: the bound as derived (test_dense_conv_exact_gpu.py and
# test_narrow_conv_gpu.py take the same).  Largest measured err / (half a unit in the last place + bound) per entry point on the MI355X
# (256 CUs), bf16 / fp16; nearly all of each figure is the rounding to the element type:
#   stem forward 0.994 / 0.962   stem weight gradient 4.6e-2 / 5.5e-3
# and of the f32 intermediates alone, err / bound: statistics partials sum z 1.8e-3 / 2.7e-3 and sum z^2 2.2e-2 / 2.6e-2 (at most 12 tiles
# each), weight-gradient partials (at most 3 stages each) 2.5e-2 / 2.9e-2.
BOUND_SCALE = 1.0


def _lib():
    from pytorch_retinanet_amd._lib import lib
    return lib


def _dt(dtype):
    from pytorch_retinanet_amd._lib import RN_BF16, RN_F16
    return RN_F16 if dtype == torch.float16 else RN_BF16


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _cus() -> int:
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _nan16(dtype) -> int:
    "The 16 bits of a quiet NaN of ``dtype``."
    return 0x7E00 if dtype == torch.float16 else 0x7FC0


def _operand(a: np.ndarray, dtype) -> torch.Tensor:
    "Values -> a flat device tensor of ``dtype``, the leading slice of an allocation whose tail is NaN."
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).reshape(-1).to(dtype)
    buf = torch.full((t.numel() + PAD,), float("nan"), dtype=dtype, device=DEV)
    buf[:t.numel()] = t.to(DEV)
    return buf[:t.numel()]


def _guarded(n: int, fill: int = 0x7B7B) -> torch.Tensor:
    "n 16-bit elements of ``fill`` to be written, then GUARD bytes of the same."
    return torch.full((n + GUARD // 2,), fill, dtype=torch.int16, device=DEV)


def _take(buf: torch.Tensor, n: int, dtype, what: str, fill: int = 0x7B7B) -> torch.Tensor:
    assert bool((buf[n:] == fill).all()), f"{what}: written behind its end"
    return buf[:n].view(dtype)


def _f32_guarded(n: int) -> torch.Tensor:
    "n floats of NaN pattern (0xFFFFFFFF) to be written, then GUARD bytes of the same."
    return torch.full((n * 4 + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)


def _take_f32(buf: torch.Tensor, n: int, what: str) -> torch.Tensor:
    assert bool((buf[n * 4:] == 0xFF).all()), f"{what}: written behind its end"
    return buf[:n * 4].view(torch.float32)


def _assert_equal(got: torch.Tensor, want: np.ndarray, what: str):
    g = got.float().cpu().numpy().reshape(want.shape)
    bad = ~(g == want)                                                  # (a NaN is a difference)
    if bad.any():
        idx = tuple(int(i[0]) for i in np.nonzero(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {idx}: {g[idx]} != {want[idx]}")


# ---- launches -------------------------------------------------------------------------------------------------------------------------

def _forward_launch(xd, wd, dtype, B, H, W, s: R.FwdSchedule, stats: bool = True):
    "rn_stem_conv_forward on device operands -> (z [pixels][64], partials [wgs][2][64] or None, the padded image for the weight gradient)."
    lib = _lib()
    need = int(lib.rn_stem_padded_bytes(B, H, W))
    assert need == R.padded_bytes(B, H, W), (need, R.padded_bytes(B, H, W))
    rows = int(lib.rn_stem_partial_rows(B, H, W))
    assert rows == s.wgs, f"rn_stem_partial_rows {rows}, the restated stem_grid {s.wgs}"
    nan = _nan16(dtype)
    xp, wk = _guarded(need // 2, nan), _guarded(R.COUT * 7 * R.KROW, nan)
    M = B * s.Ho * s.Wo
    z = _guarded(M * R.COUT)
    part = _f32_guarded(s.wgs * 2 * R.COUT)
    rc = lib.rn_stem_conv_forward(xd.data_ptr(), wd.data_ptr(), xp.data_ptr(), wk.data_ptr(), z.data_ptr(), part.data_ptr() if stats else 0, _dt(dtype),
                                  B, H, W, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    xpv, wkv = _take(xp, need // 2, dtype, "the padded image", nan), _take(wk, R.COUT * 7 * R.KROW, dtype, "the packed weights", nan)
    assert not bool(torch.isnan(xpv).any()) and not bool(torch.isnan(wkv).any()), "the padded image or the packed weights keep a NaN of the fill"
    zv = _take(z, M * R.COUT, dtype, "z").view(M, R.COUT)
    if not stats:
        assert bool((part == 0xFF).all()), "statistics written without a partial buffer"
        return zv, None, xpv
    return zv, _take_f32(part, s.wgs * 2 * R.COUT, "the statistics partials").view(s.wgs, 2, R.COUT), xpv


def _wgrad_launch(gd, xpv, dtype, B, H, W, q: R.WgradSchedule, bn=None):
    "rn_stem_conv_wgrad, or with bn = (z, coef3, fwd_coef) on the device rn_stem_conv_wgrad_bn -> (workspace [wgs][64][7][8][4] f32, dw [64][7][7][3])."
    lib = _lib()
    need = int(lib.rn_stem_wgrad_workspace_bytes(B, H, W))
    assert need == R.workspace_bytes(q), f"rn_stem_wgrad_workspace_bytes {need}, the restated stem_wgrad_grid {q.wgs} workgroups = {R.workspace_bytes(q)}"
    ws = _f32_guarded(need // 4)
    dw = _guarded(R.COUT * R.TAPS)
    if bn is None:
        rc = lib.rn_stem_conv_wgrad(gd.data_ptr(), xpv.data_ptr(), dw.data_ptr(), _dt(dtype), B, H, W, ws.data_ptr(), need, _stream())
    else:
        zd, c3, fc = bn
        rc = lib.rn_stem_conv_wgrad_bn(gd.data_ptr(), zd.data_ptr(), c3.data_ptr(), fc.data_ptr(), xpv.data_ptr(), dw.data_ptr(), _dt(dtype), B, H, W,
                                       ws.data_ptr(), need, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return (_take_f32(ws, need // 4, "the workspace").view(q.wgs, R.COUT, 7, 8, 4), _take(dw, R.COUT * R.TAPS, dtype, "dw").view(R.COUT, 7, 7, 3))


# ---- forward ----------------------------------------------------------------------------------------------------------------------------

def _fwd_path(c: R.Case, dtype, cus: int):
    "The shape of a forward case on this part; asserts the depth and the tail it is here for, and prints them."
    B, H, W = R.forward_shape(c, cus)
    s = R.fwd_schedule(B, H, W, cus)
    assert s.tiles_per_wg == c.target and s.tiles_x == c.W
    last = [len(R.fwd_tiles_of(s.wgs - 1, v, s)) for v in range(R.STEM_WAVES)]
    boundary = R.fwd_boundary_inside_a_walk(B, s)
    if "short_tail" in c.want:
        assert sum(last) < R.STEM_WAVES
    if "uneven_tail" in c.want:
        assert min(last) >= 1 and max(last) > min(last)
    if "image_boundary" in c.want:
        assert boundary
    print(f"stem forward {c.name} {dtype}: cus {cus} B {B} H {H} W {W} Ho {s.Ho} Wo {s.Wo} tiles_x {s.tiles_x} tiles {s.total_tiles} workgroups {s.wgs} "
          f"tiles_per_wg {s.tiles_per_wg} (tiles per wave {s.tiles_per_wg // 4}, ring steps {R.fwd_ring_steps(s)}) last workgroup's waves own {last} "
          f"image boundary inside a wave's walk {boundary}")
    return B, H, W, s


def _wg_pixel_starts(B, H, W, s: R.FwdSchedule) -> np.ndarray:
    return np.array([R.tile_pixel_start(wg * s.tiles_per_wg, B, H, W) for wg in range(s.wgs)])


@functools.lru_cache(maxsize=1)
def _forward_problem(name: str, cus: int):
    "Operands and references of an integer forward case, once for both element types (integers: float32 holds them all)."
    c = next(c for c in R.FCASES if c.name == name)
    B, H, W = R.forward_shape(c, cus)
    s = R.fwd_schedule(B, H, W, cus)
    x, w = R.forward_operands(B, H, W)
    R.assert_forward_exact(x, w, s.tiles_per_wg)
    y = R.conv_ref(x, w).reshape(-1, R.COUT)
    assert float(np.abs(y).max()) <= R.Y_CAP and R.exact_in_16_bits(y)
    starts = _wg_pixel_starts(B, H, W, s)
    part = np.stack([np.add.reduceat(y, starts, 0), np.add.reduceat(y * y, starts, 0)], 1)       # [wgs][sum y | sum y^2][64]
    assert float(part.max()) < 2 ** 24
    return x, w, y.astype(np.float32), part.astype(np.float32)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", [c.name for c in R.FCASES])
def test_integer_operands_give_the_exact_stem_forward_and_statistics(name, dtype):
    c = next(c for c in R.FCASES if c.name == name)
    B, H, W, s = _fwd_path(c, dtype, _cus())
    x, w, y, part = _forward_problem(name, _cus())
    xd, wd = _operand(x, dtype), _operand(w, dtype)
    z1, p1, _ = _forward_launch(xd, wd, dtype, B, H, W, s)
    _assert_equal(z1, y, "z [pixel][channel]")
    _assert_equal(p1, part, "partial[workgroup][sum z | sum z^2][channel]")
    z0, _, _ = _forward_launch(xd, wd, dtype, B, H, W, s, stats=False)
    assert torch.equal(z0, z1), "the launch without statistics stores another output"


# ---- weight gradient ----------------------------------------------------------------------------------------------------------------

def _wgrad_path(c: R.Case, what: str, dtype, cus: int):
    B, H, W = R.wgrad_shape(c, cus)
    q = R.wgrad_schedule(B, H, W, cus)
    Ho, Wo = R.out_hw(H, W)
    assert q.stages_per_wg == c.target
    last = R.wgrad_stages_of(q.wgs - 1, q)
    rows, boundary = R.wgrad_ranges_straddle_rows(q), R.wgrad_boundary_inside_a_range(B, Ho, q)
    if "last_one" in c.want:
        assert last[1] - last[0] == 1
    if "rows" in c.want:
        assert rows
    if "image_boundary" in c.want:
        assert boundary
    print(f"stem {what} {c.name} {dtype}: cus {cus} B {B} H {H} W {W} Ho {Ho} Wo {Wo} tiles_x {q.tiles_x} stages {q.total_stages} workgroups {q.wgs} "
          f"stages_per_wg {q.stages_per_wg} last workgroup {last[1] - last[0]} ranges straddle rows {rows} image boundary inside a range {boundary}")
    return B, H, W, q


def _ranges(q: R.WgradSchedule):
    return [R.wgrad_stages_of(wg, q) for wg in range(q.wgs)]


@functools.lru_cache(maxsize=1)
def _wgrad_problem(name: str, entry: str, cus: int):
    """Operands and references of an integer weight-gradient case.  entry "bn": g is the gradient behind relu(bn1(.)) and ``geff`` the
    conv-output gradient of bn_grad_ref -- the same integers in both element types; entry "plain": geff is g."""
    c = next(c for c in R.WCASES if c.name == name)
    B, H, W = R.wgrad_shape(c, cus)
    q = R.wgrad_schedule(B, H, W, cus)
    g, x = R.wgrad_operands(B, H, W)
    bn, geff, cap = None, g, R.X_CAP
    if entry == "bn":
        z, coef3, fwd = R.bn_operands(B, H, W)
        geff = R.bn_grad_ref(g, z, coef3, fwd, torch.bfloat16)
        assert np.array_equal(geff, R.bn_grad_ref(g, z, coef3, fwd, torch.float16))
        R.assert_bn_exact(z, coef3, fwd, geff)
        bn, cap = (z, coef3, fwd), R.DZ_CAP
    parts = R.wgrad_ref_ranges(geff, x, _ranges(q))
    total = R.wgrad_ref(geff, x)
    assert np.array_equal(parts.sum(0), total)
    R.assert_wgrad_exact(geff, x, total, cap)
    return g, x, bn, geff, parts.astype(np.float32), total


def _assert_workspace(ws: torch.Tensor, parts: np.ndarray, what: str):
    "ws [wgs][64][7][8][4]: the 21 real columns k = 4 px + c of every kernel row equal the reference, the c = 3 columns of px < 7 are zero."
    _assert_equal(ws[:, :, :, :7, :3], parts, f"{what}: workspace[workgroup][channel][r][px][c]")
    assert bool((ws[:, :, :, :7, 3] == 0).all()), f"{what}: a c = 3 column of the workspace is not zero"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("entry", ["plain", "bn"])
@pytest.mark.parametrize("name", [c.name for c in R.WCASES])
def test_integer_operands_give_the_exact_stem_weight_gradient_workgroup_by_workgroup(name, entry, dtype):
    c = next(c for c in R.WCASES if c.name == name)
    B, H, W, q = _wgrad_path(c, "wgrad" if entry == "plain" else "wgrad_bn", dtype, _cus())
    g, x, bn, geff, parts, total = _wgrad_problem(name, entry, _cus())
    s = R.fwd_schedule(B, H, W, _cus())
    _, _, xpv = _forward_launch(_operand(x, dtype), _operand(R.stem_weights(), dtype), dtype, B, H, W, s, stats=False)     # (the padded image)
    want_dw = R.round_to(total, dtype)
    ws, dw = _wgrad_launch(_operand(geff, dtype), xpv, dtype, B, H, W, q)
    _assert_workspace(ws, parts, "rn_stem_conv_wgrad")
    _assert_equal(dw, want_dw, "dw [channel][r][px][c] of rn_stem_conv_wgrad")
    if entry == "bn":
        z, coef3, fwd = bn
        dev = (_operand(z, dtype), torch.from_numpy(coef3).reshape(-1).to(DEV), torch.from_numpy(fwd).reshape(-1).to(DEV))
        ws_bn, dw_bn = _wgrad_launch(_operand(g, dtype), xpv, dtype, B, H, W, q, bn=dev)
        _assert_workspace(ws_bn, parts, "rn_stem_conv_wgrad_bn")
        _assert_equal(dw_bn, want_dw, "dw [channel][r][px][c] of rn_stem_conv_wgrad_bn")
        assert torch.equal(ws_bn, ws) and torch.equal(dw_bn, dw), "rn_stem_conv_wgrad_bn differs from rn_stem_conv_wgrad on the gradient of bn_grad_ref"


# ---- N(0, 1) operands: half a unit in the last place + the summation bound ------------------------------------------------------------

def _real(shape, dtype, seed: int, scale: float = 1.0) -> np.ndarray:
    "N(0, scale^2) values as ``dtype`` holds them."
    return R.round_to(np.random.default_rng(7100 + seed).standard_normal(shape, dtype=np.float32) * np.float32(scale), dtype)


def _within(got: torch.Tensor, ref: np.ndarray, bound: np.ndarray, dtype, what: str) -> float:
    "got (16-bit) against ref: |err| <= half an ulp of ref + BOUND_SCALE * bound, element by element; returns the largest ratio."
    err = np.abs(got.double().cpu().numpy().reshape(ref.shape) - ref)
    lim = R.half_ulp(ref, dtype == torch.bfloat16) + BOUND_SCALE * bound
    ratio = float((err / lim).max())
    print(f"{what} {dtype}: max err / (half ulp + bound) = {ratio:.3e}")
    assert bool((err <= lim).all()), f"{what}: max err / (half ulp + bound) = {ratio}"
    return ratio


def _f32_within(got: torch.Tensor, ref: np.ndarray, bound: np.ndarray, dtype, what: str) -> None:
    err = np.abs(got.double().cpu().numpy().reshape(ref.shape) - ref)
    ok = bound > 0
    ratio = float((err[ok] / bound[ok]).max()) if ok.any() else 0.0
    print(f"{what} {dtype}: max err / bound = {ratio:.3e} (f32)")
    assert bool((err <= BOUND_SCALE * bound).all()), f"{what}: max err / bound = {ratio}"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_real_operands_stem_forward_and_statistics_stay_inside_the_bound(dtype):
    c = R.REAL_FWD
    B, H, W, s = _fwd_path(c, dtype, _cus())
    assert s.tiles_per_wg // R.STEM_WAVES >= 3
    x, w = _real((B, H, W, 3), dtype, 1), _real((R.COUT, 7, 7, 3), dtype, 2, 0.1)
    z, part, _ = _forward_launch(_operand(x, dtype), _operand(w, dtype), dtype, B, H, W, s)
    _within(z, R.conv_ref(x, w).reshape(-1, R.COUT), R.sum_bound(R.TAPS, R.abs_conv_ref(x, w).reshape(-1, R.COUT)), dtype, "stem forward")
    # the partials: sums of the STORED values over the workgroup's own pixels (z^2 of a 16-bit value is exact in fp32): pixels - 1 additions
    stored = z.double().cpu().numpy()
    starts = _wg_pixel_starts(B, H, W, s)
    n = np.diff(np.append(starts, len(stored)))[:, None]
    _f32_within(part[:, 0], np.add.reduceat(stored, starts, 0), R.sum_bound(n, np.add.reduceat(np.abs(stored), starts, 0)), dtype, "stem forward sum z")
    _f32_within(part[:, 1], np.add.reduceat(stored ** 2, starts, 0), R.sum_bound(n, np.add.reduceat(stored ** 2, starts, 0)), dtype, "stem forward sum z^2")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_real_operands_stem_weight_gradient_stays_inside_the_bound(dtype):
    c = R.REAL_WGRAD
    B, H, W, q = _wgrad_path(c, "wgrad real", dtype, _cus())
    assert q.stages_per_wg >= 3
    Ho, Wo = R.out_hw(H, W)
    g, x = _real((B, Ho, Wo, R.COUT), dtype, 3), _real((B, H, W, 3), dtype, 4)
    s = R.fwd_schedule(B, H, W, _cus())
    _, _, xpv = _forward_launch(_operand(x, dtype), _operand(_real((R.COUT, 7, 7, 3), dtype, 5, 0.1), dtype), dtype, B, H, W, s, stats=False)
    ws, dw = _wgrad_launch(_operand(g, dtype), xpv, dtype, B, H, W, q)
    ranges = _ranges(q)
    pixels = np.array([R.tile_pixel_start(b, B, H, W, R.WG_STAGE) - R.tile_pixel_start(a, B, H, W, R.WG_STAGE) for a, b in ranges]).reshape(-1, 1, 1, 1, 1)
    _f32_within(ws[:, :, :, :7, :3], R.wgrad_ref_ranges(g, x, ranges), R.sum_bound(pixels, R.wgrad_ref_ranges(np.abs(g), np.abs(x), ranges)), dtype,
                "stem wgrad partials")
    assert bool((ws[:, :, :, :7, 3] == 0).all())
    _within(dw, R.wgrad_ref(g, x), R.sum_bound(B * Ho * Wo, R.abs_wgrad_ref(g, x)), dtype, "stem wgrad")
