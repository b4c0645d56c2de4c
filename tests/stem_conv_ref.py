"""Float64 references, schedule restatements and integer operands of the tests of csrc/stem.hip -- ``stem_fwd_kernel``
(``rn_stem_conv_forward``: the 7x7 / stride 2 / pad 3 stem convolution, 3 -> 64 channels, with bn1's statistics partials) and
``stem_wgrad_kernel`` + ``stem_wgrad_reduce_kernel`` (``rn_stem_conv_wgrad`` and, with the BatchNorm + ReLU backward in the operand
load, ``rn_stem_conv_wgrad_bn``) -- shared by ``test_stem_conv_ref.py`` (CPU: the references against torch's float64 convolution and its
weight gradient, the restatements by hand, the generators' promises) and ``test_stem_conv_exact_gpu.py``.

    y[b][yo][xo][n]  = sum over (r, px, c) of x[b][2 yo + r - 3][2 xo + px - 3][c] * w[n][r][px][c]          (zero outside the image)
    dW[n][r][px][c]  = sum over (b, yo, xo) of g[b][yo][xo][n] * x[b][2 yo + r - 3][2 xo + px - 3][c]

The references are numpy only: the 147 taps of a block of output rows gathered from a zero-bordered copy, one float64 matmul per block on
the VALUES of the operands -- no torch convolution, no MIOpen.  Float64 products and sums of small integers are exact in any order, so on
the integer operands below whatever separates a kernel from the reference is the kernel's.

Both kernels number their units of work row by row -- forward tile t = ((b Ho + yo) tiles_x + tx) of 16 output pixels, weight-gradient
stage s of 64 --, so a range of tiles or stages is a contiguous range of the flattened [B Ho Wo] output pixels; the restricted references
take (first, behind the last) tile or stage and work on that pixel range.  The schedule functions restate, from the host code of
csrc/stem.hip (``stem_grid``, ``stem_wgrad_grid``), which workgroup and wave owns which tiles and stages as functions of the shape and the
CU count alone; the GPU tests assert on them that a case reaches the depth it is here for.
"""
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

STEM_WAVES = 4          # waves of a workgroup; wave v of the forward takes tiles t_beg + v, + 4, ...
FWD_TILE = 16           # output pixels of a forward tile
WG_STAGE = 64           # output pixels of a weight-gradient stage
KROW = 32               # k elements of a kernel row in the workspace: k = 4 px + c, zeros at c = 3, neighbouring pixels at px = 7
COUT = 64
TAPS = 147              # 7 x 7 x 3
SLACK_PX = 160          # padded pixels behind the last image
H_LIMIT = 20000         # a case whose depth cannot be reached below this height fails


def out_hw(H: int, W: int) -> Tuple[int, int]:
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def padded_width(W: int) -> int:
    "Wpp: 3 border pixels to the left, at least 3 to the right, an even count."
    return (W + 7) & ~1


def padded_bytes(B: int, H: int, W: int) -> int:
    "rn_stem_padded_bytes: [B][H + 6][Wpp] pixels of 4 elements, two rows and 160 pixels of slack."
    return ((B * (H + 6) + 2) * padded_width(W) + SLACK_PX) * 8


# ---- float64 references ------------------------------------------------------------------------------------------------------------

def _taps_of_rows(x: np.ndarray, rid0: int, rid1: int) -> np.ndarray:
    "x [B][H][W][3] -> float64 [(rid1 - rid0) Wo][147]: the taps (r, px, c) of the output rows rid0 <= b Ho + yo < rid1, zero outside the image."
    B, H, W, C = x.shape
    Ho, Wo = out_hw(H, W)
    out = []
    rid = rid0
    while rid < rid1:
        b, y0 = divmod(rid, Ho)
        y1 = min(Ho, y0 + (rid1 - rid))
        n = y1 - y0
        xp = np.zeros((2 * n + 5, 2 * Wo + 5, C), np.float64)          # input rows 2 y0 - 3 .., columns -3 ..
        lo, hi = max(0, 2 * y0 - 3), min(H, 2 * y1 + 2)
        xp[lo - (2 * y0 - 3):hi - (2 * y0 - 3), 3:3 + W] = x[b, lo:hi]
        cols = np.empty((n, Wo, 7, 7, C), np.float64)
        for r in range(7):
            for px in range(7):
                cols[:, :, r, px] = xp[r:r + 2 * n - 1:2, px:px + 2 * Wo - 1:2]
        out.append(cols.reshape(n * Wo, 49 * C))
        rid += n
    return np.concatenate(out, 0) if len(out) != 1 else out[0]


def _taps_of_pixels(x: np.ndarray, m0: int, m1: int) -> np.ndarray:
    "... of the flattened output pixels m0 <= m < m1."
    _, Wo = out_hw(x.shape[1], x.shape[2])
    rid0 = m0 // Wo
    return _taps_of_rows(x, rid0, (m1 - 1) // Wo + 1)[m0 - rid0 * Wo:m1 - rid0 * Wo]


_BLOCK_ROWS = 256       # output rows gathered at a time: bounds the memory of a reference, changes no value


def _pixel_blocks(x: np.ndarray, m0: int, m1: int):
    _, Wo = out_hw(x.shape[1], x.shape[2])
    step = _BLOCK_ROWS * Wo
    for a in range(m0, m1, step):
        yield a, min(a + step, m1)


def tile_pixel_start(t: int, B: int, H: int, W: int, unit: int = FWD_TILE) -> int:
    "First flattened output pixel of forward tile t (``unit`` 16) or weight-gradient stage t (``unit`` 64); t = the total: behind the last."
    Ho, Wo = out_hw(H, W)
    tiles_x = (Wo + unit - 1) // unit
    rowid, tx = divmod(t, tiles_x)
    return min(rowid, B * Ho) * Wo + (tx * unit if rowid < B * Ho else 0)


def _pixel_range(x: np.ndarray, units: Optional[Tuple[int, int]], unit: int) -> Tuple[int, int]:
    B, H, W, _ = x.shape
    Ho, Wo = out_hw(H, W)
    if units is None:
        return 0, B * Ho * Wo
    return tile_pixel_start(units[0], B, H, W, unit), tile_pixel_start(units[1], B, H, W, unit)


def conv_ref(x: np.ndarray, w: np.ndarray, tiles: Optional[Tuple[int, int]] = None) -> np.ndarray:
    """float64 y from x [B][H][W][3] and w [64][7][7][3]: 7x7, stride 2, pad 3.  The whole output as [B][Ho][Wo][64]; with ``tiles`` =
    (t0, t1) the outputs of forward tiles t0 <= t < t1 alone, as [pixels][64] in the order of the flattened output."""
    B, H, W, _ = x.shape
    Ho, Wo = out_hw(H, W)
    wd = np.asarray(w, np.float64).reshape(w.shape[0], -1)
    m0, m1 = _pixel_range(x, tiles, FWD_TILE)
    y = np.empty((m1 - m0, wd.shape[0]), np.float64)
    for a, b in _pixel_blocks(x, m0, m1):
        y[a - m0:b - m0] = _taps_of_pixels(x, a, b) @ wd.T
    return y if tiles is not None else y.reshape(B, Ho, Wo, wd.shape[0])


def wgrad_ref(g: np.ndarray, x: np.ndarray, stages: Optional[Tuple[int, int]] = None) -> np.ndarray:
    """float64 dW [64][7][7][3] from g [B][Ho][Wo][64] and x [B][H][W][3]; ``stages`` = (s0, s1): only the output pixels of weight-gradient
    stages s0 <= s < s1 contribute."""
    Cout = g.shape[3]
    gd = np.asarray(g, np.float64).reshape(-1, Cout)
    m0, m1 = _pixel_range(x, stages, WG_STAGE)
    dw = np.zeros((Cout, 49 * x.shape[3]), np.float64)
    for a, b in _pixel_blocks(x, m0, m1):
        dw += gd[a:b].T @ _taps_of_pixels(x, a, b)
    return dw.reshape(Cout, 7, 7, x.shape[3])


def wgrad_ref_ranges(g: np.ndarray, x: np.ndarray, ranges: Sequence[Tuple[int, int]]) -> np.ndarray:
    "``wgrad_ref`` restricted to each (s0, s1) of ``ranges`` in turn: float64 [len(ranges)][64][7][7][3]."
    return np.stack([wgrad_ref(g, x, r) for r in ranges])


def abs_conv_ref(x: np.ndarray, w: np.ndarray, tiles: Optional[Tuple[int, int]] = None) -> np.ndarray:
    "sum over the taps of |x| |w| per output: what the rounding bound of a real-valued run is built from."
    return conv_ref(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)), tiles)


def abs_wgrad_ref(g: np.ndarray, x: np.ndarray, stages: Optional[Tuple[int, int]] = None) -> np.ndarray:
    return wgrad_ref(np.abs(np.asarray(g, np.float64)), np.abs(np.asarray(x, np.float64)), stages)


def round_to(a: np.ndarray, dtype: torch.dtype) -> np.ndarray:
    "Values (float32 or wider) -> the values ``dtype`` holds (round to nearest even), as float32."
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dtype).float().numpy()


def relu_alive(dtype: torch.dtype) -> float:
    "norm.hip's relu_alive_threshold: 2^-25 for fp16, the float of bit pattern 0x00004000 for bf16."
    bits = 0x33000000 if dtype == torch.float16 else 0x00004000
    return float(np.array([bits], np.uint32).view(np.float32)[0])


def bn_grad_ref(g: np.ndarray, z: np.ndarray, coef3: np.ndarray, fwd_coef: np.ndarray, dtype: torch.dtype) -> np.ndarray:
    """The conv-output gradient ``rn_stem_conv_wgrad_bn`` forms in its operand load (the comment of StemWgradArgs), as float32 values
    ``dtype`` holds: g [B][Ho][Wo][64] the gradient behind relu(bn1(.)), z the conv output, coef3 = [ba | bk0 | bk1], fwd_coef = [fa | fb]:

        g'  = g * [fma(z, fa, fb) > alive]
        out = round_dtype(fma(ba, g', fma(bk1, z, bk0)))

    Each fma is worked in float64 and rounded to float32 once -- exact on the integer operands of the tests.  Only real pixels exist
    here: what a stage holds past the end of an output row contributes ZERO to the weight gradient, not bk0."""
    c3, fc = np.asarray(coef3, np.float32).reshape(3, -1).astype(np.float64), np.asarray(fwd_coef, np.float32).reshape(2, -1).astype(np.float64)
    ba, bk0, bk1 = c3
    fa, fb = fc
    gd, zd = np.asarray(g, np.float64), np.asarray(z, np.float64)
    act = (zd * fa + fb).astype(np.float32)
    gp = np.where(act > np.float32(relu_alive(dtype)), gd, 0.0)
    inner = (bk1 * zd + bk0).astype(np.float32).astype(np.float64)
    return round_to((ba * gp + inner).astype(np.float32), dtype)


def sum_bound(K: int, abs_sum: np.ndarray) -> np.ndarray:
    "|fp32 sum - exact sum| <= (K - 1) 2^-24 sum |term| for K exact terms added in any order, one rounding per addition."
    return (K - 1) * 2.0 ** -24 * abs_sum


def half_ulp(ref: np.ndarray, bf16: bool) -> np.ndarray:
    "Half a unit in the last place of bf16 / fp16 at |ref| (float64)."
    p, emin = (7, -126) if bf16 else (10, -14)
    _, e = np.frexp(np.abs(ref))
    e = np.where(ref == 0, -2000, e)
    return np.ldexp(1.0, np.maximum(e - 1, emin) - p - 1)


# ---- the schedules: who owns which tiles and stages ------------------------------------------------------------------------------------

class FwdSchedule(NamedTuple):
    Ho: int
    Wo: int
    tiles_x: int                # tiles of 16 pixels per output row, the last one ragged
    total_tiles: int
    wgs: int
    tiles_per_wg: int           # a multiple of 4: every wave of the grid runs tiles_per_wg / 4 ring steps, rounded up to pairs


def fwd_schedule(B: int, H: int, W: int, cus: int) -> FwdSchedule:
    "``stem_grid``: at most 2 workgroups per CU and at least 4 tiles each; tiles per workgroup rounded up to the 4 waves."
    Ho, Wo = out_hw(H, W)
    tiles_x = (Wo + FWD_TILE - 1) // FWD_TILE
    T = B * Ho * tiles_x
    wgs = max(1, min(2 * cus, (T + STEM_WAVES - 1) // STEM_WAVES))
    tpw = (T + wgs - 1) // wgs
    tpw = (tpw + STEM_WAVES - 1) // STEM_WAVES * STEM_WAVES
    return FwdSchedule(Ho, Wo, tiles_x, T, (T + tpw - 1) // tpw, tpw)


def fwd_wg_tiles(wg: int, s: FwdSchedule) -> Tuple[int, int]:
    "(t_beg, t_end) of workgroup wg."
    return wg * s.tiles_per_wg, min((wg + 1) * s.tiles_per_wg, s.total_tiles)


def fwd_tiles_of(wg: int, wave: int, s: FwdSchedule) -> List[int]:
    "The tiles wave ``wave`` of workgroup ``wg`` computes, in its order: t_beg + wave, + 4, ... below t_end."
    t_beg, t_end = fwd_wg_tiles(wg, s)
    return list(range(t_beg + wave, t_end, STEM_WAVES))


def fwd_ring_steps(s: FwdSchedule) -> int:
    "(load, compute) steps every wave runs: n_iter * 2; the steps past a wave's last tile are masked."
    return (s.tiles_per_wg // STEM_WAVES + 1) // 2 * 2


def tile_coords(t: int, s: FwdSchedule) -> Tuple[int, int, int]:
    "(b, yo, tx) of tile t."
    rowid, tx = divmod(t, s.tiles_x)
    b, yo = divmod(rowid, s.Ho)
    return b, yo, tx


class WgradSchedule(NamedTuple):
    tiles_x: int                # stages of 64 pixels per output row
    total_stages: int
    wgs: int
    stages_per_wg: int


def wgrad_schedule(B: int, H: int, W: int, cus: int) -> WgradSchedule:
    "``stem_wgrad_grid``: at most 2 workgroups per CU, a contiguous range of stages each."
    Ho, Wo = out_hw(H, W)
    tiles_x = (Wo + WG_STAGE - 1) // WG_STAGE
    S = B * Ho * tiles_x
    wgs = max(1, min(2 * cus, S))
    spw = (S + wgs - 1) // wgs
    return WgradSchedule(tiles_x, S, (S + spw - 1) // spw, spw)


def wgrad_stages_of(wg: int, s: WgradSchedule) -> Tuple[int, int]:
    "(s_beg, s_end) of workgroup wg: stage k of it is staged in LDS buffer k & 1."
    return wg * s.stages_per_wg, min((wg + 1) * s.stages_per_wg, s.total_stages)


def workspace_bytes(s: WgradSchedule) -> int:
    return s.wgs * COUT * 7 * KROW * 4


# ---- integer operands ----------------------------------------------------------------------------------------------------------------

X_CAP = 2               # |x|, |g| and |z| of the integer operands
Y_CAP = 128             # |y| of the integer forward: sum |w| * X_CAP per output channel
MAX_TILES_PER_WG = 60   # 60 tiles x 16 pixels x 128^2 < 2^24: a workgroup's sum of squares is exact in fp32 in any order
DZ_CAP = 8              # |conv-output gradient| of the BatchNorm variant: |ba| X_CAP + |bk1| X_CAP + |bk0|


def stem_weights(seed: int = 0) -> np.ndarray:
    """w [64][7][7][3] float32 in {-1, 0, 1}: channel n holds a weight where (n + r + px + c) % 3 == 0 -- 49 of the 147 taps, 7 in every
    kernel row, all three input channels --, the sign drawn; every tap is set in 21 or 22 of the channels."""
    rng = np.random.default_rng(5100 + seed)
    n, r, px, c = np.meshgrid(np.arange(COUT), np.arange(7), np.arange(7), np.arange(3), indexing="ij")
    sign = rng.choice(np.array([-1.0, 1.0], np.float32), size=n.shape)
    return np.where((n + r + px + c) % 3 == 0, sign, np.float32(0)).astype(np.float32)


def forward_operands(B: int, H: int, W: int, seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    "(x [B][H][W][3] integers in [-2, 2], w of ``stem_weights``) as float32."
    rng = np.random.default_rng(4100 + seed)
    return rng.integers(-X_CAP, X_CAP + 1, size=(B, H, W, 3)).astype(np.float32), stem_weights(seed)


def _integers(a: np.ndarray, cap: float) -> bool:
    a = np.asarray(a, np.float64)
    return bool(np.array_equal(a, np.round(a))) and float(np.abs(a).max(initial=0.0)) <= cap


def exact_in_16_bits(a: np.ndarray) -> bool:
    "Integers of at most 8 significant bits (bf16) inside the fp16 range: exact in both element types."
    a = np.asarray(a, np.float64)
    if not _integers(a, 65504):
        return False
    m, _ = np.frexp(a)
    return bool(np.array_equal(m * 256, np.round(m * 256)))


def assert_forward_exact(x: np.ndarray, w: np.ndarray, tiles_per_wg: int) -> None:
    "What lets the GPU test ask for equality of the outputs and of every workgroup's statistics.  Conditions, never a clip."
    assert _integers(x, X_CAP)
    wd = np.asarray(w, np.float64)
    assert wd.shape == (COUT, 7, 7, 3) and bool(((wd == 0) | (np.abs(wd) == 1)).all())
    assert float(np.abs(wd).reshape(COUT, -1).sum(1).max()) * X_CAP <= Y_CAP          # every output an integer of at most 8 bits
    assert int((wd != 0).reshape(COUT, TAPS).sum(0).min()) >= 4, "a tap that fewer than four channels see"
    assert bool((wd != 0).reshape(COUT, 7, 21).any(2).all()), "a channel without a weight in some kernel row"
    assert tiles_per_wg <= MAX_TILES_PER_WG and tiles_per_wg * FWD_TILE * Y_CAP ** 2 < 2 ** 24


def wgrad_operands(B: int, H: int, W: int, seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    "(g [B][Ho][Wo][64], x [B][H][W][3]) float32: integers in [-2, 2]."
    rng = np.random.default_rng(6100 + seed)
    Ho, Wo = out_hw(H, W)
    return (rng.integers(-X_CAP, X_CAP + 1, size=(B, Ho, Wo, COUT)).astype(np.float32),
            rng.integers(-X_CAP, X_CAP + 1, size=(B, H, W, 3)).astype(np.float32))


def bn_operands(B: int, H: int, W: int, seed: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(z [B][Ho][Wo][64] integers in [-2, 2], coef3 [3][64] = ba | bk0 | bk1, fwd_coef [2][64] = fa | fb) float32: fa = 1 and fb = 0, so a
    pixel is alive where z > 0; ba in {1, 2, -1}, bk1 in {-1, 0, 1}, bk0 in {1, -1, 2, -2} -- never 0, so a masked pixel that went through
    the formula (z = 0, g = 0 -> bk0) changes the weight gradient by an integer."""
    rng = np.random.default_rng(6600 + seed)
    Ho, Wo = out_hw(H, W)
    z = rng.integers(-X_CAP, X_CAP + 1, size=(B, Ho, Wo, COUT)).astype(np.float32)
    n = np.arange(COUT)
    coef3 = np.stack([np.array([1, 2, -1])[n % 3], np.array([1, -1, 2, -2])[n % 4], np.array([-1, 0, 1])[(n // 2) % 3]]).astype(np.float32)
    fwd = np.stack([np.ones(COUT), np.zeros(COUT)]).astype(np.float32)
    return z, coef3, fwd


def assert_bn_exact(z: np.ndarray, coef3: np.ndarray, fwd_coef: np.ndarray, dz: np.ndarray) -> None:
    assert _integers(z, X_CAP) and bool((z > 0).any()) and bool((z < 0).any()) and bool((z == 0).any())
    assert _integers(coef3, 2) and bool((coef3[1] != 0).all()) and np.array_equal(fwd_coef[0], np.ones(COUT)) and not fwd_coef[1].any()
    assert _integers(dz, DZ_CAP) and exact_in_16_bits(dz)


def assert_wgrad_exact(g: np.ndarray, x: np.ndarray, total: np.ndarray, g_cap: int = X_CAP) -> None:
    """Integer operands; every partial sum of every workgroup and of the total is below 2^24 in magnitude (all pixels x the largest
    product bounds them all), so fp32 accumulation is exact in any order; the total inside the fp16 range."""
    assert _integers(g, g_cap) and _integers(x, X_CAP)
    pixels = g.size // g.shape[-1]
    assert pixels * g_cap * X_CAP < 2 ** 24, pixels
    assert _integers(total, 65504)


# ---- the cases: by the depth they are to reach, the height derived ---------------------------------------------------------------------

# image widths by the tiles of 16 output pixels they give: W 30 -> Wo 15, one ragged tile (an advance of 4 tiles wraps four rows);
# W 33 -> Wo 17 = 16 + 1; W 81 -> Wo 41 = 16 + 16 + 9; W 131 -> Wo 66 = 4 x 16 + 2, five tiles: coprime with the four waves
FWD_WIDTHS = {1: 30, 2: 33, 3: 81, 5: 131}


class Case(NamedTuple):
    name: str
    target: int                 # tiles_per_wg / stages_per_wg to reach
    W: int                      # the image width (weight gradient); the key of FWD_WIDTHS, tiles per output row (forward)
    B: int
    want: Tuple[str, ...]       # properties of the tail and of the image boundary the height is chosen for


def fwd_last_wg_tiles(s: FwdSchedule) -> int:
    return s.total_tiles - (s.wgs - 1) * s.tiles_per_wg


def fwd_boundary_inside_a_walk(B: int, s: FwdSchedule) -> bool:
    "Some wave owns tiles of two images."
    for b in range(1, B):
        wg = (b * s.Ho * s.tiles_x) // s.tiles_per_wg
        if any(len({tile_coords(t, s)[0] for t in fwd_tiles_of(wg, v, s)}) > 1 for v in range(STEM_WAVES)):
            return True
    return False


def _fwd_has(prop: str, B: int, s: FwdSchedule) -> bool:
    last = fwd_last_wg_tiles(s)
    if prop == "short_tail":            # a last workgroup with fewer tiles than waves
        return last < STEM_WAVES
    if prop == "uneven_tail":           # ... whose waves own different tile counts, none of them zero
        return last > STEM_WAVES and last % STEM_WAVES != 0
    if prop == "image_boundary":
        return fwd_boundary_inside_a_walk(B, s)
    raise KeyError(prop)


def forward_case(target_tiles_per_wg: int, tiles_x_kind: int, B: int, cus: int, want: Sequence[str] = ()) -> Tuple[int, int, int]:
    "(B, H, W): the smallest height at which ``stem_grid`` gives ``target_tiles_per_wg`` on ``cus`` CUs with the properties of ``want``."
    W = FWD_WIDTHS[tiles_x_kind]
    for H in range(1, H_LIMIT):
        s = fwd_schedule(B, H, W, cus)
        if s.tiles_per_wg == target_tiles_per_wg and all(_fwd_has(p, B, s) for p in want):
            return B, H, W
    raise AssertionError(f"tiles_per_wg {target_tiles_per_wg} with {tuple(want)} is out of reach below H = {H_LIMIT} at W {W}, B {B} on {cus} CUs")


def wgrad_boundary_inside_a_range(B: int, Ho: int, s: WgradSchedule) -> bool:
    return any((b * Ho * s.tiles_x) % s.stages_per_wg != 0 for b in range(1, B))


def wgrad_ranges_straddle_rows(s: WgradSchedule) -> bool:
    return any(a // s.tiles_x != (b - 1) // s.tiles_x for a, b in (wgrad_stages_of(wg, s) for wg in range(s.wgs)))


def _wgrad_has(prop: str, B: int, Ho: int, s: WgradSchedule) -> bool:
    if prop == "last_one":              # a last workgroup with one stage
        return s.total_stages - (s.wgs - 1) * s.stages_per_wg == 1
    if prop == "image_boundary":
        return wgrad_boundary_inside_a_range(B, Ho, s)
    if prop == "rows":
        return wgrad_ranges_straddle_rows(s)
    raise KeyError(prop)


def wgrad_case(target_stages_per_wg: int, W: int, B: int, cus: int, want: Sequence[str] = ()) -> Tuple[int, int, int]:
    "(B, H, W): the smallest height at which ``stem_wgrad_grid`` gives ``target_stages_per_wg`` on ``cus`` CUs with the properties of ``want``."
    for H in range(1, H_LIMIT):
        s = wgrad_schedule(B, H, W, cus)
        if s.stages_per_wg == target_stages_per_wg and all(_wgrad_has(p, B, out_hw(H, W)[0], s) for p in want):
            return B, H, W
    raise AssertionError(f"stages_per_wg {target_stages_per_wg} with {tuple(want)} is out of reach below H = {H_LIMIT} at W {W}, B {B} on {cus} CUs")


# forward: (target, tiles_x kind as W, B, want).  Depth 8: two tiles per wave, both ring slots computed; 12: three per wave, the last
# ring step masked for every wave; 20: five per wave, three passes of the ring
FCASES = [
    Case("t8_x1_b2_boundary_short", 8, 1, 2, ("image_boundary", "short_tail")),
    Case("t8_x2_uneven",            8, 2, 1, ("uneven_tail",)),
    Case("t12_x3_short",            12, 3, 1, ("short_tail",)),
    Case("t12_x5_b2_boundary",      12, 5, 2, ("image_boundary",)),
    Case("t20_x2_b2_boundary",      20, 2, 2, ("image_boundary",)),
    Case("t20_x1_uneven",           20, 1, 1, ("uneven_tail",)),
]

# weight gradient: (target, W, B, want).  W 66 -> Wo 33, one ragged stage per row; W 130 -> Wo 65 = 64 + 1; W 258 -> Wo 129 = 64 + 64 + 1
WCASES = [
    Case("s2_w258_last_one",        2, 258, 1, ("last_one", "rows")),
    Case("s3_w130_b2_boundary",     3, 130, 2, ("image_boundary", "rows")),
    Case("s3_w66",                  3, 66, 1, ()),
    Case("s5_w130_b2_last_one",     5, 130, 2, ("image_boundary", "last_one", "rows")),
]

REAL_FWD = Case("real_t12_x3", 12, 3, 1, ("uneven_tail",))
REAL_WGRAD = Case("real_s3_w130_b2", 3, 130, 2, ("image_boundary",))


def forward_shape(c: Case, cus: int) -> Tuple[int, int, int]:
    return forward_case(c.target, c.W, c.B, cus, c.want)


def wgrad_shape(c: Case, cus: int) -> Tuple[int, int, int]:
    return wgrad_case(c.target, c.W, c.B, cus, c.want)
