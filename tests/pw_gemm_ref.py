"""Float64 reference of ``pw_gemm_kernel`` (csrc/pw.hip) -- the forward and data-gradient GEMM of the trunk and FPN convolutions -- and
the shapes its tests run, shared by ``test_pw_gemm_ref.py`` (CPU: the reference against torch's float64 convolution, the epilogue
restatements, the work split, the operand generator's promises) and ``test_pw_gemm_gpu.py``.

    Y[m][n] = epi( sum_{tap, c}  X'[pos(m, tap)][c] * W[n][tap][c] )          X' = pro(X), rounded to the 16-bit type

``gemm_ref`` is index arithmetic and one float64 matmul per tap -- no torch convolution -- on the 16-bit operand VALUES.  The gather
(``tap_rows``), the prologues (``pro_bn_bwd``, ``pro_affine_relu``), the ReLU bits and the rounding bounds are those of
``pw_wgrad_ref.py``; this module adds the epilogues and the work split.

The kernel's workgroups are persistent row-tile walkers: ``walk(M)`` restates ``walkers()`` -- one walker per 128-row tile up to 512
tiles, above that ``rounds = ceil(MT / 512)`` tiles per walker with stride ``gx``.  The shapes (``CASES``) are the smallest that give a
walker two or more row tiles: the staging registers shared between a tile's later K-tiles and the next tile's first one, the f32 tile
that overlays the two LDS stages, the row decode of the next tile under the current epilogue, and the column sums carried across a
walker's tiles run only there.  ``EXPECT_WALK`` is ``walkers()`` worked through and is documentation -- the GPU test reads the walker
count from the library and fails if a case no longer reaches the depth it claims.

The operands come from a counter-based integer hash evaluated with int64 tensor arithmetic that never overflows, so the CPU test sees
the very integers the GPU test generates on the device.
"""
import math
import zlib
from typing import List, NamedTuple, Optional, Tuple

import torch

from pw_wgrad_ref import (ALIVE, Geometry, _fma32, geometry, half_ulp, pack_bits, pro_affine_relu, pro_bn_bwd, sum_bound, tap_rows,
                          unpack_bits)

__all__ = ["ALIVE", "Geometry", "geometry", "half_ulp", "pack_bits", "unpack_bits", "sum_bound", "tap_rows", "pro_bn_bwd", "pro_affine_relu"]

BM, BK, MAX_GX = 128, 64, 512           # csrc/pw.hip: PW_BM, PW_BK, PW_MAX_GX


# ---- the contraction ---------------------------------------------------------------------------------------------------------

def gemm_ref(xt: torch.Tensor, w: torch.Tensor, taps: int, stride: int, pad: int, geo: Geometry) -> torch.Tensor:
    """float64 [M][N] from the TRANSFORMED activation xt [nimg * H * W][Cin] and w [N][taps][Cin] (any float type: the values are taken
    as they are).  A tap outside the image contributes 0 -- the padding applies to X', not to X."""
    assert xt.shape[0] == geo.rows and w.shape[1] == taps and w.shape[2] == xt.shape[1], (tuple(xt.shape), tuple(w.shape), geo)
    xd, wd = xt.double(), w.double()
    rows, ok = tap_rows(geo, taps, stride, pad, xd.device)
    out = torch.zeros((geo.M, wd.shape[0]), dtype=torch.float64, device=xd.device)
    zero = torch.zeros((), dtype=torch.float64, device=xd.device)
    for tap in range(taps):
        out += torch.where(ok[tap][:, None], xd[rows[tap]], zero) @ wd[:, tap, :].t()
    return out


def abs_terms(xt: torch.Tensor, w: torch.Tensor, taps: int, stride: int, pad: int, geo: Geometry) -> torch.Tensor:
    "sum_{tap, c} |X'[pos(m, tap)][c] * W[n][tap][c]| with the reference's own gather."
    return gemm_ref(xt.double().abs(), w.double().abs(), taps, stride, pad, geo)


# ---- the work split (csrc/pw.hip: walkers(), the loop ``for (mt = walker; mt < MT; mt += gx)``) ---------------------------------

class Walk(NamedTuple):
    M: int
    MT: int             # 128-row tiles
    rounds: int         # ceil(MT / 512): what walkers() divides by
    gx: int             # walkers = rows of the partial sums

    def tiles(self, walker: int) -> List[int]:
        return list(range(walker, self.MT, self.gx))

    @property
    def depth(self) -> int:
        "row tiles of the busiest walker"
        return len(self.tiles(0))

    @property
    def ragged(self) -> Tuple[int, int, int]:
        "(walker, position among that walker's tiles, rows) of the last row tile"
        return (self.MT - 1) % self.gx, (self.MT - 1) // self.gx, self.M - (self.MT - 1) * BM


def walk(M: int) -> Walk:
    MT = (M + BM - 1) // BM
    if MT <= MAX_GX:
        return Walk(M, MT, 1, MT)
    rounds = (MT + MAX_GX - 1) // MAX_GX
    return Walk(M, MT, rounds, (MT + rounds - 1) // rounds)


def walker_sums(t: torch.Tensor, wk: Walk) -> torch.Tensor:
    "float64 [gx][N]: the sum of t [M][N] over the rows of each walker's tiles (tile r * gx + w is walker w's r-th)."
    M, N = t.shape
    assert M == wk.M
    full = torch.zeros((wk.depth * wk.gx * BM, N), dtype=torch.float64, device=t.device)
    full[:M] = t
    return full.view(wk.depth, wk.gx, BM, N).sum((0, 2))


def walker_rows(wk: Walk) -> List[int]:
    "rows each walker sums over"
    return [sum(min(BM, wk.M - t * BM) for t in wk.tiles(w)) for w in range(wk.gx)]


# ---- the epilogues -----------------------------------------------------------------------------------------------------------------

def _round_to(v64: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    "One rounding of a float64 value to ``dtype``, returned as float64.  (Through fp32: exact for the integers below 2^24 the equality tests use.)"
    return v64.float().to(dtype).double()


def resid_term(R: torch.Tensor, rbits: Optional[torch.Tensor], res_stride: int, M: int, rH: int = 0, rW: int = 0) -> torch.Tensor:
    """EPI_RESID's addend, float64 [M][N].  res_stride 1: R [M][N], times its ReLU bits where given.  res_stride 2: R lives on the
    [nimg][ceil(rH / 2)][ceil(rW / 2)] grid of the output grid [nimg][rH][rW]; rows with even (y, x) take R[n][y / 2][x / 2], all others nothing."""
    N = R.shape[1]
    if res_stride != 2:
        assert R.shape[0] == M
        r = R.double()
        return r * unpack_bits(rbits, M, N) if rbits is not None else r
    assert rbits is None and M % (rH * rW) == 0
    m = torch.arange(M, device=R.device, dtype=torch.int64)
    n, rem = m // (rH * rW), m % (rH * rW)
    y, x = rem // rW, rem % rW
    h2, w2 = (rH + 1) // 2, (rW + 1) // 2
    assert R.shape[0] == (M // (rH * rW)) * h2 * w2
    on = (y % 2 == 0) & (x % 2 == 0)
    src = torch.where(on, (n * h2 + y // 2) * w2 + x // 2, torch.zeros_like(m))
    return torch.where(on[:, None], R.double()[src], torch.zeros((), dtype=torch.float64, device=R.device))


def epi_store(acc: torch.Tensor, dtype: torch.dtype, bias: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None,
              relu: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(the float64 value before rounding, the stored value as float64) of act(acc + bias[n] + resid), act = ReLU when ``relu``: the
    residual joins BEFORE the ReLU, and there is one rounding, at the end."""
    v = acc
    if bias is not None:
        v = v + bias.double()[None, :]
    if resid is not None:
        v = v + resid
    if relu:
        v = torch.clamp(v, min=0)
    return v, _round_to(v, dtype)


def stats_terms(y: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    "EPI_STATS: the terms of s and q = sum y^2 -- of the STORED output y (float64 of the 16-bit values)."
    return y, y * y


class ReluBwd(NamedTuple):
    y: torch.Tensor         # the stored output: the rounded accumulator, zero where the ReLU was shut
    alive: torch.Tensor     # fma32(Zp, ea, eb) > ALIVE[dtype]
    near: torch.Tensor      # the restated fma lies within one fp32 unit of the threshold: a real fma may decide otherwise
    xhat: torch.Tensor      # (Zp - emean) * einv formed with the kernel's two fp32 operations, as float64


def relu_bwd(acc: torch.Tensor, zp: torch.Tensor, est: torch.Tensor, dtype: torch.dtype) -> ReluBwd:
    "EPI_RELU_BWD on acc float64 [M][N], Zp [M][N] of the 16-bit type and est = f32 (emean | einv | ea | eb)[N]; the sums are of y and y * xhat."
    N = acc.shape[1]
    emean, einv, ea, eb = (est[i * N:(i + 1) * N].float() for i in range(4))
    z = zp.float()
    t = _fma32(z, ea, eb)
    thr = torch.full((), ALIVE[dtype], dtype=torch.float32, device=acc.device)
    lo, hi = torch.nextafter(thr, thr - 1), torch.nextafter(thr, thr + 1)
    alive = t > thr
    xhat = ((z - emean) * einv).double()            # two fp32 operations: a subtraction, then a multiplication
    return ReluBwd(torch.where(alive, _round_to(acc, dtype), torch.zeros_like(acc)), alive, (t >= lo) & (t <= hi), xhat)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------

class Case(NamedTuple):
    name: str
    Cin: int
    N: int
    taps: int
    stride: int
    nimg: int
    H: int                  # INPUT size (1 x M for the plain 1x1 cases: the kernel decodes no position there)
    W: int
    pro: object             # None, "aff" (PRO_AFFINE_RELU), or the relu_mode 0 / 2 / 3 of PRO_BN_BWD
    epi: str                # "", "stats", "resid_bits", "resid", "resid_s2", "relu_bwd", "bias", "bias_resid_relu"
    KT: int                 # K-tiles of 64 per row tile = taps * Cin / 64           (asserted)
    ny: int                 # column tiles; >= 2: the XCD-mapped 1-D grid           (asserted)
    real: bool              # also run with N(0, 1) operands against the summation bound

    @property
    def geo(self) -> Geometry:
        return geometry(self.nimg, self.H, self.W, self.taps, self.stride)[0]

    @property
    def pad(self) -> int:
        return 1 if self.taps == 9 else 0

    @property
    def M(self) -> int:
        return self.geo.M

    @property
    def BN(self) -> int:
        return 128 if self.N % 128 == 0 else 64

    @property
    def plain(self) -> bool:
        return self.taps == 1 and self.stride == 1

    @property
    def res_hw(self) -> Tuple[int, int]:
        "resid_s2: the output grid [nimg][rH][rW] the residual's stride-2 grid belongs to"
        return self.H, self.W


M2, M3, M3S = 65537, 131073 + 128, 131073
# M -> (MT, rounds, gx, (walker, position, rows) of the ragged last tile): walkers() worked through
EXPECT_WALK = {
    M2: (513, 2, 257, (255, 1, 1)),             # walker 255's SECOND tile is the 1-row tile 512; walker 256 has one tile
    M3: (1026, 3, 342, (341, 2, 1)),            # every walker has three tiles, the last walker's third has one row
    M3S: (1025, 3, 342, (340, 2, 1)),           # walker 341 has two tiles, next to walkers with three
    2 * 182 * 182: (518, 2, 259, (258, 1, 72)),    # (the seam between the two images, row 33124, lies in tile 258: a FIRST tile)
    3 * 182 * 182: (777, 2, 389, (387, 1, 44)),    # three images: the second seam, row 66248, lies in tile 517 = walker 128's second
    2 * 363 * 363: (2059, 5, 412, (410, 4, 114)),       # resid_s2 needs the 363 x 363 output grid: five rounds, walker 411 has four tiles
}


def _plain(name, Cin, N, M, pro=None, epi="", real=False):
    return Case(name, Cin, N, 1, 1, 1, 1, M, pro, epi, Cin // 64, N // (128 if N % 128 == 0 else 64), real)


def _conv(name, Cin, N, taps, stride, H, W, real=False, nimg=2):
    return Case(name, Cin, N, taps, stride, nimg, H, W, None, "", taps * Cin // 64, N // (128 if N % 128 == 0 else 64), real)


CASES = [
    # rounds 2, PLAIN: KT 2, 3 (odd), 4; BN 64 and 128; the 2-D grid and the XCD map with gx = 257 (7 idle slots)
    _plain("r2_128x64", 128, 64, M2, real=True),
    _plain("r2_192x64", 192, 64, M2, real=True),
    _plain("r2_128x128", 128, 128, M2),
    _plain("r2_256x256", 256, 256, M2, real=True),
    _plain("r2_64x192", 64, 192, M2),
    # rounds 3, PLAIN: three column tiles on the XCD map; at M3S a walker with two tiles next to walkers with three
    _plain("r3_128x128", 128, 128, M3),
    _plain("r3_192x192", 192, 192, M3, real=True),
    _plain("r3s_128x128", 128, 128, M3S),
    _plain("r3s_192x192", 192, 192, M3S),
    # the position decode in a later round: image borders inside second-round tiles; with three images also a seam between images
    _conv("s2_1x1_c64", 64, 64, 1, 2, 363, 363),
    _conv("s2_1x1_c128", 128, 256, 1, 2, 363, 363, real=True),
    _conv("s2_3x3_c64", 64, 64, 9, 2, 363, 363),
    _conv("s2_3x3_c128", 128, 128, 9, 2, 363, 363, real=True),
    _conv("s1_3x3_c64", 64, 64, 9, 1, 182, 182, real=True),
    _conv("s1_3x3_c128", 128, 128, 9, 1, 182, 182),
    _conv("s2_3x3_c64_n3", 64, 64, 9, 2, 363, 363, nimg=3),
    _conv("s1_3x3_c64_n3", 64, 64, 9, 1, 182, 182, nimg=3),
    # prologues (N = 128: the BN = 128 instantiation of PRO_BN_BWD, whose epilogue operands are loaded late)
    _plain("aff_128x64", 128, 64, M2, "aff", real=True),
    _plain("aff_256x128", 256, 128, M2, "aff"),
    _plain("bn0_128x64", 128, 64, M2, 0),
    _plain("bn0_256x128", 256, 128, M2, 0),
    _plain("bn2_128x64", 128, 64, M2, 2, real=True),
    _plain("bn2_256x128", 256, 128, M2, 2),
    _plain("bn3_128x64", 128, 64, M2, 3),
    _plain("bn3_256x128", 256, 128, M2, 3, real=True),
    # epilogues at rounds 2 with KT 2; the two that carry sums across a walker's tiles also at rounds 3 and on the XCD map
    _plain("stats", 128, 64, M2, None, "stats", real=True),
    _plain("stats_r3", 128, 64, M3, None, "stats"),
    _plain("stats_xcd", 128, 256, M2, None, "stats"),
    _plain("resid_bits", 128, 64, M2, None, "resid_bits"),
    _plain("resid", 128, 64, M2, None, "resid", real=True),
    Case("resid_s2", 128, 64, 1, 1, 2, 363, 363, None, "resid_s2", 2, 1, True),
    _plain("relu_bwd", 128, 64, M2, None, "relu_bwd", real=True),
    _plain("relu_bwd_r3", 128, 64, M3, None, "relu_bwd"),
    _plain("bias", 128, 64, M2, None, "bias"),
    _plain("bias_resid_relu", 128, 64, M2, None, "bias_resid_relu", real=True),
    # the pairs the fused bottleneck launches (pwconv._BottleneckFn): conv3 forward, conv3 data gradient, conv1 data gradient
    _plain("aff_stats", 128, 256, M2, "aff", "stats", real=True),
    _plain("bn3_relu_bwd_256x64", 256, 64, M2, 3, "relu_bwd"),
    _plain("bn3_relu_bwd_256x128", 256, 128, M2, 3, "relu_bwd", real=True),      # BN = 128: Zp is loaded after the last MFMA
    _plain("none_resid_bits_128x256", 128, 256, M2, None, "resid_bits"),
    _plain("bn2_relu_bwd_128x64", 128, 64, M2, 2, "relu_bwd"),
    _plain("bn2_relu_bwd_128x128", 128, 128, M2, 2, "relu_bwd", real=True),
]


# ---- operands ---------------------------------------------------------------------------------------------------------------------------

def _hash32(n: int, key: int, device) -> torch.Tensor:
    "int64 [n] of 32-bit hashes of (index, key).  Every intermediate stays below 2^63: the same integers on every device."
    x = (torch.arange(n, device=device, dtype=torch.int64) * 0x9E3779B1) & 0xFFFFFFFF
    x = ((x ^ (x >> 16)) * 0x45D9F3B) & 0xFFFFFFFF
    x = x ^ key                                     # (after the first round: two keys do not give shifted copies of one sequence)
    for _ in range(2):
        x = ((x ^ (x >> 16)) * 0x45D9F3B) & 0xFFFFFFFF
    return x ^ (x >> 16)


class _Draw:
    def __init__(self, case: Case, integer: bool, seed: int, device):
        self.tag, self.integer, self.device = f"{case.name}/{seed}/", integer, device

    def _h(self, what: str, n: int) -> torch.Tensor:
        return _hash32(n, zlib.crc32((self.tag + what).encode()), self.device)

    def ints(self, what: str, shape, lo: int, hi: int) -> torch.Tensor:
        return (lo + self._h(what, math.prod(shape)) % (hi - lo + 1)).view(shape)

    def uniform(self, what: str, shape) -> torch.Tensor:
        return ((self._h(what, math.prod(shape)).double() + 0.5) / 2.0 ** 32).view(shape)

    def normal(self, what: str, shape) -> torch.Tensor:
        return torch.sqrt(-2.0 * torch.log(self.uniform(what + "/r", shape))) * torch.cos(2.0 * math.pi * self.uniform(what + "/t", shape))

    def values(self, what: str, shape, peak: int, dtype) -> torch.Tensor:
        "integers in [-peak, peak], or N(0, 1)"
        return (self.ints(what, shape, -peak, peak) if self.integer else self.normal(what, shape)).to(dtype)

    def coef(self, what: str, n: int, kind: str) -> torch.Tensor:
        "scale: {1, 2} / U(0.5, 1.5); small, shift: {-1, 0, 1} / N(0, 0.05^2), N(0, 0.3^2)"
        if self.integer:
            return (self.ints(what, (n,), 1, 2) if kind == "scale" else self.ints(what, (n,), -1, 1)).float()
        if kind == "scale":
            return (self.uniform(what, (n,)) + 0.5).float()
        return (self.normal(what, (n,)) * (0.3 if kind == "shift" else 0.05)).float()


class Operands(NamedTuple):
    x: torch.Tensor                 # [rows][Cin], 16-bit
    w: torch.Tensor                 # [N][taps][Cin]
    z: Optional[torch.Tensor]       # PRO_BN_BWD: the BN input, [rows][Cin]
    coef3: Optional[torch.Tensor]   # f32 (a | k0 | k1)[Cin]
    fwd: Optional[torch.Tensor]     # relu_mode 2: f32 (fa | fb)[Cin]
    xbits: Optional[torch.Tensor]   # relu_mode 3: uint8 [rows * Cin / 8]
    xcoef: Optional[torch.Tensor]   # PRO_AFFINE_RELU: f32 (a | b)[Cin]
    bias: Optional[torch.Tensor]    # f32 [N]
    R: Optional[torch.Tensor]       # [M][N], or the stride-2 grid's rows
    rbits: Optional[torch.Tensor]   # uint8 [M * N / 8]
    zp: Optional[torch.Tensor]      # EPI_RELU_BWD: [M][N]
    est: Optional[torch.Tensor]     # f32 (emean | einv | ea | eb)[N]


X_PEAK, W_PEAK, E_PEAK = 2, 2, 3      # integer operands: |X|, |z| <= 2, |W| <= 2; bias, R, Zp in [-3, 3]
XT_PEAK = {None: X_PEAK, "aff": 2 * X_PEAK + 1, 0: 3 * X_PEAK + 1, 2: 3 * X_PEAK + 1, 3: 3 * X_PEAK + 1}     # |X'| of the integer generator


def operands(case: Case, dtype: torch.dtype, integer: bool, device="cpu", seed: int = 0) -> Operands:
    """Tensors for ``case`` on ``device``.  integer: small integers and integer coefficients (scales 1 or 2, offsets in [-1, 1]), so every
    transformed operand is an integer of magnitude <= XT_PEAK, exact in bf16 and fp16, and every accumulator and every partial sum stays
    far below 2^24: fp32 arithmetic is exact in any order.  Otherwise N(0, 1) operands and BatchNorm-like real coefficients."""
    d = _Draw(case, integer, seed, device)
    rows, M, Cin, N = case.geo.rows, case.M, case.Cin, case.N
    x = d.values("x", (rows, Cin), X_PEAK, dtype)
    w = d.values("w", (N, case.taps, Cin), W_PEAK, dtype)
    z = coef3 = fwd = xbits = xcoef = None
    if case.pro == "aff":
        xcoef = torch.cat([d.coef("xa", Cin, "scale"), d.coef("xb", Cin, "shift")])
    elif case.pro is not None:
        z = d.values("z", (rows, Cin), X_PEAK, dtype)
        coef3 = torch.cat([d.coef("pa", Cin, "scale"), d.coef("pk0", Cin, "small"), d.coef("pk1", Cin, "small")])
        if case.pro == 2:
            fwd = torch.cat([d.coef("fa", Cin, "scale"), d.coef("fb", Cin, "shift")])
        if case.pro == 3:
            xbits = pack_bits(d.uniform("xbits", (rows, Cin)) > 0.4)
    return Operands(x, w, z, coef3, fwd, xbits, xcoef, *epilogue_operands(case, dtype, integer, device, seed))


def epilogue_operands(case: Case, dtype: torch.dtype, integer: bool, device="cpu", seed: int = 0):
    "(bias, R, rbits, zp, est) of ``operands``: what the epilogue of ``case`` reads."
    d = _Draw(case, integer, seed, device)
    M, N = case.M, case.N
    bias = R = rbits = zp = est = None
    if case.epi in ("bias", "bias_resid_relu"):
        bias = d.values("bias", (N,), E_PEAK, torch.float32)
    if case.epi in ("resid", "resid_bits", "bias_resid_relu"):
        R = d.values("R", (M, N), E_PEAK, dtype)
        if case.epi == "resid_bits":
            rbits = pack_bits(d.uniform("rbits", (M, N)) > 0.5)
    if case.epi == "resid_s2":
        rH, rW = case.res_hw
        R = d.values("R", (case.nimg * ((rH + 1) // 2) * ((rW + 1) // 2), N), E_PEAK, dtype)
    if case.epi == "relu_bwd":
        zp = d.values("zp", (M, N), E_PEAK, dtype)
        est = torch.cat([d.coef("emean", N, "shift"), d.coef("einv", N, "scale"), d.coef("ea", N, "scale"), d.coef("eb", N, "shift")])
    return bias, R, rbits, zp, est


def round_f16_once(v: torch.Tensor) -> torch.Tensor:
    "float64 -> the nearest fp16 value (ties to even), as float64: ONE rounding, not one to fp32 and a second to fp16."
    _, e = torch.frexp(v.abs())                                    # |v| = m 2^e, m in [0.5, 1): 11 significant bits end at 2^(e - 11)
    q = torch.clamp(e - 11, min=-24)                                # (subnormals: multiples of 2^-24)
    # 2^q and 2^-q from their bit patterns: exact on every device (torch.ldexp multiplies by pow(2, q), which a GPU may round)
    up, down = (((q.long() + 1023) << 52).view(torch.float64) for q in (q, -q))
    return torch.round(v * down) * up                               # torch.round: halves to even


def pro_bn_bwd_f16(g: torch.Tensor, z: torch.Tensor, coef3: torch.Tensor, relu_mode: int, fwd: Optional[torch.Tensor] = None,
                   bits: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``pro_bn_bwd`` as the fp16 instantiation of pw_gemm_kernel is compiled: the outer multiply-add of dz = fmaf(a, g', fmaf(k1, z, k0))
    and the conversion to fp16 are ONE instruction there (v_fma_mixlo_f16 / v_fma_mixhi_f16 in the kernel's code object: fp32 operands,
    the exact a g' + t rounded once to fp16), where the bf16 instantiation rounds to fp32 and converts.  The inner fma is an fp32 one in
    both.  The two restatements differ where the fp32 rounding lands on an fp16 tie: about one element in 2^13, by one fp16 unit."""
    Cc = g.shape[1]
    a, k0, k1 = coef3[:Cc].float(), coef3[Cc:2 * Cc].float(), coef3[2 * Cc:].float()
    gj, zf = g.float(), z.float()
    if relu_mode == 2:
        gj = torch.where(_fma32(zf, fwd[:Cc].float(), fwd[Cc:].float()) > ALIVE[torch.float16], gj, torch.zeros_like(gj))
    elif relu_mode == 3:
        gj = torch.where(unpack_bits(bits, g.shape[0], Cc), gj, torch.zeros_like(gj))
    else:
        assert relu_mode == 0
    # (24 x 11 bits of product + 24 bits of t: float64 holds the sum exactly unless their exponents lie more than 18 apart, and then
    # its own rounding is 2^-29 of an fp32 unit away from mattering)
    return round_f16_once(a.double() * gj.double() + _fma32(k1, zf, k0).double())


def transformed(case: Case, op: Operands, dtype: torch.dtype) -> torch.Tensor:
    "X' in float64: what the kernel multiplies."
    if case.pro is None:
        return op.x.double()
    if case.pro == "aff":
        return pro_affine_relu(op.x, op.xcoef, dtype)
    if dtype == torch.float16:
        return pro_bn_bwd_f16(op.x, op.z, op.coef3, case.pro, op.fwd, op.xbits)
    return pro_bn_bwd(op.x, op.z, op.coef3, case.pro, dtype, op.fwd, op.xbits)


class Expected(NamedTuple):
    acc: torch.Tensor                       # float64 [M][N]: the contraction
    pre: torch.Tensor                       # the value the epilogue rounds (float64)
    y: torch.Tensor                         # the stored output (float64 of the 16-bit value)
    keep: Optional[torch.Tensor]            # relu_bwd: elements whose mask the restatement decides for certain (else None: all)
    alive: Optional[torch.Tensor]
    xhat: Optional[torch.Tensor]            # relu_bwd: the factor of the second sum
    extra_terms: int                        # addends the epilogue puts on top of the K products
    extra_abs: Optional[torch.Tensor]       # ... and their magnitudes, float64 [M][N] (or None)


def expected(case: Case, op: Operands, dtype: torch.dtype, xt: Optional[torch.Tensor] = None) -> Expected:
    "The reference output of ``case``: the contraction, then the case's epilogue restated in float64 with the kernel's roundings."
    xt = transformed(case, op, dtype) if xt is None else xt
    acc = gemm_ref(xt, op.w, case.taps, case.stride, case.pad, case.geo)
    if case.epi == "relu_bwd":
        rb = relu_bwd(acc, op.zp, op.est, dtype)
        return Expected(acc, acc, rb.y, ~rb.near, rb.alive, rb.xhat, 0, None)
    resid = None
    if case.epi in ("resid", "resid_bits", "bias_resid_relu"):
        resid = resid_term(op.R, op.rbits, 1, case.M)
    elif case.epi == "resid_s2":
        resid = resid_term(op.R, None, 2, case.M, *case.res_hw)
    pre, y = epi_store(acc, dtype, op.bias, resid, relu=case.epi == "bias_resid_relu")
    extra = (op.bias is not None) + (resid is not None)
    extra_abs = None
    if extra:
        extra_abs = torch.zeros_like(acc)
        if op.bias is not None:
            extra_abs += op.bias.double().abs()[None, :]
        if resid is not None:
            extra_abs += resid.abs()
    return Expected(acc, pre, y, None, None, None, extra, extra_abs)


def partial_terms(case: Case, ex: Expected, y: torch.Tensor) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
    "The terms of the two column sums of ``case`` over the stored output ``y`` (float64 [M][N]), or None where the epilogue keeps none."
    if case.epi == "stats":
        return stats_terms(y)
    if case.epi == "relu_bwd":
        return y, y * ex.xhat
    return None
