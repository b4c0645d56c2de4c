"""Float64 reference of ``pw_wgrad_kernel`` (csrc/pw.hip) and the shapes its tests run, shared by ``test_pw_wgrad_ref.py``
(CPU: the reference against torch's float64 convolution backward, the operand generators) and ``test_pw_wgrad_gpu.py``.

    dW[n][tap][c] = sum_m  G'[m][n] * X'[pos(m, tap)][c]          G' = gpro(G), X' = xpro(X), both rounded to the 16-bit type

``wgrad_ref`` is index arithmetic and one float64 matmul per tap -- no torch convolution -- on the 16-bit operand VALUES, so
whatever separates it from the kernel is the kernel's.  ``pro_bn_bwd`` / ``pro_affine_relu`` restate ``transform<>`` with the
kernel's own fp32 multiply-adds and its rounding of the transformed operand to the element type.

The shapes (``CASES``) are the smallest that put more than one 64-position K-tile into a workgroup (``tiles_per_split`` > 1) on
each of the six (TN, TK) tiles: the S / KT columns are ``wgrad_splits`` worked through for 256 CUs and are documentation --
the GPU test reads S from the library and fails if a case no longer reaches the depth it claims.

numpy's PCG64 draws the operands (as tests/synth.py does), so the CPU test sees the bytes the GPU test runs.
"""
import struct
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch


class Geometry(NamedTuple):
    nimg: int
    H: int
    W: int
    Ho: int
    Wo: int

    @property
    def M(self) -> int:
        return self.nimg * self.Ho * self.Wo

    @property
    def rows(self) -> int:
        return self.nimg * self.H * self.W


def geometry(nimg: int, H: int, W: int, taps: int, stride: int) -> Tuple[Geometry, int]:
    "Output grid of a k x k / stride / pad k // 2 convolution over [nimg][H][W] (k = 3 for 9 taps, else 1); returns (geometry, pad)."
    k, pad = (3, 1) if taps == 9 else (1, 0)
    return Geometry(nimg, H, W, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1), pad


def tap_rows(geo: Geometry, taps: int, stride: int, pad: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    "pos(m, tap): the input row of output row m = (n, ho, wo) under each tap [taps][M], and whether the tap stays inside the image."
    m = torch.arange(geo.M, device=device, dtype=torch.int64)
    hw = geo.Ho * geo.Wo
    n, rem = m // hw, m % hw
    ho, wo = rem // geo.Wo, rem % geo.Wo
    rows, oks = [], []
    for tap in range(taps):
        dy, dx = (tap // 3, tap % 3) if taps == 9 else (0, 0)
        y, x = ho * stride - pad + dy, wo * stride - pad + dx
        ok = (y >= 0) & (y < geo.H) & (x >= 0) & (x < geo.W)
        rows.append(torch.where(ok, n * (geo.H * geo.W) + y * geo.W + x, torch.zeros_like(m)))
        oks.append(ok)
    return torch.stack(rows), torch.stack(oks)


def wgrad_ref(g2d: torch.Tensor, x: torch.Tensor, taps: int, stride: int, pad: int, geo: Geometry) -> torch.Tensor:
    "float64 [N][taps][Cin] from g2d [M][N] and x [nimg * H * W][Cin] (any float type: the values are taken as they are)."
    assert g2d.shape[0] == geo.M and x.shape[0] == geo.rows, (tuple(g2d.shape), tuple(x.shape), geo)
    g, xd = g2d.double(), x.double()
    rows, ok = tap_rows(geo, taps, stride, pad, g.device)
    out = torch.empty((g.shape[1], taps, xd.shape[1]), dtype=torch.float64, device=g.device)
    gt = g.t().contiguous()
    for tap in range(taps):
        xt = torch.where(ok[tap][:, None], xd[rows[tap]], torch.zeros((), dtype=torch.float64, device=g.device))
        out[:, tap, :] = gt @ xt
    return out


def abs_terms_sum(g2d: torch.Tensor, x: torch.Tensor, taps: int, stride: int, pad: int, geo: Geometry) -> torch.Tensor:
    "sum_m |G[m][n] * X[pos(m, tap)][c]| with the reference's own gather."
    return wgrad_ref(g2d.double().abs(), x.double().abs(), taps, stride, pad, geo)


def sum_bound(M: int, abs_sum: torch.Tensor) -> torch.Tensor:
    """``_sum_bound`` of test_pwconv_gpu.py for a sum of M exact products: |fp32 sum - exact sum| <= (M - 1) 2^-24 sum |term| for ANY
    order of summation with one rounding per addition (products of two 16-bit values are exact in fp32: 8 + 8 or 11 + 11 bits)."""
    return (M - 1) * 2.0 ** -24 * abs_sum


def half_ulp(ref: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    "Half a unit in the last place of ``dtype`` at |ref| (float64)."
    p, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    _, e = torch.frexp(ref.abs())                       # |ref| = m 2^e, m in [0.5, 1)
    e = torch.where(ref == 0, torch.full_like(e, -2000), e)
    return torch.ldexp(torch.ones_like(ref), torch.clamp(e - 1, min=emin) - p - 1)


# ---- the operand prologues (csrc/pw.hip: load_coef<>, transform<>) -----------------------------------------------------------

def _f32_bits(u: int) -> float:
    return struct.unpack("<f", struct.pack("<I", u))[0]


# alive_dt<DT>(): the threshold a pre-activation must exceed for its ReLU to count as open
ALIVE = {torch.bfloat16: _f32_bits(0x00004000), torch.float16: _f32_bits(0x33000000)}


def _fma32(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    "fmaf(a, b, c) on fp32 values: the product of two fp32 numbers is exact in float64, the sum is rounded there and once more to fp32."
    return (a.double() * b.double() + c.double()).float()


def pack_bits(mask: torch.Tensor) -> torch.Tensor:
    "ReLU bits as the kernels read them: uint8 [M * C / 8], bit j of byte (m * C + c) / 8 = channel c + j."
    M, Cc = mask.shape
    w = 2 ** torch.arange(8, device=mask.device, dtype=torch.int32)
    return (mask.view(M, Cc // 8, 8).to(torch.int32) * w).sum(-1).to(torch.uint8).contiguous().view(-1)


def unpack_bits(bits: torch.Tensor, M: int, Cc: int) -> torch.Tensor:
    b = bits.view(M, Cc // 8, 1).to(torch.int32)
    return ((b >> torch.arange(8, device=bits.device, dtype=torch.int32)) & 1).bool().view(M, Cc)


def pro_bn_bwd(g: torch.Tensor, z: torch.Tensor, coef3: torch.Tensor, relu_mode: int, dtype: torch.dtype,
               fwd: Optional[torch.Tensor] = None, bits: Optional[torch.Tensor] = None) -> torch.Tensor:
    """PRO_BN_BWD on [M][C] operands: dz = fmaf(a, g', fmaf(k1, z, k0)), coef3 = f32 (a | k0 | k1); g' = g where the ReLU was open --
    mode 0: everywhere, 2: fmaf(z, fa, fb) > alive with fwd = f32 (fa | fb), 3: the packed bits.  Returns the value the kernel stages:
    rounded to ``dtype``, as float64."""
    Cc = g.shape[1]
    a, k0, k1 = coef3[:Cc].float(), coef3[Cc:2 * Cc].float(), coef3[2 * Cc:].float()
    gj, zf = g.float(), z.float()
    if relu_mode == 2:
        gj = torch.where(_fma32(zf, fwd[:Cc].float(), fwd[Cc:].float()) > ALIVE[dtype], gj, torch.zeros_like(gj))
    elif relu_mode == 3:
        gj = torch.where(unpack_bits(bits, g.shape[0], Cc), gj, torch.zeros_like(gj))
    else:
        assert relu_mode == 0
    return _fma32(a, gj, _fma32(k1, zf, k0)).to(dtype).double()


def pro_affine_relu(x: torch.Tensor, coef2: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    "PRO_AFFINE_RELU on [rows][C]: t = fmaf(x, a, b); t > 0 ? t : 0; rounded to ``dtype``; coef2 = f32 (a | b)."
    Cc = x.shape[1]
    t = _fma32(x.float(), coef2[:Cc].float(), coef2[Cc:].float())
    return torch.where(t > 0, t, torch.zeros_like(t)).to(dtype).double()


# ---- launch shape (csrc/pw.hip: wgrad_tile, launch_wgrad_dt) ----------------------------------------------------------------

def wgrad_tile(N: int, Cin: int, g_transform: bool) -> Tuple[int, int]:
    if N >= 128 and Cin >= 128:
        TN, TK = 128, 128
    elif N >= 128:
        TN, TK = (256 if N >= 256 and not g_transform else 128), 64
    elif Cin >= 128:
        TN, TK = 64, (256 if Cin >= 256 else 128)
    else:
        TN, TK = 64, 64
    while N % TN:
        TN >>= 1
    while Cin % TK:
        TK >>= 1
    return TN, TK


class Launch(NamedTuple):
    tile: Tuple[int, int]
    gy: int             # output tiles (column tiles x row tiles x taps)
    ktiles: int         # 64-position K-tiles in M
    S: int
    KT: int             # K-tiles a workgroup walks
    xcd: bool           # the 1-D XCD-mapped grid (else the plain S x gy grid)
    last_tiles: int     # K-tiles of the last split
    ragged: int         # rows of the last K-tile (0: full)


def launch_of(case: "Case", S: int) -> Launch:
    "What the kernel runs for ``case`` when the library reports S splits."
    tile = wgrad_tile(case.N, case.Cin, case.gpro is not None)
    gy = (case.N // tile[0]) * (case.Cin // tile[1]) * case.taps
    ktiles = (case.M + 63) // 64
    KT = (ktiles + S - 1) // S
    return Launch(tile, gy, ktiles, S, KT, 2 <= gy <= 64 and S >= 8, ktiles - (S - 1) * KT, case.M % 64)


# ---- the cases -------------------------------------------------------------------------------------------------------------

class Case(NamedTuple):
    name: str
    N: int
    Cin: int
    taps: int
    stride: int
    nimg: int
    H: int              # INPUT size
    W: int
    gpro: Optional[int]     # None, or the relu_mode of a PRO_BN_BWD prologue on G
    xpro: bool              # PRO_AFFINE_RELU on X
    depth: int              # K-tiles per workgroup the case exists for: asserted against the library's S
    tile: Tuple[int, int]
    S: int                  # at 256 CUs (documentation)
    KT: int
    xcd: bool               # grid form, asserted
    s_mod8_zero: Optional[bool]     # asserted where the case is there for it
    short_last: Optional[bool]      # the last split holds fewer K-tiles than the others: asserted where the case is there for it
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


#        name              N     Cin  taps s  img  H    W   gpro  xpro  depth tile       S    KT  xcd    S%8==0 short  real
CASES = [
    Case("t128x128_m1050", 2048, 512, 1, 1, 2, 21, 25, None, False, 3, (128, 128), 6, 3, False, None, True, True),      # last split: 2 of 3 tiles, 26 rows in the last
    Case("t128x128_m1150", 2048, 512, 1, 1, 2, 23, 25, None, False, 3, (128, 128), 6, 3, False, None, False, False),    # last split full, 62 rows in the last tile
    Case("t128x128_gy128", 2048, 1024, 1, 1, 2, 19, 23, None, False, 4, (128, 128), 4, 4, False, None, True, False),    # gy = 128 > 64: plain grid
    Case("t256x64_m4230", 2048, 64, 1, 1, 2, 47, 45, None, False, 2, (256, 64), 34, 2, True, False, True, True),        # last split: one tile of 6 rows; S % 8 = 2
    Case("t128x64_n1920", 1920, 64, 1, 1, 2, 33, 37, None, False, 2, (128, 64), 20, 2, True, False, True, True),        # 256 does not divide 1920
    Case("t64x256_m5074", 64, 2048, 1, 1, 2, 43, 59, None, False, 2, (64, 256), 40, 2, True, True, False, True),        # S % 8 = 0 on the XCD map
    Case("t64x128_c1920", 64, 1920, 1, 1, 2, 33, 37, None, False, 2, (64, 128), 20, 2, True, False, True, True),
    Case("t64x64_3x3", 64, 64, 9, 1, 2, 45, 43, None, False, 2, (64, 64), 31, 2, True, False, True, True),
    Case("t64x64_3x3_s2", 64, 64, 9, 2, 2, 89, 85, None, False, 2, (64, 64), 31, 2, True, False, True, False),          # odd input: the last row / column tap is inside
    Case("t64x64_one_tile", 64, 64, 1, 1, 2, 130, 130, None, False, 2, (64, 64), 265, 2, False, None, True, False),     # gy = 1
    Case("t128x128_3x3_s2", 128, 128, 9, 2, 3, 71, 69, None, False, 2, (128, 128), 30, 2, True, False, False, True),    # 1260 rows per image: borders inside K-tiles
    Case("t128x128_1x1_s2", 512, 256, 1, 2, 2, 129, 129, None, False, 3, (128, 128), 45, 3, True, False, True, False),  # KT = 3 on the XCD map
    # prologues: conv3's weight gradient of a fused bottleneck (bn3-backward with ReLU bits on G, relu(bn2) on X) at layer1 / layer2 widths
    Case("bn3_aff_256x64", 256, 64, 1, 1, 2, 91, 93, 3, True, 2, (128, 64), 133, 2, True, False, True, True),
    Case("bn3_aff_512x128", 512, 128, 1, 1, 2, 65, 67, 3, True, 2, (128, 128), 69, 2, True, False, True, True),
    # the other two forms of the ReLU mask (instantiated, not reached by today's call sites)
    Case("bn2_2048x64", 2048, 64, 1, 1, 2, 33, 37, 2, False, 2, (128, 64), 20, 2, True, False, True, True),
    Case("bn0_2048x64", 2048, 64, 1, 1, 2, 33, 37, 0, False, 2, (128, 64), 20, 2, True, False, True, False),
]


class Operands(NamedTuple):
    g: torch.Tensor                 # [M][N], 16-bit
    x: torch.Tensor                 # [rows][Cin]
    z: Optional[torch.Tensor]       # PRO_BN_BWD: the BN input [M][N]
    coef3: Optional[torch.Tensor]   # f32 (a | k0 | k1)
    fwd: Optional[torch.Tensor]     # relu_mode 2: f32 (fa | fb)
    bits: Optional[torch.Tensor]    # relu_mode 3: uint8 [M * N / 8]
    xcoef: Optional[torch.Tensor]   # PRO_AFFINE_RELU: f32 (a | b)


def _t(a: np.ndarray, dtype: torch.dtype) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def operands(case: Case, dtype: torch.dtype, integer: bool, seed: int = 0) -> Operands:
    """CPU tensors for ``case``.  integer: G, X, z in [-3, 3] and integer coefficients (scale 1 or 2, offsets in [-1, 1]), so every
    transformed operand is an integer of magnitude <= 10 (G') / 7 (X'), exact in bf16 and fp16, and every partial sum stays below 2^24
    (``operand_peak``): fp32 accumulation is exact in any order.  Otherwise N(0, 1) operands and BatchNorm-like real coefficients."""
    rng = np.random.default_rng(1000 + seed)
    M, rows, N, Cin = case.M, case.geo.rows, case.N, case.Cin

    def draw(shape):
        if integer:
            return rng.integers(-3, 4, size=shape).astype(np.float32)
        return rng.standard_normal(shape, dtype=np.float32)

    def coef(n, kind):
        if integer:
            return rng.integers(1, 3, size=n).astype(np.float32) if kind == "scale" else rng.integers(-1, 2, size=n).astype(np.float32)
        return (rng.random(n, dtype=np.float32) + 0.5) if kind == "scale" else rng.standard_normal(n, dtype=np.float32) * (0.3 if kind == "shift" else 0.05)

    g, x = _t(draw((M, N)), dtype), _t(draw((rows, Cin)), dtype)
    z = coef3 = fwd = bits = xcoef = None
    if case.gpro is not None:
        z = _t(draw((M, N)), dtype)
        coef3 = _t(np.concatenate([coef(N, "scale"), coef(N, "small"), coef(N, "small")]), torch.float32)
        if case.gpro == 2:
            fwd = _t(np.concatenate([coef(N, "scale"), coef(N, "shift")]), torch.float32)
        if case.gpro == 3:
            bits = pack_bits(torch.from_numpy(rng.random((M, N)) > 0.4))
    if case.xpro:
        xcoef = _t(np.concatenate([coef(Cin, "scale"), coef(Cin, "shift")]), torch.float32)
    return Operands(g, x, z, coef3, fwd, bits, xcoef)


def transformed(case: Case, op: Operands, dtype: torch.dtype) -> Tuple[torch.Tensor, torch.Tensor]:
    "(G', X') in float64: what the kernel multiplies."
    g = op.g.double() if case.gpro is None else pro_bn_bwd(op.g, op.z, op.coef3, case.gpro, dtype, op.fwd, op.bits)
    x = pro_affine_relu(op.x, op.xcoef, dtype) if case.xpro else op.x.double()
    return g, x


def operand_peak(case: Case, gt: torch.Tensor, xt: torch.Tensor) -> float:
    "Upper bound on every partial sum of |G'| |X'| over the M positions of ``case``."
    return float(gt.abs().max()) * float(xt.abs().max()) * case.M
