"""Float64 references, schedule restatements and integer operands of the tests of the dense 3x3 MFMA family of csrc/conv.hip --
``conv3x3_canvas_kernel<MODE_DENSE>`` (``rn_conv3x3_dense_batched[_act]``, ``rn_conv3x3_dense_splitk``), ``conv3x3_dense_band_kernel``
(``rn_conv3x3_dense_band[_stats]``) and ``conv3x3_wgrad_kernel<DENSE>`` + ``wgrad_reduce_dense_kernel`` (``rn_conv3x3_dense_wgrad_batched``)
-- shared by ``test_dense_conv_ref.py`` (CPU: the references against torch's float64 convolution and its autograd, the restatements by
hand, the generators' promises) and ``test_dense_conv_exact_gpu.py``.

    y[n][h][w][o]    = sum over (kh, kw, c) of x[n][h + kh - 1][w + kw - 1][c] * w[o][kh][kw][c]          (zero outside the image)
    dW[o][kh][kw][c] = sum over (n, h, w) of g[n][h][w][o] * x[n][h + kh - 1][w + kw - 1][c]

The references are numpy only: a zero-padded shift per tap and one float64 matmul per tap on the VALUES of the operands -- no torch
convolution, no MIOpen.  Float64 products and sums of small integers are exact in any order, so on the integer operands below whatever
separates a kernel from the reference is the kernel's.

The schedule functions restate, from the comments and the host code of csrc/conv.hip, which workgroup owns which rows, which K-tiles and
which positions, as functions of the shape and the CU count alone; the GPU tests assert on them that a case reaches the path it is here for.
"""
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

CONV_BM = 256           # positions of a row tile (forward kernels); tiles run over the flattened N * H * W positions
CONV_BN = 256           # output channels of a column tile of the MODE_DENSE launch
BAND_BN = 128           # ... of the band kernel
CONV_BK = 64            # channels of a K-tile (one chunk of one tap)
BAND_POS = CONV_BM + 2  # positions of a band: the tile's 256 and one to either side
WG_POS = 64             # positions of a K-tile of the weight gradient
MAX_PROBLEMS = 4


# ---- float64 references ------------------------------------------------------------------------------------------------------------

def shifted_taps(x: np.ndarray) -> np.ndarray:
    "x [N][H][W][C] -> float64 [N * H * W][9][C]: under tap (kh, kw) position (h, w) sees x[h + kh - 1][w + kw - 1], zero outside the image."
    N, H, W, C = x.shape
    xp = np.zeros((N, H + 2, W + 2, C), np.float64)
    xp[:, 1:H + 1, 1:W + 1] = x
    return np.stack([xp[:, kh:kh + H, kw:kw + W] for kh in range(3) for kw in range(3)], axis=3).reshape(N * H * W, 9, C)


def conv_ref(x: np.ndarray, w: np.ndarray, bias: Optional[np.ndarray] = None, relu: bool = False,
             ktiles: Optional[Tuple[int, int]] = None) -> np.ndarray:
    """float64 y [N][H][W][Cout] from x [N][H][W][Cin] and w [Cout][3][3][Cin]: 3x3, stride 1, pad 1; with ``bias`` conv + bias, with
    ``relu`` max(., 0) of that.  ``ktiles`` = (k0, k1): only K-tiles k0 <= kt < k1 of the MODE_DENSE walk, kt = 9 * chunk + tap (chunk
    outer, tap inner, 64 channels each) -- what one range of the split-K launch sums."""
    N, H, W, Cin = x.shape
    Cout = w.shape[0]
    xt = shifted_taps(x)
    wd = np.asarray(w, np.float64).reshape(Cout, 9, Cin)
    y = np.zeros((N * H * W, Cout), np.float64)
    k0, k1 = ktiles if ktiles is not None else (0, 9 * ((Cin + CONV_BK - 1) // CONV_BK))
    for kt in range(k0, k1):
        chunk, tap = divmod(kt, 9)
        c0, c1 = chunk * CONV_BK, min((chunk + 1) * CONV_BK, Cin)
        y += xt[:, tap, c0:c1] @ wd[:, tap, c0:c1].T
    if bias is not None:
        y = y + np.asarray(bias, np.float64)[None, :]
    if relu:
        y = np.maximum(y, 0.0)
    return y.reshape(N, H, W, Cout)


def wgrad_ref_ranges(g: np.ndarray, x: np.ndarray, ranges: Sequence[Tuple[int, int]]) -> List[np.ndarray]:
    "``wgrad_ref`` restricted to each (m0, m1) of ``ranges`` in turn (the taps are gathered once)."
    N, H, W, Cout = g.shape
    Cin = x.shape[3]
    M = N * H * W
    gd = np.asarray(g, np.float64).reshape(M, Cout)
    xt = shifted_taps(x).reshape(M, 9 * Cin)
    out = []
    for m0, m1 in ranges:
        m0, m1 = max(0, min(m0, M)), max(0, min(m1, M))
        out.append((gd[m0:m1].T @ xt[m0:m1]).reshape(Cout, 3, 3, Cin))
    return out


def wgrad_ref(g: np.ndarray, x: np.ndarray, rows: Optional[Tuple[int, int]] = None) -> np.ndarray:
    """float64 dW [Cout][3][3][Cin] from g [N][H][W][Cout] and x [N][H][W][Cin]; ``rows`` = (m0, m1): only the flattened positions
    m0 <= m < m1 contribute (the taps of a position still reach its neighbours, inside or outside the range)."""
    N, H, W, _ = g.shape
    return wgrad_ref_ranges(g, x, [rows if rows is not None else (0, N * H * W)])[0]


def abs_conv_ref(x: np.ndarray, w: np.ndarray) -> np.ndarray:
    "sum over (tap, channel) of |x| |w| per output: what the rounding bound of a real-valued run is built from."
    return conv_ref(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)))


def abs_wgrad_ref(g: np.ndarray, x: np.ndarray, rows: Optional[Tuple[int, int]] = None) -> np.ndarray:
    return wgrad_ref(np.abs(np.asarray(g, np.float64)), np.abs(np.asarray(x, np.float64)), rows)


def dgrad_weights(w: np.ndarray) -> np.ndarray:
    "w [Cout][3][3][Cin] -> [Cin][3][3][Cout], out[ci][8 - t][co] = w[co][t][ci]: the input gradient is conv_ref(g, dgrad_weights(w))."
    return np.ascontiguousarray(np.asarray(w)[:, ::-1, ::-1, :].transpose(3, 1, 2, 0))


def sum_bound(K: int, abs_sum: np.ndarray) -> np.ndarray:
    "|fp32 sum - exact sum| <= (K - 1) 2^-24 sum |term| for K exact terms added in any order, one rounding per addition."
    return (K - 1) * 2.0 ** -24 * abs_sum


def half_ulp(ref: np.ndarray, bf16: bool) -> np.ndarray:
    "Half a unit in the last place of bf16 / fp16 at |ref| (float64)."
    p, emin = (7, -126) if bf16 else (10, -14)
    _, e = np.frexp(np.abs(ref))
    e = np.where(ref == 0, -2000, e)
    return np.ldexp(1.0, np.maximum(e - 1, emin) - p - 1)


# ---- the schedules: who owns which rows, K-tiles and positions ------------------------------------------------------------------------

def row_tiles(M: int) -> int:
    return (M + CONV_BM - 1) // CONV_BM


class DenseGrid(NamedTuple):
    tile_beg: List[int]         # first row tile of problem p in blockIdx.x, and the total behind the last
    col_tiles: int
    ktiles: int                 # K-tiles a workgroup walks: 9 taps x Cin / 64 chunks

    @property
    def tiles(self) -> int:
        return self.tile_beg[-1]

    def tiles_of(self, p: int) -> int:
        return self.tile_beg[p + 1] - self.tile_beg[p]


def dense_grid(Ms: Sequence[int], Cin: int, Cout: int) -> DenseGrid:
    "rn_conv3x3_dense_batched_act: the problems' row tiles one after the other in blockIdx.x, Cout / 256 column tiles in blockIdx.y."
    assert 1 <= len(Ms) <= MAX_PROBLEMS and Cin % CONV_BK == 0 and Cout % CONV_BN == 0
    beg = [0]
    for M in Ms:
        beg.append(beg[-1] + row_tiles(M))
    return DenseGrid(beg, Cout // CONV_BN, 9 * (Cin // CONV_BK))


def straddling_tiles(N: int, H: int, W: int) -> int:
    "Row tiles of [N * H * W] that hold positions of two images."
    M, hw = N * H * W, H * W
    return sum(1 for t in range(row_tiles(M)) if (t * CONV_BM) // hw != (min((t + 1) * CONV_BM, M) - 1) // hw)


class BandWalk(NamedTuple):
    tiles: int
    col_tiles: int
    NB: int                                     # bands per tile: 3 kernel rows x Cin / 64 chunks
    bands: List[Tuple[int, int, int]]           # band b -> (chunk, kernel row, band buffer b & 1); its taps 3 r + s read tap buffer s
    last_rows: int                              # positions of the last tile


def band_walk(N: int, H: int, W: int, Cin: int, Cout: int) -> BandWalk:
    """conv3x3_dense_band_kernel: band b is (chunk b / 3, kernel row b % 3): the 258 positions from m0 + (r - 1) W - 1, clamped into the
    tensor, in band buffer b & 1; tap column s of the band reads tap buffer s (three buffers, refilled one step after their last reader)."""
    assert Cin % CONV_BK == 0 and Cout % BAND_BN == 0
    M = N * H * W
    NB = 3 * (Cin // CONV_BK)
    return BandWalk(row_tiles(M), Cout // BAND_BN, NB, [(b // 3, b % 3, b & 1) for b in range(NB)], M - (row_tiles(M) - 1) * CONV_BM)


def dense_ksplit(M: int, Cout: int, cus: int) -> int:
    "K ranges of rn_conv3x3_dense_splitk: cus / workgroups, at most 3; 1 = the entry point declines."
    wgs = row_tiles(M) * (Cout // CONV_BN)
    if wgs <= 0:
        return 0
    s = cus // wgs
    return 3 if s >= 3 else (2 if s >= 2 else 1)


def ksplit_ranges(Cin: int, S: int) -> List[Tuple[int, int]]:
    "conv3x3_canvas_kernel, ksplit > 1: range z walks K-tiles z KT / S .. (z + 1) KT / S - 1 of the walk (kt = 9 * chunk + tap)."
    KT = 9 * (Cin // CONV_BK)
    return [(z * KT // S, (z + 1) * KT // S) for z in range(S)]


class WgradSplits(NamedTuple):
    budget: int
    tps: int                                    # K-tiles (64 positions) per split
    beg: List[int]                              # first split of problem p, and the total behind the last
    rows: List[Tuple[int, int, int]]            # split -> (problem, m0, m1): the positions it sums (the last of a problem: what is left)

    @property
    def total(self) -> int:
        return self.beg[-1]

    def tiles_of(self, s: int) -> int:
        _, m0, m1 = self.rows[s]
        return (m1 - m0 + WG_POS - 1) // WG_POS


def dense_splits(Ms: Sequence[int], cus: int) -> WgradSplits:
    """``dense_splits`` of csrc/conv.hip: as many splits as fit one round of the chip at nine taps each (cus / 9, at least one per
    problem), every split ``tps`` K-tiles of 64 positions; split s of a problem covers positions s * tps * 64 .. of it."""
    P = len(Ms)
    assert 1 <= P <= MAX_PROBLEMS
    budget = max(cus // 9, P)
    kt = [(M + WG_POS - 1) // WG_POS for M in Ms]
    tps = max(1, (sum(kt) + budget - 1) // budget)
    while sum((k + tps - 1) // tps for k in kt) > budget:
        tps += 1
    beg, rows = [0], []
    for p, M in enumerate(Ms):
        n = (kt[p] + tps - 1) // tps
        beg.append(beg[-1] + n)
        rows += [(p, s * tps * WG_POS, min((s + 1) * tps * WG_POS, M)) for s in range(n)]
    return WgradSplits(budget, tps, beg, rows)


# ---- integer operands ----------------------------------------------------------------------------------------------------------------

Y_CAP = 256             # |y| that bf16 holds exactly (8 significant bits); the same cap for fp16 so that one input set serves both
STATS_CAP = 128         # |y| of the statistics cases: a 256-row tile's sum of y^2 is then <= 2^22, exact in fp32 in any order


def forward_weights(Cout: int, Cin: int, seed: int = 0) -> np.ndarray:
    """w [Cout][3][3][Cin] float32: per output channel o and tap t ONE +-1 per 64-channel chunk, at channel (7 o + 5 t + 3 chunk) mod 64
    of the chunk -- every (tap, chunk) K-tile contributes to every output, and over the output channels every channel lane is used."""
    rng = np.random.default_rng(5000 + seed)
    w = np.zeros((Cout, 9, Cin), np.float32)
    sign = rng.choice(np.array([-1.0, 1.0], np.float32), size=(Cout, 9, Cin // CONV_BK))
    for chunk in range(Cin // CONV_BK):
        for t in range(9):
            o = np.arange(Cout)
            w[o, t, chunk * CONV_BK + (7 * o + 5 * t + 3 * chunk) % CONV_BK] = sign[:, t, chunk]
    return w.reshape(Cout, 3, 3, Cin)


def forward_operands(N: int, H: int, W: int, Cin: int, Cout: int, seed: int = 0):
    """(x [N][H][W][Cin] integers in [-3, 3], w of ``forward_weights``, integer bias [Cout]) as float32: |conv| <= 27 Cin / 64 by
    construction (216 at Cin = 512) and |bias| <= 40, so |conv + bias| <= 256.  With Cin <= 64 a bias below -27 empties its whole
    column under the ReLU."""
    rng = np.random.default_rng(4000 + seed)
    x = rng.integers(-3, 4, size=(N, H, W, Cin)).astype(np.float32)
    bias = rng.integers(-40, 41, size=Cout).astype(np.float32)
    bias[:4] = (-40, 40, -28, 0)
    return x, forward_weights(Cout, Cin, seed), bias


def dgrad_operands(N: int, H: int, W: int, Cin: int, Cout: int, seed: int = 0):
    """(g [N][H][W][Cout] integers in [-3, 3], w [Cout][3][3][Cin] of ``forward_weights``, its flipped form [Cin][3][3][Cout]): 7 is a unit
    mod 64, so the flipped weights hold one +-1 per (input channel, tap, chunk of 64 output channels) as well: |dx| <= 27 Cout / 64."""
    rng = np.random.default_rng(4500 + seed)
    g = rng.integers(-3, 4, size=(N, H, W, Cout)).astype(np.float32)
    w = forward_weights(Cout, Cin, seed)
    return g, w, dgrad_weights(w)


def _exact_in_16_bits(a: np.ndarray) -> bool:
    "Integers of at most 8 significant bits (bf16) inside the fp16 range: exact in both element types."
    a = np.asarray(a, np.float64)
    if not np.array_equal(a, np.round(a)) or float(np.abs(a).max(initial=0.0)) > 65504:
        return False
    m, _ = np.frexp(a)
    return bool(np.array_equal(m * 256, np.round(m * 256)))


def assert_forward_exact(x: np.ndarray, w: np.ndarray, bias: Optional[np.ndarray], y: np.ndarray, yb: Optional[np.ndarray], cap: int = Y_CAP) -> None:
    "What lets the GPU test ask for equality.  y: the reference without bias, yb: with bias, before the ReLU.  A condition, never a clip."
    xd, wd = np.asarray(x, np.float64), np.asarray(w, np.float64)
    assert np.array_equal(xd, np.round(xd)) and float(np.abs(xd).max()) <= 3
    assert bool(((wd == 0) | (np.abs(wd) == 1)).all())
    Cout, Cin = wd.shape[0], wd.shape[3]
    assert int((wd != 0).reshape(Cout, 9, Cin // CONV_BK, CONV_BK).sum(3).max()) <= 1, "more than one weight per (output channel, tap, chunk)"
    for t in (y,) if yb is None else (y, yb):
        assert float(np.abs(t).max()) <= cap, float(np.abs(t).max())
        assert _exact_in_16_bits(t)
    if bias is not None:
        assert np.array_equal(bias, np.round(bias))


def wgrad_density(M: int) -> float:
    "Share of non-zero elements of g and x: a sum of M products of two such draws has a standard deviation of at most 40."
    return min(0.5, 8.0 / np.sqrt(M))


def wgrad_operands(N: int, H: int, W: int, Cout: int, Cin: int, integer: bool = True, seed: int = 0):
    "(g [N][H][W][Cout], x [N][H][W][Cin]) float32: integers in [-3, 3], ``wgrad_density`` of them non-zero; or N(0, 1)."
    rng = np.random.default_rng(6000 + seed)
    d = wgrad_density(N * H * W)

    def draw(shape):
        if not integer:
            return rng.standard_normal(shape, dtype=np.float32)
        return (rng.integers(-3, 4, size=shape) * (rng.random(shape, dtype=np.float32) < d)).astype(np.float32)

    return draw((N, H, W, Cout)), draw((N, H, W, Cin))


def assert_wgrad_exact(g: np.ndarray, x: np.ndarray, ref: np.ndarray, abs_sum: np.ndarray) -> None:
    "Integer operands, every partial sum of every split below 2^24 (bounded by the sum of magnitudes), dW exact in both element types."
    for t in (g, x):
        td = np.asarray(t, np.float64)
        assert np.array_equal(td, np.round(td)) and float(np.abs(td).max()) <= 3
    assert float(abs_sum.max()) < 2 ** 24, float(abs_sum.max())
    assert float(np.abs(ref).max()) <= Y_CAP, float(np.abs(ref).max())
    assert _exact_in_16_bits(ref)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------

class FCase(NamedTuple):
    name: str
    N: int
    hw: Tuple[Tuple[int, int], ...]     # one (h, w) per problem
    Cin: int
    Cout: int

    @property
    def Ms(self) -> List[int]:
        return [self.N * h * w for h, w in self.hw]


# MODE_DENSE forward (rn_conv3x3_dense_batched_act); each runs plain, with bias, and with bias + ReLU
FCASES = [
    FCase("p4_m1_255_256_4",   1, ((1, 1), (1, 255), (256, 1), (2, 2)), 64, 256),     # every degenerate geometry; 1, 255, 256 positions
    FCase("p3_m257_513_4",     1, ((1, 257), (19, 27), (2, 2)), 128, 512),            # 257 and 513: a last tile of one position
    FCase("p2_n3_straddle",    3, ((9, 30), (5, 17)), 512, 256),                      # 810 = 3 x 270: tiles 1, 2 and 3 hold two images; 255
    FCase("p1_n3_m513_c512",   3, ((9, 19),), 512, 512),                              # 513 = 3 x 171
    FCase("p1_m256_c64",       1, ((16, 16),), 64, 256),                              # exactly one full tile, one chunk
]

# data gradient: the same launch on g [N][h][w][Cout] with the flipped weights [Cin][3][3][Cout] (Cin of the convolution % 256 == 0)
DCASES = [
    FCase("d_n3_straddle_64_256", 3, ((9, 30),), 256, 64),                           # Cin / Cout of the CONVOLUTION: 256 -> 64
    FCase("d_m513_512_512",       1, ((19, 27),), 512, 512),
    FCase("d_p2_1xw_2x2",         1, ((1, 257), (2, 2)), 256, 128),
]


class BCase(NamedTuple):
    name: str
    N: int
    H: int
    W: int
    Cin: int
    Cout: int

    @property
    def M(self) -> int:
        return self.N * self.H * self.W


# band kernel (rn_conv3x3_dense_band)
BCASES = [
    BCase("m1",            1, 1, 1, 64, 128),        # NB = 3: the tap buffers never wrap, the band buffers once
    BCase("m255_1xw",      1, 1, 255, 128, 128),
    BCase("m256_w256",     1, 1, 256, 192, 256),     # an odd chunk count: band parity flips at the chunk boundary
    BCase("m257_w257",     1, 1, 257, 64, 384),      # a row longer than a band
    BCase("m258_h2",       1, 2, 129, 128, 128),
    BCase("m259",          1, 1, 259, 192, 128),
    BCase("m515_c512",     1, 1, 515, 512, 128),
    BCase("m512_w256_h2",  1, 2, 256, 64, 128),      # +-W lands exactly one tile away
    BCase("n3_w300_h2",    3, 2, 300, 128, 256),     # a row longer than a band: +-W lands in other tiles
    BCase("n3_w257_h2",    3, 2, 257, 512, 128),
    BCase("n3_w2_h2",      3, 2, 2, 64, 128),
    BCase("n3_w3_h1",      3, 1, 3, 192, 128),
    BCase("n3_w1_h2",      3, 2, 1, 128, 128),
    BCase("n3_9x30",       3, 9, 30, 128, 128),      # 810: tiles straddle images, ragged last tile
]

# band kernel with statistics (rn_conv3x3_dense_band_stats): a ragged last tile, tiles that straddle images, two column tiles
SCASES = [
    BCase("s_n3_9x30",     3, 9, 30, 128, 128),
    BCase("s_n2_w257_h2",  2, 2, 257, 64, 256),
    BCase("s_m1",          1, 1, 1, 64, 128),
]

# the real-valued pass: one mid-size shape per entry point
REAL_DENSE = FCase("real_dense", 2, ((13, 21), (7, 11)), 128, 256)
REAL_DGRAD = FCase("real_dgrad", 2, ((13, 21),), 256, 128)
REAL_BAND = BCase("real_band", 2, 13, 21, 128, 128)
REAL_SPLITK = BCase("real_splitk", 2, 13, 21, 192, 256)
REAL_WGRAD = (2, ((13, 21), (7, 11), (5, 9)))


def splitk_shape(S: int, Cout: int, cus: int) -> Tuple[int, int, int]:
    "(N, H, W) at which rn_conv3x3_dense_splitk cuts K into S ranges on a part with ``cus`` CUs: S = 3 three ragged tiles, S = 2 about 0.4 cus tiles."
    if S == 3:
        return 1, 7, 109                            # 763 positions: three row tiles, the last of 251
    t = (2 * cus) // 5 // (Cout // CONV_BN)
    return 2, 2 * t, 63                             # 252 t positions: t row tiles or one fewer, ragged, rows of 63


WKINDS = ["p1_m1", "p1_m63_1xw", "p1_m64_hx1", "p1_m65", "p1_m127_1xw", "p1_n3_m195", "p3_tps3_tails", "p3_tps3_small", "p3_tps3_64_65"]


def wgrad_case_shapes(kind: str, cus: int) -> Tuple[int, List[Tuple[int, int]]]:
    """(N, [(h, w) per problem]) of a weight-gradient case.  The P = 3 cases reach ``tps`` = 3 with a filler problem whose height is searched
    so that ``dense_splits`` gives exactly that; the other two problems are sized from it."""
    T = 3
    table = {
        "p1_m1": (1, [(1, 1)]), "p1_m63_1xw": (1, [(1, 63)]), "p1_m64_hx1": (1, [(64, 1)]), "p1_m65": (1, [(5, 13)]),
        "p1_m127_1xw": (1, [(1, 127)]),                                               # 64 (2 tps) - 1 at tps = 1
        "p1_n3_m195": (3, [(5, 13)]),                                                 # 64 tps + 3 at tps = 1, three images
    }
    if kind in table:
        return table[kind]
    small = {"p3_tps3_tails": [(1, 64 * T + 1), (64 * 2 * T - 1, 1)],                 # last split: one tile of one position / a nearly full one
             "p3_tps3_small": [(1, 1), (7, 9)],                                      # 1 and 63 positions next to a deep walk
             "p3_tps3_64_65": [(64, 1), (5, 13)]}[kind]
    for h in range(1, 4096):
        hw = small + [(h, 31)]
        if dense_splits([a * b for a, b in hw], cus).tps == T:
            return 1, hw
    raise AssertionError(f"{kind}: no filler height gives tps = {T} on {cus} CUs")
