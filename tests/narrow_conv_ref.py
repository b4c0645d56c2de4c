"""Float64 references, schedule restatements, integer operands and the shapes of the tests of the two narrow 3x3 kernels --
``wgrad3x3_kernel`` (csrc/wgrad3x3.hip) and ``conv3x3_narrow64_kernel`` (csrc/narrow3x3.hip) -- shared by ``test_narrow_conv_ref.py``
(CPU: the references against torch's float64 convolution and its autograd, the restatements, the generators' promises) and
``test_narrow_conv_gpu.py``.

    dW[o][kh][kw][c] = sum over (n, h, w) of g[n][h][w][o] * x[n][h + kh - 1][w + kw - 1][c]
    y[n][h][w][o]    = sum over (kh, kw, c) of x[n][h + kh - 1][w + kw - 1][c] * w[o][kh][kw][c]

Both references are index arithmetic (a zero-padded shift per tap) and one float64 matmul per tap on the 16-bit operand VALUES -- no
torch convolution, no MIOpen -- so whatever separates them from a kernel is the kernel's.  They run on whatever device the operands
are on: float64 products and sums of small integers are exact in any order, on any device.

``wgrad_schedule`` / ``band_schedule`` restate which tiles a team of ``wgrad3x3_kernel`` and which rows a workgroup of
``conv3x3_narrow64_kernel`` walks.  The depth of both walks follows the CU count of the part, so the shapes of the GPU cases are
derived at run time (``wgrad_shape``, ``forward_images``) from what the library reports and every case asserts what it reached; the
"256 CUs" figures in the case tables are documentation.

numpy's PCG64 draws the operands (as tests/synth.py does), so the CPU test sees the bytes the GPU test runs.
"""
from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch

W3_PX = 64              # output pixels of a wgrad3x3 tile (two 32-pixel k-steps)
W3_OUT = 64 * 9 * 64    # floats of one workgroup's partial [n][tap][c]
N3_TW = 128             # output pixels of a strip of the forward kernel


# ---- float64 references ------------------------------------------------------------------------------------------------------

def shifted_taps(x: torch.Tensor) -> torch.Tensor:
    "x [N][H][W][C] -> float64 [N * H * W][9][C]: under tap (kh, kw) pixel (h, w) sees x[h + kh - 1][w + kw - 1], zero outside the image."
    N, H, W, Cc = x.shape
    xp = torch.zeros((N, H + 2, W + 2, Cc), dtype=torch.float64, device=x.device)
    xp[:, 1:H + 1, 1:W + 1] = x.double()
    return torch.stack([xp[:, kh:kh + H, kw:kw + W] for kh in range(3) for kw in range(3)], dim=3).reshape(N * H * W, 9, Cc)


def wgrad_ref(g: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    "float64 dW [Cout][9][Cin] from g [N][H][W][Cout] and x [N][H][W][Cin] (any float type: the values as they are), one image at a time."
    N, H, W, Cn = g.shape
    out = torch.zeros((Cn, 9, x.shape[3]), dtype=torch.float64, device=g.device)
    for i in range(N):
        xt = shifted_taps(x[i:i + 1])
        out += (g[i].double().reshape(H * W, Cn).t() @ xt.reshape(H * W, -1)).view_as(out)
    return out


def abs_terms_sum(g: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    "sum over pixels of |g * x| per element of dW, with the reference's own gather."
    return wgrad_ref(g.double().abs(), x.double().abs())


def forward_ref(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, relu: bool = False) -> torch.Tensor:
    "float64 y [N][H][W][Cout] from x [N][H][W][C] and w [Cout][3][3][C]; with ``bias``: act(conv + bias)."
    N, H, W, Cc = x.shape
    xp = torch.zeros((N, H + 2, W + 2, Cc), dtype=torch.float64, device=x.device)
    xp[:, 1:H + 1, 1:W + 1] = x.double()
    wd = w.double()
    y = torch.zeros((N * H * W, w.shape[0]), dtype=torch.float64, device=x.device)
    for kh in range(3):
        for kw in range(3):
            y += xp[:, kh:kh + H, kw:kw + W].reshape(N * H * W, Cc) @ wd[:, kh, kw, :].t()
    if bias is not None:
        y = y + bias.double()[None, :]
        if relu:
            y = torch.clamp(y, min=0)
    return y.view(N, H, W, -1)


def sum_bound(M: int, abs_sum: torch.Tensor) -> torch.Tensor:
    "``sum_bound`` of pw_wgrad_ref.py: |fp32 sum - exact sum| <= (M - 1) 2^-24 sum |term| for any order, one rounding per addition."
    return (M - 1) * 2.0 ** -24 * abs_sum


def half_ulp(ref: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    "Half a unit in the last place of ``dtype`` at |ref| (float64)."
    p, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    _, e = torch.frexp(ref.abs())
    e = torch.where(ref == 0, torch.full_like(e, -2000), e)
    return torch.ldexp(torch.ones_like(ref), torch.clamp(e - 1, min=emin) - p - 1)


# ---- wgrad3x3_kernel: who walks which tile -------------------------------------------------------------------------------------

class WgradSchedule(NamedTuple):
    N: int
    H: int
    W: int
    subs: int
    subs_c: int
    wgs_per_sub: int
    tiles_x: int
    tiles: int
    tiles_per_team: int
    tile_map: List[Tuple[int, int, int, int]]                   # tile -> (image, row, x0, ksteps)
    ranges: List[Tuple[Tuple[int, int], Tuple[int, int]]]       # workgroup sub * wgs_per_sub + wsub -> ((t_beg, t_end) of team 0, of team 1)

    def block(self, wg: int) -> Tuple[int, int]:
        "(n0, c0): the 64 x 64 block of dW workgroup ``wg`` adds to."
        sub = wg // self.wgs_per_sub
        return (sub // self.subs_c) * 64, (sub % self.subs_c) * 64

    def pixel_start(self, t: int) -> int:
        "Index of tile t's first pixel in [N * H * W] (t == tiles: one past the last pixel)."
        if t >= self.tiles:
            return self.N * self.H * self.W
        b, y, x0, _ = self.tile_map[t]
        return (b * self.H + y) * self.W + x0

    def team_sizes(self) -> List[int]:
        "Tiles of team 2 * wsub + team, in team order (the sub-problems all walk the same tiles)."
        return [e - b for r in self.ranges[:self.wgs_per_sub] for (b, e) in r]

    def describe(self) -> str:
        s = self.team_sizes()
        working = sum(1 for v in s if v)
        return (f"tiles {self.tiles} ({self.tiles_x} per row) tiles_per_team {self.tiles_per_team} teams {len(s)} working {working} "
                f"last working team {s[working - 1] if working else 0} tiles")


def wgrad_schedule(N: int, H: int, W: int, Cout: int, Cin: int, wgs_per_sub: int) -> WgradSchedule:
    "rn_conv3x3_wgrad_narrow's host arithmetic and the kernel's t_beg / t_end / stage() / compute() index arithmetic."
    subs_c = Cin // 64
    subs = (Cout // 64) * subs_c
    tiles_x = (W + W3_PX - 1) // W3_PX
    tiles = N * H * tiles_x
    tpt = (tiles + 2 * wgs_per_sub - 1) // (2 * wgs_per_sub)
    tile_map = []
    for t in range(tiles):
        tx, rowid = t % tiles_x, t // tiles_x
        x0 = tx * W3_PX
        tile_map.append((rowid // H, rowid % H, x0, 2 if x0 + 32 < W else 1))
    ranges = []
    for wg in range(subs * wgs_per_sub):
        wsub = wg % wgs_per_sub
        r = []
        for team in range(2):
            t_beg = min((2 * wsub + team) * tpt, tiles)
            r.append((t_beg, min(t_beg + tpt, tiles)))
        ranges.append((r[0], r[1]))
    return WgradSchedule(N, H, W, subs, subs_c, wgs_per_sub, tiles_x, tiles, tpt, tile_map, ranges)


def wgrad_partials_ref(g: torch.Tensor, x: torch.Tensor, s: WgradSchedule) -> torch.Tensor:
    """float64 [workgroups][64][9][64]: the reference restricted to each workgroup's own tiles and (n0, c0) block.  The tiles of a
    workgroup's two teams are consecutive, and consecutive tiles are consecutive pixels of [N * H * W]."""
    N, H, W, Cn = g.shape
    Cc = x.shape[3]
    gd, xt = g.double().reshape(N * H * W, Cn), shifted_taps(x).reshape(N * H * W, 9 * Cc)
    out = torch.zeros((s.subs * s.wgs_per_sub, 64, 9, 64), dtype=torch.float64, device=g.device)
    for wsub in range(s.wgs_per_sub):
        (b0, e0), (b1, e1) = s.ranges[wsub]
        assert e0 == b1 or b1 == e1
        p0, p1 = s.pixel_start(b0), s.pixel_start(max(e0, e1))
        if p0 >= p1:
            continue
        full = (gd[p0:p1].t() @ xt[p0:p1]).view(Cn // 64, 64, 9, s.subs_c, 64)        # [n block][n][tap][c block][c]
        out[wsub::s.wgs_per_sub] = full.permute(0, 3, 1, 2, 4).reshape(s.subs, 64, 9, 64)
    return out


def total_from_partials(partials: torch.Tensor, s: WgradSchedule, Cout: int, Cin: int) -> torch.Tensor:
    "[workgroups][64][9][64] -> [Cout][9][Cin]: every sub-problem's workgroups summed into its block."
    per_sub = partials.view(s.subs, s.wgs_per_sub, 64, 9, 64).sum(1)
    return per_sub.view(Cout // 64, s.subs_c, 64, 9, 64).permute(0, 2, 3, 1, 4).reshape(Cout, 9, Cin)


def reduce_ref(partials_f32: torch.Tensor, s: WgradSchedule, Cout: int, Cin: int, dtype: torch.dtype) -> torch.Tensor:
    """The order of wgrad3x3_reduce_kernel on f32 partials: slice l = 0..7 adds workgroups l, l + 8, ... of the sub-problem in sequence,
    starting from zero; the eight sums are added 0..7; one rounding to the element type.  [Cout][9][Cin]."""
    p = partials_f32.view(s.subs, s.wgs_per_sub, 64, 9, 64)
    sums = []
    for l in range(8):
        acc = torch.zeros_like(p[:, 0])
        for w in range(l, s.wgs_per_sub, 8):
            acc = acc + p[:, w]
        sums.append(acc)
    t = sums[0]
    for l in range(1, 8):
        t = t + sums[l]
    return t.view(Cout // 64, s.subs_c, 64, 9, 64).permute(0, 2, 3, 1, 4).reshape(Cout, 9, Cin).to(dtype)


# ---- conv3x3_narrow64_kernel: who walks which row ------------------------------------------------------------------------------

class BandSchedule(NamedTuple):
    strips: int
    bands: int
    rows_per_band: int
    band_rows: List[Tuple[int, int]]        # band -> (y0, y1), the same in every strip of every image
    last_strip_pixels: int

    @property
    def last_band_rows(self) -> int:
        y0, y1 = self.band_rows[-1]
        return y1 - y0


def band_schedule(N: int, H: int, W: int, rows_per_band: int) -> BandSchedule:
    "rn_conv3x3_narrow_forward's band count from rows_per_band and the kernel's y0 / y1."
    strips = (W + N3_TW - 1) // N3_TW
    bands = (H + rows_per_band - 1) // rows_per_band
    rows = [(b * rows_per_band, min((b + 1) * rows_per_band, H)) for b in range(bands)]
    return BandSchedule(strips, bands, rows_per_band, rows, W - (strips - 1) * N3_TW)


def store_counts(W: int) -> List[int]:
    "Per strip and pixel half: the 16-pixel half tiles that start inside the image = the kernel's vmcnt(stores), in launch order."
    out = []
    for strip in range((W + N3_TW - 1) // N3_TW):
        for pw in range(2):
            xb = strip * N3_TW + pw * 64
            out.append(sum(1 for k in range(4) if xb + 16 * k < W))
    return out


# ---- integer operands ----------------------------------------------------------------------------------------------------------

def _t(a: np.ndarray, dtype: torch.dtype) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def wgrad_operands(N: int, H: int, W: int, Cout: int, Cin: int, dtype: torch.dtype, integer: bool, seed: int = 0):
    """(g [N][H][W][Cout], x [N][H][W][Cin]) on the CPU.  integer: values in [-3, 3], about two in three of them zero, so every sum of
    |g| |x| over any set of pixels stays below 2^24 (fp32 accumulation exact in any order, in the kernel and in the reduction over the
    workgroups) and dW inside the fp16 range: ``assert_wgrad_exactness`` checks both on the reference.  Otherwise N(0, 1)."""
    rng = np.random.default_rng(2000 + seed)

    def draw(shape):
        if not integer:
            return rng.standard_normal(shape, dtype=np.float32)
        return (rng.integers(-3, 4, size=shape) * (rng.random(shape, dtype=np.float32) < 0.4)).astype(np.float32)

    return _t(draw((N, H, W, Cout)), dtype), _t(draw((N, H, W, Cin)), dtype)


def assert_wgrad_exactness(g: torch.Tensor, x: torch.Tensor, ref: torch.Tensor, abs_sum: torch.Tensor) -> None:
    "What lets the GPU test ask for equality: integer operands exact in both 16-bit types, every partial sum below 2^24, dW inside fp16."
    for t in (g, x):
        td = t.double()
        assert torch.equal(td, td.round()) and float(td.abs().max()) <= 3
        assert torch.equal(td.to(torch.bfloat16).double(), td) and torch.equal(td.to(torch.float16).double(), td)
    assert torch.equal(ref, ref.round())
    assert float(abs_sum.max()) < 2 ** 24, float(abs_sum.max())         # bounds every partial sum of every workgroup, and their sum
    assert float(ref.abs().max()) <= 65504, float(ref.abs().max())


def forward_operands(N: int, H: int, W: int, dtype: torch.dtype, seed: int = 0):
    """(x [N][H][W][64] in [-2, 2], w [64][3][3][64] with at most 64 non-zero +-1 per output channel, integer bias f32 [64] in [-128, 128])
    on the CPU: every output is an integer with |y| <= 128 and |y + b| <= 256, exact in bf16 and fp16 and in fp32 at every step."""
    rng = np.random.default_rng(3000 + seed)
    x = rng.integers(-2, 3, size=(N, H, W, 64)).astype(np.float32)
    w = np.zeros((64, 576), np.float32)
    for o in range(64):
        k = int(rng.integers(40, 65))
        w[o, rng.choice(576, size=k, replace=False)] = rng.choice(np.array([-1.0, 1.0], np.float32), size=k)
    bias = rng.integers(-128, 129, size=64).astype(np.float32)
    return _t(x, dtype), _t(w.reshape(64, 3, 3, 64), dtype), _t(bias, torch.float32)


def assert_forward_exactness(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, y: torch.Tensor, yb: torch.Tensor) -> None:
    "y: the reference without bias, yb: with bias (before the ReLU)."
    xd, wd = x.double(), w.double()
    assert torch.equal(xd, xd.round()) and float(xd.abs().max()) <= 2
    assert bool(((wd == 0) | (wd.abs() == 1)).all()) and int((wd != 0).reshape(64, -1).sum(1).max()) <= 64
    assert torch.equal(bias.double(), bias.double().round())
    for t, peak in ((y, 128), (yb, 256)):
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= peak
        assert torch.equal(t.to(torch.bfloat16).double(), t) and torch.equal(t.to(torch.float16).double(), t)


# ---- the weight-gradient cases ---------------------------------------------------------------------------------------------------

class WCase(NamedTuple):
    name: str
    Cout: int
    Cin: int
    W: int
    H: int                      # 0: one image, H = the tile count the case asks for (W <= 64)
    depth: int                  # tiles_per_team the case exists for
    exact_depth: bool           # == depth (else >= depth)
    full: bool                  # every team holds exactly ``depth`` tiles
    last: Optional[int]         # tiles of the last working team (ragged tail), with ...
    odd_working: Optional[bool]     # ... an odd number of working teams: some workgroup has team 0 working and team 1 idle
    mixed: bool                 # one-k-step and two-k-step tiles inside one team's walk
    straddle: bool              # some team's tiles lie in two images
    real: bool                  # also run with N(0, 1) operands against the summation bound
    wrapper: bool               # also run through biasact.conv3x3_wgrad_narrow


#       name               Cout Cin  W   H  depth exact full   last  odd    mixed  strad  real   wrapper       (teams at 256 CUs: 512 / 256 / 8)
WCASES = [
    WCase("c64_full2",      64,  64, 52, 0, 2, True, True,  None, None,  False, False, False, False),    # no refill: the prologue's two stages are all
    WCase("r64x128_full2",  64, 128, 33, 0, 2, True, True,  None, None,  False, False, False, False),
    WCase("c512_full2",    512, 512, 40, 0, 2, True, True,  None, None,  False, False, False, False),
    WCase("c64_d3_w96",     64,  64, 96, 5, 3, True, False, None, None,  True,  True,  True,  True),     # first refill of team 0, the i > 0 refill of team 1
    WCase("r128x64_d3_w97", 128, 64, 97, 7, 3, True, False, None, None,  False, True,  False, False),
    WCase("c512_d3_w70",   512, 512, 70, 5, 3, True, False, None, None,  True,  True,  True,  False),
    WCase("c64_d4_w33",     64,  64, 33, 7, 4, True, False, None, None,  False, True,  False, False),    # both buffer parities of the refill
    WCase("c512_d4_w64",   512, 512, 64, 3, 4, True, False, None, None,  False, True,  False, False),
    WCase("r128x64_d5_w64", 128, 64, 64, 3, 5, True, False, None, None,  False, True,  False, False),
    WCase("c512_d5_w96",   512, 512, 96, 3, 5, True, False, None, None,  True,  True,  True,  False),
    WCase("r64x128_d8_w33", 64, 128, 33, 7, 8, False, False, None, None, False, True,  True,  False),    # steady state
    WCase("c512_d9_w97",   512, 512, 97, 3, 9, False, False, None, None, False, True,  True,  False),
    WCase("c64_d3_w1",      64,  64,  1, 7, 3, True, False, None, None,  False, True,  False, False),    # one-pixel rows: every horizontal tap but the centre leaves the image
    # ragged tails (one image, H = tiles): the last working team holds 1 / 2 tiles, whole teams hold none
    WCase("c64_tail1",      64,  64, 33, 0, 3, True, False, 1,    True,  False, False, False, False),
    WCase("c64_tail2",      64,  64, 64, 0, 3, True, False, 2,    False, False, False, False, False),
    WCase("c512_tail1_w1", 512, 512,  1, 0, 3, True, False, 1,    True,  False, False, False, False),
    WCase("c512_tail2",    512, 512, 33, 0, 3, True, False, 2,    False, False, False, False, True),
    WCase("r128x64_tail2_d5", 128, 64, 40, 0, 5, True, False, 2,  True,  False, False, False, False),
]


def tiles_for_tail(teams: int, depth: int, last: int, odd_working: bool) -> Optional[int]:
    "Fewest tiles that give tiles_per_team == depth, ``last`` tiles in the last working team and the asked parity of working teams."
    for working in range(1, teams):                         # (< teams: at least one whole team holds none)
        tiles = (working - 1) * depth + last
        if (tiles + teams - 1) // teams == depth and (working % 2 == 1) == odd_working:
            return tiles
    return None


def wgrad_shape(case: WCase, wgs_per_sub: int) -> Tuple[int, int, int]:
    "(N, H, W) at which ``case`` reaches its depth when a sub-problem has ``wgs_per_sub`` workgroups."
    teams, tx = 2 * wgs_per_sub, (case.W + W3_PX - 1) // W3_PX
    if case.last is not None:
        tiles = tiles_for_tail(teams, case.depth, case.last, case.odd_working)
        assert tiles is not None and tx == 1, f"{case.name}: no tile count gives this tail on {teams} teams"
        return 1, tiles, case.W
    if case.full:
        assert tx == 1
        return 1, teams * case.depth, case.W
    per_image = case.H * tx
    N = ((case.depth - 1) * teams + per_image) // per_image           # fewest images with more than (depth - 1) * teams tiles
    return N, case.H, case.W


def check_wgrad_case(case: WCase, s: WgradSchedule) -> None:
    "Hard failure, not a skip: a change of the host's tile arithmetic must not quietly turn these into depth-1 tests."
    why = (f"{case.name}: the library now runs {s.describe()} -- the tile arithmetic of csrc/wgrad3x3.hip or the CU count changed and this "
           f"shape no longer covers what it is here for; choose a new shape in tests/narrow_conv_ref.py (WCASES)")
    sizes = s.team_sizes()
    working = sum(1 for v in sizes if v)
    assert sum(sizes) == s.tiles and all(v for v in sizes[:working]) and not any(sizes[working:]), why
    assert (s.tiles_per_team == case.depth) if case.exact_depth else (s.tiles_per_team >= case.depth), why
    assert max(sizes) == s.tiles_per_team, why
    if case.full:
        assert all(v == s.tiles_per_team for v in sizes), why
    if case.last is not None:
        assert sizes[working - 1] == case.last < s.tiles_per_team and working < len(sizes), why
        assert (working % 2 == 1) == case.odd_working, why
    teams = [r for pair in s.ranges[:s.wgs_per_sub] for r in pair]
    if case.mixed:
        assert any({s.tile_map[t][3] for t in range(b, e)} == {1, 2} for b, e in teams), why
    if case.straddle:
        assert s.N >= 2 and s.H % 2 == 1 and any(e > b and s.tile_map[b][0] != s.tile_map[e - 1][0] for b, e in teams), why


# ---- the forward cases ---------------------------------------------------------------------------------------------------------

class FCase(NamedTuple):
    name: str
    H: int
    W: int
    rows: int                   # rows_per_band the case exists for (== H: a single band per strip)
    bands: int
    last_rows: int              # rows of the last band
    strips: int
    last_pixels: int            # pixels of the last strip
    probe: bool                 # the tap probe runs here (the deepest walks)


#       name             H    W  rows bands last strips px          N at 256 CUs (the smallest that reaches ``rows``)
FCASES = [
    FCase("r3_w129",      7, 129,  3, 3, 1, 2,  1, False),          # 65: the ring before its first wrap; a last band of one row
    FCase("r4_w130",     11, 130,  4, 3, 3, 2,  2, False),          # 65: at the wrap; last band rows - 1
    FCase("r5_w137",     10, 137,  5, 2, 5, 2,  9, False),          # 86: after the wrap
    FCase("r6_w144",     16, 144,  6, 3, 4, 2, 16, False),          # 65
    FCase("r5_w176",     13, 176,  5, 3, 3, 2, 48, False),          # 65
    FCase("r10_w145",    19, 145, 10, 2, 9, 2, 17, True),           # 86: a second wrap; last band rows - 1
    FCase("r3_w258",      7, 258,  3, 3, 1, 3,  2, False),          # 43: three strips
    FCase("one_band_w33", 12, 33, 12, 1, 12, 1, 33, True),          # 257: rows_per_band == H, the longest walk
    FCase("r4_w40",       13, 40,  4, 4, 1, 1, 40, False),          # 103: one strip, W <= 40; four bands, the last of one row
]


def forward_images(case: FCase, rows_per_band_of) -> Optional[int]:
    "The fewest images at which the library walks ``case.rows`` rows per band (``rows_per_band_of(N, H, W)``: the library's export)."
    for N in range(1, 4097):
        r = rows_per_band_of(N, case.H, case.W)
        if r == case.rows:
            return N
        if r > case.rows:
            return None
    return None


def check_forward_case(case: FCase, N: Optional[int], rows_per_band: int) -> BandSchedule:
    why = (f"{case.name}: the library now walks {rows_per_band} rows per band at N = {N} -- the band arithmetic of csrc/narrow3x3.hip or the "
           f"CU count changed and this shape no longer covers what it is here for; choose a new shape in tests/narrow_conv_ref.py (FCASES)")
    assert N is not None and rows_per_band == case.rows, why
    s = band_schedule(N, case.H, case.W, rows_per_band)
    assert (s.bands, s.last_band_rows, s.strips, s.last_strip_pixels) == (case.bands, case.last_rows, case.strips, case.last_pixels), why
    return s
