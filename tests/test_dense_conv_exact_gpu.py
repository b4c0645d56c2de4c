"""GPU: the dense 3x3 MFMA family of csrc/conv.hip -- ``rn_conv3x3_dense_batched[_act]`` (forward and, with the flipped weights, data
gradient), ``rn_conv3x3_dense_band[_stats]``, ``rn_conv3x3_dense_splitk`` and ``rn_conv3x3_dense_wgrad_batched`` -- against the float64
references of ``dense_conv_ref.py``, in bf16 and fp16.

Integer operands: every product and every partial sum is an integer below 2^24 and every result one the element type holds, so fp32
accumulation is exact in any order and the kernels must EQUAL the reference -- outputs, the f32 workspace of the split-K launch K range
by K range, the f32 partials of the weight gradient split by split, the statistics partials tile by tile.  A dropped or doubled product,
a tap bit wrong on one row, a band read one parity late or a K range that loses a tile changes an integer.  N(0, 1) operands: each
element within half a unit in the last place plus the order-independent summation bound.

Every buffer the kernels write is followed by a guard pattern that must come back untouched; the activations are followed by NaN rows,
so a read past the end shows in the result.  The tile, band, K-range and split counts follow the shape and the CU count: every case
first asserts, as a hard failure, that it reaches the path it is here for, and prints what it reached.
"""
import functools

import numpy as np
import pytest
import torch

import dense_conv_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "f16"]
GUARD = 4096            # bytes of pattern behind a buffer the kernels must not touch
PAD_ROWS = 320          # NaN positions behind an activation tensor: more than a band
RN_EUNSUPPORTED = -4

# Factor on the summation bound of the real-valued cases: (K - 1) 2^-24 sum |a b| holds for one rounding per addition in any order; what
# the matrix unit's adder does inside an instruction is not documented.  1: the bound as derived (test_pw_wgrad_gpu.py and
# test_narrow_conv_gpu.py take the same).  Largest measured err / (half a unit in the last place + bound) per entry point on the MI355X
# (256 CUs), bf16 / fp16; nearly all of each figure is the rounding to the element type:
#   dense_batched 0.919 / 0.578   data gradient 0.909 / 0.532   dense_band 0.882 / 0.571   dense_splitk 0.842 / 0.381   dense_wgrad 0.996 / 0.981
# and of the f32 intermediates alone, err / bound: split-K workspace 3.3e-3 / 3.3e-3, weight-gradient partials (64 positions each, where the
# bound is tightest) 7.7e-2 / 8.7e-2, dense_band_stats sum y 5.7e-4 / 5.2e-3 and sum y^2 7.2e-2 / 1.5e-1 (the ragged tile of 34 rows).
BOUND_SCALE = 1.0


def _lib():
    from pytorch_retinanet_amd._lib import lib
    return lib


def _dt(dtype):
    from pytorch_retinanet_amd._lib import RN_BF16, RN_F16
    return RN_F16 if dtype == torch.float16 else RN_BF16


def _zero():
    from pytorch_retinanet_amd._launch import zero_page
    return zero_page(torch.device(DEV))


def _ptrs(ts):
    from pytorch_retinanet_amd._launch import ptr_array
    return ptr_array(ts)


def _ints(v):
    from pytorch_retinanet_amd._launch import int_array
    return int_array(v)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _cus() -> int:
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _act(a: np.ndarray, dtype) -> torch.Tensor:
    "[N][h][w][C] values -> device [M][C] of ``dtype``, the leading slice of an allocation whose tail is NaN rows."
    C = a.shape[-1]
    t = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1, C).to(dtype)
    buf = torch.full((t.shape[0] + PAD_ROWS, C), float("nan"), dtype=dtype, device=DEV)
    buf[:t.shape[0]] = t.to(DEV)
    return buf[:t.shape[0]]


def _dev(a: np.ndarray, dtype) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV).contiguous()


def _guarded(n: int) -> torch.Tensor:
    "n 16-bit elements to be written, then GUARD bytes of pattern."
    return torch.full((n + GUARD // 2,), 0x7B7B, dtype=torch.int16, device=DEV)


def _take(buf: torch.Tensor, n: int, dtype, what: str) -> torch.Tensor:
    assert bool((buf[n:] == 0x7B7B).all()), f"{what}: written behind its end"
    return buf[:n].view(dtype)


def _f32_guarded(n: int) -> torch.Tensor:
    "n floats of NaN pattern (0xFFFFFFFF) to be written, then GUARD bytes of the same."
    return torch.full((n * 4 + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)


def _take_f32(buf: torch.Tensor, n: int, what: str) -> torch.Tensor:
    assert bool((buf[n * 4:] == 0xFF).all()), f"{what}: written behind its end"
    return buf[:n * 4].view(torch.float32)


def _np(t: torch.Tensor) -> np.ndarray:
    return t.double().cpu().numpy()


def _assert_equal(got: torch.Tensor, want: np.ndarray, what: str, row_len: int = 0):
    g = _np(got).reshape(want.shape)
    bad = ~(g == want)                                                  # (a NaN is a difference)
    if bad.any():
        idx = tuple(int(i[0]) for i in np.nonzero(bad))
        flat = np.nonzero(bad.reshape(-1, want.shape[-1]).any(1))[0]
        where = f"; flattened positions {flat[:12].tolist()} (tile, row in tile) {[(int(m) // 256, int(m) % 256) for m in flat[:6]]}" if row_len else ""
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {idx}: {g[idx]} != {want[idx]}{where}")


def _round_to(a: np.ndarray, dtype) -> np.ndarray:
    "float64 values -> the values ``dtype`` holds (round to nearest even), as float32."
    return torch.from_numpy(np.asarray(a, np.float32)).to(dtype).float().numpy()


# ---- MODE_DENSE: forward and data gradient ------------------------------------------------------------------------------------------

def _dense_launch(xs, ws, biases, relu, dtype, N, hw, Cin, Cout):
    "rn_conv3x3_dense_batched[_act] on device operands; returns the outputs [M_p][Cout]."
    lib = _lib()
    P = len(xs)
    outs = [_guarded(x.shape[0] * Cout) for x in xs]
    hs, wds = _ints([h for h, _ in hw]), _ints([w for _, w in hw])
    if biases is None and not relu:
        rc = lib.rn_conv3x3_dense_batched(_ptrs(xs), _ptrs(ws), None, _ptrs(outs), P, _dt(dtype), N, hs, wds, Cin, Cout, _zero().data_ptr(), _stream())
    else:
        rc = lib.rn_conv3x3_dense_batched_act(_ptrs(xs), _ptrs(ws), _ptrs(biases) if biases is not None else None, _ptrs(outs), P, _dt(dtype), N, hs, wds,
                                              Cin, Cout, _zero().data_ptr(), int(relu), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((_zero() == 0).all()), "the zero page was written"
    return [_take(o, x.shape[0] * Cout, dtype, f"y of problem {p}").view(x.shape[0], Cout) for p, (o, x) in enumerate(zip(outs, xs))]


@functools.lru_cache(maxsize=None)
def _forward_problem(name: str):
    "Operands and float64 references of a forward case, once for both element types."
    case = next(c for c in R.FCASES if c.name == name)
    ops = [R.forward_operands(case.N, h, w, case.Cin, case.Cout, seed=p) for p, (h, w) in enumerate(case.hw)]
    refs = []
    for x, w, bias in ops:
        y, yb = R.conv_ref(x, w), R.conv_ref(x, w, bias)
        R.assert_forward_exact(x, w, bias, y, yb)
        refs.append((y, yb, np.maximum(yb, 0.0)))
    return case, ops, refs


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", [c.name for c in R.FCASES])
def test_integer_operands_give_the_exact_dense_forward(name, dtype):
    case, ops, refs = _forward_problem(name)
    grid = R.dense_grid(case.Ms, case.Cin, case.Cout)
    assert [grid.tiles_of(p) for p in range(len(case.Ms))] == [int(_lib().rn_conv3x3_dense_band_tiles(case.N, h, w)) for h, w in case.hw]
    print(f"dense {name} {dtype}: P {len(case.Ms)} N {case.N} M {case.Ms} row tiles {grid.tile_beg} column tiles {grid.col_tiles} K-tiles {grid.ktiles} "
          f"straddling {[R.straddling_tiles(case.N, h, w) for h, w in case.hw]}")
    xs = [_act(x, dtype) for x, _, _ in ops]
    ws = [_dev(w, dtype) for _, w, _ in ops]
    bs = [_dev(b, torch.float32) for _, _, b in ops]
    for what, biases, relu, k in (("plain", None, False, 0), ("with bias", bs, False, 1), ("with bias and ReLU", bs, True, 2), ("ReLU alone", None, True, None)):
        ys = _dense_launch(xs, ws, biases, relu, dtype, case.N, case.hw, case.Cin, case.Cout)
        for p, y in enumerate(ys):
            want = refs[p][k] if k is not None else np.maximum(refs[p][0], 0.0)
            _assert_equal(y, want.reshape(-1, case.Cout), f"{what}, problem {p}", 256)
    if case.Cin == 64:          # the known subset: |conv| <= 27, so the columns with a bias below -27 are empty under the ReLU and those above 27 full
        for p, (_, _, b) in enumerate(ops):
            assert not refs[p][2][..., b < -27].any() and refs[p][2][..., b > 27].all() and int((b < -27).sum()) >= 2


@functools.lru_cache(maxsize=None)
def _dgrad_problem(name: str):
    case = next(c for c in R.DCASES if c.name == name)
    ops = [R.dgrad_operands(case.N, h, w, case.Cin, case.Cout, seed=p) for p, (h, w) in enumerate(case.hw)]
    refs = []
    for g, _, wf in ops:
        dx = R.conv_ref(g, wf)
        R.assert_forward_exact(g, wf, None, dx, None)
        refs.append(dx)
    return case, ops, refs


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", [c.name for c in R.DCASES])
def test_integer_operands_give_the_exact_data_gradient(name, dtype):
    "dx = the MODE_DENSE launch on g with the weights rn_conv3x3_dgrad_weight_batched flips (themselves equal to the flip by index)."
    case, ops, refs = _dgrad_problem(name)
    lib = _lib()
    P = len(ops)
    grid = R.dense_grid(case.Ms, case.Cout, case.Cin)                   # the launch contracts over the convolution's OUTPUT channels
    print(f"dgrad {name} {dtype}: P {P} N {case.N} M {case.Ms} row tiles {grid.tile_beg} column tiles {grid.col_tiles} K-tiles {grid.ktiles}")
    ws = [_dev(w, dtype) for _, w, _ in ops]
    flipped = [_guarded(case.Cin * 9 * case.Cout) for _ in ops]
    rc = lib.rn_conv3x3_dgrad_weight_batched(_ptrs(ws), _ptrs(flipped), P, case.Cout, case.Cin, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    wfs = [_take(f, case.Cin * 9 * case.Cout, dtype, "flipped weights") for f in flipped]
    for wf_dev, (_, _, wf) in zip(wfs, ops):
        _assert_equal(wf_dev, wf.reshape(-1, case.Cout), "flipped weights")
    gs = [_act(g, dtype) for g, _, _ in ops]
    dxs = _dense_launch(gs, wfs, None, False, dtype, case.N, case.hw, case.Cout, case.Cin)
    for p, dx in enumerate(dxs):
        _assert_equal(dx, refs[p].reshape(-1, case.Cin), f"dx of problem {p}", 256)


# ---- the band kernel ----------------------------------------------------------------------------------------------------------------

def _band_launch(x, w, dtype, c: R.BCase, stats: bool):
    lib = _lib()
    y = _guarded(c.M * c.Cout)
    tiles = int(lib.rn_conv3x3_dense_band_tiles(c.N, c.H, c.W))
    if stats:
        part = _f32_guarded(tiles * 2 * c.Cout)
        rc = lib.rn_conv3x3_dense_band_stats(x.data_ptr(), w.data_ptr(), y.data_ptr(), part.data_ptr(), _dt(dtype), c.N, c.H, c.W, c.Cin, c.Cout,
                                             _zero().data_ptr(), _stream())
    else:
        rc = lib.rn_conv3x3_dense_band(x.data_ptr(), w.data_ptr(), y.data_ptr(), _dt(dtype), c.N, c.H, c.W, c.Cin, c.Cout, _zero().data_ptr(), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((_zero() == 0).all()), "the zero page was written"
    yv = _take(y, c.M * c.Cout, dtype, "y").view(c.M, c.Cout)
    return (yv, _take_f32(part, tiles * 2 * c.Cout, "the statistics partials").view(tiles, 2, c.Cout)) if stats else yv


def _check_band_path(c: R.BCase, dtype, what: str) -> R.BandWalk:
    bw = R.band_walk(c.N, c.H, c.W, c.Cin, c.Cout)
    assert bw.tiles == int(_lib().rn_conv3x3_dense_band_tiles(c.N, c.H, c.W)) and bw.NB == 3 * c.Cin // 64 and bw.col_tiles == c.Cout // 128
    print(f"{what} {c.name} {dtype}: N {c.N} H {c.H} W {c.W} M {c.M} tiles {bw.tiles} (last {bw.last_rows} rows) column tiles {bw.col_tiles} NB {bw.NB} "
          f"straddling {R.straddling_tiles(c.N, c.H, c.W)}")
    return bw


@functools.lru_cache(maxsize=None)
def _band_problem(name: str):
    c = next(c for c in R.BCASES + R.SCASES if c.name == name)
    x, w, _ = R.forward_operands(c.N, c.H, c.W, c.Cin, c.Cout)
    y = R.conv_ref(x, w)
    R.assert_forward_exact(x, w, None, y, None, cap=R.STATS_CAP if c in R.SCASES else R.Y_CAP)
    return c, x, w, y


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", [c.name for c in R.BCASES])
def test_integer_operands_give_the_exact_band_convolution(name, dtype):
    c, x, w, y = _band_problem(name)
    _check_band_path(c, dtype, "band")
    got = _band_launch(_act(x, dtype), _dev(w, dtype), dtype, c, False)
    _assert_equal(got, y.reshape(c.M, c.Cout), "y", 256)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", [c.name for c in R.SCASES])
def test_integer_operands_give_exact_statistics_partials_tile_by_tile(name, dtype):
    c, x, w, y = _band_problem(name)
    bw = _check_band_path(c, dtype, "band_stats")
    xd, wd = _act(x, dtype), _dev(w, dtype)
    y0 = _band_launch(xd, wd, dtype, c, False)
    y1, part = _band_launch(xd, wd, dtype, c, True)
    assert torch.equal(y1, y0), "the launch with statistics stores another output than the plain one"
    _assert_equal(y1, y.reshape(c.M, c.Cout), "y", 256)
    stored = _np(y1)
    want = np.zeros((bw.tiles, 2, c.Cout))
    for t in range(bw.tiles):
        rows = stored[t * 256:(t + 1) * 256]
        want[t, 0], want[t, 1] = rows.sum(0), (rows ** 2).sum(0)
    assert float(want[:, 1].max()) <= 2 ** 22
    _assert_equal(part, want, "partial[tile][sum y | sum y^2][channel]")


# ---- split-K --------------------------------------------------------------------------------------------------------------------------

def _splitk_launch(x, w, dtype, N, H, W, Cin, Cout, S):
    lib = _lib()
    M = N * H * W
    need = int(lib.rn_conv3x3_dense_splitk_workspace_bytes(N, H, W, Cout))
    assert need == S * M * Cout * 4, (need, S, M, Cout)
    ws = _f32_guarded(need // 4)
    y = _guarded(M * Cout)
    rc = lib.rn_conv3x3_dense_splitk(x.data_ptr(), w.data_ptr(), y.data_ptr(), _dt(dtype), N, H, W, Cin, Cout, _zero().data_ptr(), ws.data_ptr(), need, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((_zero() == 0).all()), "the zero page was written"
    return _take(y, M * Cout, dtype, "y").view(M, Cout), _take_f32(ws, need // 4, "the workspace").view(S, M, Cout)


def _splitk_path(S: int, Cin: int, Cout: int, dtype, what: str):
    cus = _cus()
    N, H, W = R.splitk_shape(S, Cout, cus)
    M = N * H * W
    got = R.dense_ksplit(M, Cout, cus)
    assert got == S, (f"{what}: {M} positions x {Cout} channels are {R.row_tiles(M) * (Cout // 256)} workgroups on {cus} CUs: {got} K ranges, not {S} -- "
                      f"choose a new shape in tests/dense_conv_ref.py (splitk_shape)")
    ranges = R.ksplit_ranges(Cin, S)
    print(f"{what} {dtype}: cus {cus} N {N} H {H} W {W} M {M} tiles {R.row_tiles(M)} column tiles {Cout // 256} S {S} K ranges {ranges} of {9 * Cin // 64} K-tiles")
    return N, H, W, ranges


@functools.lru_cache(maxsize=2)
def _splitk_problem(S: int, Cin: int, Cout: int, N: int, H: int, W: int):
    x, w, _ = R.forward_operands(N, H, W, Cin, Cout)
    y = R.conv_ref(x, w)
    R.assert_forward_exact(x, w, None, y, None)
    parts = [R.conv_ref(x, w, ktiles=r) for r in R.ksplit_ranges(Cin, S)]
    return x, w, y, parts


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("S,Cin,Cout", [(3, 64, 512), (3, 192, 512), (2, 64, 256), (2, 192, 256)])
def test_integer_operands_give_the_exact_split_k_convolution_range_by_range(S, Cin, Cout, dtype):
    N, H, W, ranges = _splitk_path(S, Cin, Cout, dtype, f"splitk S{S} Cin {Cin} Cout {Cout}")
    x, w, y, parts = _splitk_problem(S, Cin, Cout, N, H, W)
    got, ws = _splitk_launch(_act(x, dtype), _dev(w, dtype), dtype, N, H, W, Cin, Cout, S)
    for z, r in enumerate(ranges):
        _assert_equal(ws[z], parts[z].reshape(-1, Cout), f"workspace of K range {z} (K-tiles {r[0]} .. {r[1] - 1}, kt = 9 chunk + tap)", 256)
    _assert_equal(got, y.reshape(-1, Cout), "y", 256)


def test_split_k_declines_where_one_range_fills_half_the_chip():
    lib = _lib()
    cus = _cus()
    tiles = cus // 2 + 1
    N, H, W = 1, tiles, 256
    assert R.dense_ksplit(N * H * W, 256, cus) == 1 and R.dense_ksplit((tiles - 1) * 256, 256, cus) == 2
    assert lib.rn_conv3x3_dense_splitk_workspace_bytes(N, H, W, 256) == 0
    assert lib.rn_conv3x3_dense_splitk_workspace_bytes(1, tiles - 1, 256, 256) == 2 * (tiles - 1) * 256 * 256 * 4
    assert lib.rn_conv3x3_dense_splitk_workspace_bytes(1, 3, 256, 500) == 0                  # Cout not a multiple of 256
    x = torch.zeros((N * H * W, 64), dtype=torch.bfloat16, device=DEV)
    w = torch.zeros((256, 9, 64), dtype=torch.bfloat16, device=DEV)
    y = _guarded(N * H * W * 256)
    ws = _f32_guarded(4)
    rc = lib.rn_conv3x3_dense_splitk(x.data_ptr(), w.data_ptr(), y.data_ptr(), _dt(torch.bfloat16), N, H, W, 64, 256, _zero().data_ptr(), ws.data_ptr(), 16, _stream())
    torch.cuda.synchronize()
    assert rc == RN_EUNSUPPORTED, rc
    assert bool((y == 0x7B7B).all()) and bool((ws == 0xFF).all()), "a declined call wrote"
    print(f"splitk declined: cus {cus} tiles {tiles} S 1")


# ---- the weight gradient ------------------------------------------------------------------------------------------------------------

def _wgrad_launch(gs, xs, dtype, N, hw, splits: R.WgradSplits):
    "-> (partials f32 [splits][9][256][256] as wgrad_reduce_dense_kernel reads them, [dW [256][9][256] per problem])"
    lib = _lib()
    P = len(gs)
    need = int(lib.rn_conv3x3_dense_wgrad_workspace_bytes(P))
    assert need == splits.budget * 9 * 65536 * 4, (need, splits.budget)
    ws = _f32_guarded(need // 4)
    dws = [_guarded(256 * 9 * 256) for _ in range(P)]
    rc = lib.rn_conv3x3_dense_wgrad_batched(_ptrs(gs), _ptrs(xs), _ptrs(dws), P, _dt(dtype), N, _ints([h for h, _ in hw]), _ints([w for _, w in hw]), 256, 256,
                                            _zero().data_ptr(), ws.data_ptr(), need, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((_zero() == 0).all()), "the zero page was written"
    part = _take_f32(ws, need // 4, "the workspace").view(splits.budget, 9, 256, 256)
    assert bool((part[splits.total:].view(torch.int32) == -1).all()), "a split that does not exist was written"
    return part[:splits.total], [_take(d, 256 * 9 * 256, dtype, f"dW of problem {p}").view(256, 9, 256) for p, d in enumerate(dws)]


def _wgrad_path(kind: str, N: int, hw, dtype) -> R.WgradSplits:
    cus = _cus()
    Ms = [N * h * w for h, w in hw]
    s = R.dense_splits(Ms, cus)
    assert s.budget == max(cus // 9, len(Ms))
    print(f"wgrad {kind} {dtype}: cus {cus} P {len(Ms)} N {N} hw {hw} M {Ms} budget {s.budget} tps {s.tps} splits {s.beg} "
          f"tiles per split {[s.tiles_of(i) for i in range(s.total)]}")
    return s


def _split_refs(g, x, s: R.WgradSplits, p: int, absolute: bool = False):
    "The reference restricted to the positions of each split of problem p, in the workspace's [tap][n][c] order."
    if absolute:
        g, x = np.abs(g), np.abs(x)
    ranges = [(m0, m1) for q, m0, m1 in s.rows if q == p]
    return [r.reshape(256, 9, 256).transpose(1, 0, 2) for r in R.wgrad_ref_ranges(g, x, ranges)]


@functools.lru_cache(maxsize=2)
def _wgrad_problem(kind: str, cus: int):
    N, hw = R.wgrad_case_shapes(kind, cus)
    ops = [R.wgrad_operands(N, h, w, 256, 256, seed=p) for p, (h, w) in enumerate(hw)]
    refs = [R.wgrad_ref(g, x) for g, x in ops]
    for (g, x), ref in zip(ops, refs):
        R.assert_wgrad_exact(g, x, ref, R.abs_wgrad_ref(g, x))
    s = R.dense_splits([N * h * w for h, w in hw], cus)
    split_refs = [r.astype(np.float32) for p, (g, x) in enumerate(ops) for r in _split_refs(g, x, s, p)]      # (integers below 2^24: exact)
    return N, hw, ops, refs, split_refs


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", R.WKINDS)
def test_integer_operands_give_the_exact_weight_gradient_split_by_split(kind, dtype):
    N, hw, ops, refs, split_refs = _wgrad_problem(kind, _cus())
    s = _wgrad_path(kind, N, hw, dtype)
    want_tps = 3 if kind.startswith("p3") else 1
    assert s.tps == want_tps, f"{kind}: tps {s.tps}, not {want_tps} -- choose new shapes in tests/dense_conv_ref.py (wgrad_case_shapes)"
    if kind == "p3_tps3_tails":
        assert [N * h * w for h, w in hw[:2]] == [64 * s.tps + 1, 64 * 2 * s.tps - 1] and [s.tiles_of(i) for i in range(4)] == [3, 1, 3, 3]
    part, dws = _wgrad_launch([_act(g, dtype) for g, _ in ops], [_act(x, dtype) for _, x in ops], dtype, N, hw, s)
    for i, (p, m0, m1) in enumerate(s.rows):
        _assert_equal(part[i], split_refs[i], f"partial of split {i} (problem {p}, positions {m0} .. {m1 - 1}) [tap][n][c]")
    for p, dw in enumerate(dws):
        _assert_equal(dw, refs[p].reshape(256, 9, 256), f"dW of problem {p} [n][tap][c]")


# ---- N(0, 1) operands: half a unit in the last place + the summation bound ------------------------------------------------------------

def _real(shape, dtype, seed: int) -> np.ndarray:
    "N(0, 1) values as ``dtype`` holds them."
    return _round_to(np.random.default_rng(7000 + seed).standard_normal(shape, dtype=np.float32), dtype)


def _within(got: torch.Tensor, ref: np.ndarray, bound: np.ndarray, dtype, what: str) -> float:
    "got (16-bit) against ref: |err| <= half an ulp of ref + BOUND_SCALE * bound, element by element; returns the largest ratio."
    err = np.abs(_np(got).reshape(ref.shape) - ref)
    lim = R.half_ulp(ref, dtype == torch.bfloat16) + BOUND_SCALE * bound
    ratio = float((err / lim).max())
    print(f"{what} {dtype}: max err / (half ulp + bound) = {ratio:.3e}")
    assert bool((err <= lim).all()), f"{what}: max err / (half ulp + bound) = {ratio}"
    return ratio


def _f32_within(got: torch.Tensor, ref: np.ndarray, bound: np.ndarray, dtype, what: str) -> None:
    err = np.abs(_np(got).reshape(ref.shape) - ref)
    ok = bound > 0
    ratio = float((err[ok] / bound[ok]).max()) if ok.any() else 0.0
    print(f"{what} {dtype}: max err / bound = {ratio:.3e} (f32)")
    assert bool((err <= BOUND_SCALE * bound).all()), f"{what}: max err / bound = {ratio}"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_real_operands_dense_forward_and_data_gradient_stay_inside_the_bound(dtype):
    c = R.REAL_DENSE
    xs = [_real((c.N, h, w, c.Cin), dtype, p) for p, (h, w) in enumerate(c.hw)]
    ws = [_real((c.Cout, 3, 3, c.Cin), dtype, 10 + p) for p in range(len(c.hw))]
    print(f"dense real {dtype}: M {c.Ms} row tiles {R.dense_grid(c.Ms, c.Cin, c.Cout).tile_beg}")
    ys = _dense_launch([_act(x, dtype) for x in xs], [_dev(w, dtype) for w in ws], None, False, dtype, c.N, c.hw, c.Cin, c.Cout)
    for p, y in enumerate(ys):
        ref = R.conv_ref(xs[p], ws[p]).reshape(-1, c.Cout)
        _within(y, ref, R.sum_bound(9 * c.Cin, R.abs_conv_ref(xs[p], ws[p]).reshape(-1, c.Cout)), dtype, f"dense_batched problem {p}")
    d = R.REAL_DGRAD
    g = _real((d.N, *d.hw[0], d.Cout), dtype, 20)
    w = _real((d.Cout, 3, 3, d.Cin), dtype, 21)
    wf = R.dgrad_weights(w)
    dx = _dense_launch([_act(g, dtype)], [_dev(wf, dtype)], None, False, dtype, d.N, d.hw, d.Cout, d.Cin)[0]
    _within(dx, R.conv_ref(g, wf).reshape(-1, d.Cin), R.sum_bound(9 * d.Cout, R.abs_conv_ref(g, wf).reshape(-1, d.Cin)), dtype, "dgrad")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_real_operands_band_convolution_and_statistics_stay_inside_the_bound(dtype):
    c = R.REAL_BAND
    bw = _check_band_path(c, dtype, "band real")
    x, w = _real((c.N, c.H, c.W, c.Cin), dtype, 30), _real((c.Cout, 3, 3, c.Cin), dtype, 31)
    xd, wd = _act(x, dtype), _dev(w, dtype)
    y0 = _band_launch(xd, wd, dtype, c, False)
    y1, part = _band_launch(xd, wd, dtype, c, True)
    assert torch.equal(y1, y0)
    _within(y0, R.conv_ref(x, w).reshape(c.M, c.Cout), R.sum_bound(9 * c.Cin, R.abs_conv_ref(x, w).reshape(c.M, c.Cout)), dtype, "dense_band")
    stored = _np(y1)
    for t in range(bw.tiles):                       # sums of the STORED values (y^2 of a 16-bit value is exact in fp32): rows - 1 additions each
        rows = stored[t * 256:(t + 1) * 256]
        _f32_within(part[t, 0], rows.sum(0), R.sum_bound(len(rows), np.abs(rows).sum(0)), dtype, f"band_stats tile {t} sum y")
        _f32_within(part[t, 1], (rows ** 2).sum(0), R.sum_bound(len(rows), (rows ** 2).sum(0)), dtype, f"band_stats tile {t} sum y^2")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_real_operands_split_k_stays_inside_the_bound(dtype):
    c = R.REAL_SPLITK
    S = R.dense_ksplit(c.M, c.Cout, _cus())
    assert S == 3, f"{c.M} positions x {c.Cout} channels: {S} K ranges on {_cus()} CUs"
    ranges = R.ksplit_ranges(c.Cin, S)
    print(f"splitk real {dtype}: M {c.M} tiles {R.row_tiles(c.M)} S {S} K ranges {ranges}")
    x, w = _real((c.N, c.H, c.W, c.Cin), dtype, 40), _real((c.Cout, 3, 3, c.Cin), dtype, 41)
    y, ws = _splitk_launch(_act(x, dtype), _dev(w, dtype), dtype, c.N, c.H, c.W, c.Cin, c.Cout, S)
    xa, wa = np.abs(x), np.abs(w)
    for z, r in enumerate(ranges):
        _f32_within(ws[z], R.conv_ref(x, w, ktiles=r).reshape(c.M, c.Cout), R.sum_bound(64 * (r[1] - r[0]), R.conv_ref(xa, wa, ktiles=r).reshape(c.M, c.Cout)),
                    dtype, f"dense_splitk workspace of range {z}")
    # y: the ranges added in order z = 0, 1, .. in f32 and rounded once (dense_ksplit_reduce_kernel) -- bit for bit
    acc = ws[0].clone()
    for z in range(1, S):
        acc = acc + ws[z]
    assert torch.equal(y, acc.to(dtype)), "y is not the ordered f32 sum of the workspace, rounded once"
    _within(y, R.conv_ref(x, w).reshape(c.M, c.Cout), R.sum_bound(9 * c.Cin, R.abs_conv_ref(x, w).reshape(c.M, c.Cout)), dtype, "dense_splitk")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_real_operands_weight_gradient_stays_inside_the_bound(dtype):
    N, hw = R.REAL_WGRAD
    s = _wgrad_path("real", N, hw, dtype)
    assert s.total >= len(hw)
    ops = [(_real((N, h, w, 256), dtype, 50 + p), _real((N, h, w, 256), dtype, 60 + p)) for p, (h, w) in enumerate(hw)]
    part, dws = _wgrad_launch([_act(g, dtype) for g, _ in ops], [_act(x, dtype) for _, x in ops], dtype, N, hw, s)
    want = [r for p, (g, x) in enumerate(ops) for r in _split_refs(g, x, s, p)]
    mags = [r for p, (g, x) in enumerate(ops) for r in _split_refs(g, x, s, p, absolute=True)]
    for i, (p, m0, m1) in enumerate(s.rows):
        _f32_within(part[i], want[i], R.sum_bound(m1 - m0, mags[i]), dtype, f"dense_wgrad partial of split {i}")
    for p, dw in enumerate(dws):
        # dW: the problem's splits added in order in f32 from zero and rounded once (wgrad_reduce_dense_kernel) -- bit for bit
        acc = torch.zeros_like(part[0])
        for q in range(s.beg[p], s.beg[p + 1]):
            acc = acc + part[q]
        assert torch.equal(dw, acc.permute(1, 0, 2).to(dtype)), f"dW of problem {p} is not the ordered f32 sum of its splits, rounded once"
        M = N * hw[p][0] * hw[p][1]
        _within(dw, R.wgrad_ref(*ops[p]).reshape(256, 9, 256), R.sum_bound(M, R.abs_wgrad_ref(*ops[p]).reshape(256, 9, 256)), dtype, f"dense_wgrad problem {p}")
