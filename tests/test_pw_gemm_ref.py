"""CPU: the float64 reference of ``pw_gemm_ref.py`` on its own -- the contraction against torch's float64 convolution, the epilogue
restatements against plain float64 / int64 arithmetic, the work split, and for every case of the table the properties it is there for and
the operand generator's promises (exact small integers in bf16 and fp16, every accumulator and every per-walker partial sum an integer
below 2^24) that let ``test_pw_gemm_gpu.py`` ask the kernel for equality."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pw_gemm_ref as R

DTYPES = [torch.bfloat16, torch.float16]


@pytest.mark.parametrize("nimg", [1, 2, 3])
@pytest.mark.parametrize("taps,stride", [(1, 1), (1, 2), (9, 1), (9, 2)])
@pytest.mark.parametrize("H,W", [(13, 17), (12, 10), (1, 5)])
def test_reference_equals_the_float64_convolution(nimg, taps, stride, H, W):
    N, Cin, k = 5, 6, (3 if taps == 9 else 1)
    geo, pad = R.geometry(nimg, H, W, taps, stride)
    gen = torch.Generator().manual_seed(100 * nimg + 10 * taps + stride)
    x = torch.randn((nimg, Cin, H, W), dtype=torch.float64, generator=gen)
    w = torch.randn((N, Cin, k, k), dtype=torch.float64, generator=gen)
    x2d, w3d = x.permute(0, 2, 3, 1).reshape(geo.rows, Cin), w.permute(0, 2, 3, 1).reshape(N, taps, Cin)
    for f, g in ((lambda t: t, R.gemm_ref), (torch.abs, R.abs_terms)):
        want = F.conv2d(f(x), f(w), None, stride, pad).permute(0, 2, 3, 1).reshape(geo.M, N)
        got = g(x2d, w3d, taps, stride, pad, geo)
        assert got.shape == want.shape and got.dtype == torch.float64
        err, scale = float((got - want).abs().max()), float(want.abs().max())
        assert err <= 1e-12 * scale, (err, scale)


def test_padding_applies_to_the_transformed_activation():
    "relu(x a + b) with b > 0 is not zero at x = 0: a tap outside the image must still contribute nothing."
    geo, pad = R.geometry(1, 3, 3, 9, 1)
    x = torch.zeros((9, 64), dtype=torch.bfloat16)
    coef = torch.cat([torch.ones(64), torch.ones(64)])                  # X' = 1 everywhere inside the image
    xt = R.pro_affine_relu(x, coef, torch.bfloat16)
    y = R.gemm_ref(xt, torch.ones((1, 9, 64), dtype=torch.bfloat16), 9, 1, pad, geo)
    assert [int(v) for v in y[:, 0]] == [64 * n for n in (4, 6, 4, 6, 9, 6, 4, 6, 4)]


@pytest.mark.parametrize("M", [1, 127, 128, 129, 65536, 65537, 65664, 65665, 131072, 131073, 131201, 66248, 263538, 537600])
def test_walk_partitions_the_row_tiles(M):
    wk = R.walk(M)
    assert wk.MT == -(-M // 128) and wk.gx <= 512 and wk.rounds == -(-wk.MT // 512)
    assert (wk.rounds == 1) == (M <= 65536) and (wk.gx == wk.MT) == (wk.rounds == 1)
    seen = np.zeros(wk.MT, dtype=np.int64)
    for w in range(wk.gx):
        t = wk.tiles(w)
        assert 1 <= len(t) <= wk.rounds and t == [w + r * wk.gx for r in range(len(t))]
        seen[t] += 1
    assert (seen == 1).all()
    assert sum(R.walker_rows(wk)) == M and wk.depth == -(-wk.MT // wk.gx)
    w, r, rows = wk.ragged
    assert wk.tiles(w)[r] == wk.MT - 1 and rows == M - 128 * (wk.MT - 1)


def test_walker_sums_against_a_loop():
    M, N = 3 * 128 + 5, 4
    wk = R.Walk(M, 4, 2, 2)                 # (a split the library would not choose at this size: the restatement is general)
    t = torch.arange(M * N, dtype=torch.float64).view(M, N)
    got = R.walker_sums(t, wk)
    for w in range(2):
        want = sum(t[tile * 128:(tile + 1) * 128].sum(0) for tile in wk.tiles(w))
        assert torch.equal(got[w], want)
    assert R.walker_rows(wk) == [256, 133]


def test_the_production_row_count_walks_nine_tiles():
    wk = R.walk(8 * 200 * 336)
    assert (wk.MT, wk.rounds, wk.gx, wk.depth) == (4200, 9, 467, 9)


# ---- epilogue restatements -------------------------------------------------------------------------------------------------------

def _ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, shape)


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bias_residual_relu_restatement(dtype):
    rng = np.random.default_rng(3)
    M, N = 37, 64
    acc, b, r = _ints(rng, -40, 40, (M, N)), _ints(rng, -3, 3, N), _ints(rng, -3, 3, (M, N))
    mask = rng.random((M, N)) > 0.5
    for use_b, use_r, relu in ((True, False, False), (True, False, True), (True, True, True), (True, True, False), (False, True, False)):
        want = acc + (b if use_b else 0) + (r if use_r else 0)
        want = np.maximum(want, 0) if relu else want
        pre, y = R.epi_store(_t(acc, torch.float64), dtype, _t(b, torch.float32) if use_b else None,
                             R.resid_term(_t(r, dtype), None, 1, M) if use_r else None, relu)
        assert np.array_equal(y.numpy(), want.astype(np.float64)) and torch.equal(pre, y)
    got = R.resid_term(_t(r, dtype), R.pack_bits(torch.from_numpy(mask)), 1, M)
    assert np.array_equal(got.numpy(), (r * mask).astype(np.float64))
    # one rounding, at the end, after the residual and the ReLU: 256.5 + 0.75 is 257.25 -> 257 (fp16) / 258 (bf16), not round(256.5) + 0.75
    pre, y = R.epi_store(torch.tensor([[256.5, -1.0]], dtype=torch.float64), dtype, None, torch.tensor([[0.75, 0.25]], dtype=torch.float64), True)
    assert pre.tolist() == [[257.25, 0.0]] and y.tolist() == [[257.25 if dtype == torch.float16 else 258.0, 0.0]]


@pytest.mark.parametrize("rH,rW", [(5, 7), (4, 6), (1, 3)])
def test_stride_2_residual_joins_the_even_rows_only(rH, rW):
    nimg, N = 2, 8
    h2, w2 = (rH + 1) // 2, (rW + 1) // 2
    Rs = torch.arange(1, nimg * h2 * w2 * N + 1, dtype=torch.float64).view(nimg * h2 * w2, N)
    got = R.resid_term(Rs, None, 2, nimg * rH * rW, rH, rW).view(nimg, rH, rW, N)
    want = torch.zeros((nimg, rH, rW, N), dtype=torch.float64)
    want[:, ::2, ::2, :] = Rs.view(nimg, h2, w2, N)
    assert torch.equal(got, want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_relu_backward_restatement_on_integers(dtype):
    rng = np.random.default_rng(4)
    M, N = 41, 64
    acc, zp = _ints(rng, -300, 300, (M, N)), _ints(rng, -3, 3, (M, N))
    emean, einv, ea, eb = _ints(rng, -1, 1, N), _ints(rng, 1, 2, N), _ints(rng, 1, 2, N), _ints(rng, -1, 1, N)
    est = _t(np.concatenate([emean, einv, ea, eb]), torch.float32)
    rb = R.relu_bwd(_t(acc, torch.float64), _t(zp, dtype), est, dtype)
    alive = zp * ea + eb >= 1
    stored = _t(acc, torch.float32).to(dtype).double().numpy()          # |acc| up to 300 needs nine bits: bf16 rounds some of them
    assert np.array_equal(rb.alive.numpy(), alive) and not bool(rb.near.any())
    assert np.array_equal(rb.y.numpy(), stored * alive)
    assert np.array_equal(rb.xhat.numpy(), ((zp - emean) * einv).astype(np.float64))
    s, q = R.partial_terms(R.CASES[[c.name for c in R.CASES].index("relu_bwd")], R.Expected(None, None, rb.y, None, rb.alive, rb.xhat, 0, None), rb.y)
    assert np.array_equal(q.numpy(), stored * alive * (zp - emean) * einv) and s is rb.y


def test_relu_backward_threshold_and_its_neighbourhood():
    "The mask opens strictly above alive_dt; the two fp32 neighbours of the threshold and the threshold itself are 'near'."
    for dtype in DTYPES:
        thr = torch.tensor(R.ALIVE[dtype], dtype=torch.float32)
        up, dn = torch.nextafter(thr, thr + 1), torch.nextafter(thr, thr - 1)
        up2 = torch.nextafter(up, up + 1)
        eb = torch.stack([thr, up, dn, up2, torch.zeros(()), -thr])
        n = eb.numel()
        est = torch.cat([torch.zeros(n), torch.ones(n), torch.zeros(n), eb])        # ea = 0: the fma is eb
        rb = R.relu_bwd(torch.ones((1, n), dtype=torch.float64), torch.ones((1, n), dtype=dtype), est, dtype)
        assert rb.alive.tolist() == [[False, True, False, True, False, False]]
        assert rb.near.tolist() == [[True, True, True, False, False, False]]


def test_stats_are_those_of_the_stored_output():
    y = torch.tensor([[258.0, -3.0]], dtype=torch.float64)
    s, q = R.stats_terms(y)
    assert s.tolist() == [[258.0, -3.0]] and q.tolist() == [[258.0 ** 2, 9.0]]


# ---- the case table --------------------------------------------------------------------------------------------------------------------

def test_case_table_covers_what_it_claims():
    names = [c.name for c in R.CASES]
    assert len(set(names)) == len(names)
    by = {c.name: c for c in R.CASES}
    for c in R.CASES:
        wk = R.walk(c.M)
        assert (wk.MT, wk.rounds, wk.gx, wk.ragged) == R.EXPECT_WALK[c.M], (c.name, wk, wk.ragged)
        assert wk.rounds >= 2 and wk.depth == wk.rounds and wk.ragged[1] >= 1, c.name        # the ragged tile is a LATER tile of its walker
        assert c.Cin % 64 == 0 and c.N % 64 == 0 and c.KT == c.taps * c.Cin // 64 and c.ny == c.N // c.BN, c.name
        assert c.M * c.N < 2 ** 31 and c.geo.rows * c.Cin < 2 ** 31
    r2 = [by[n] for n in ("r2_128x64", "r2_192x64", "r2_128x128", "r2_256x256", "r2_64x192")]
    assert all(c.M == 65537 and c.plain and c.pro is None and not c.epi for c in r2)
    assert [(c.KT, c.BN, c.ny) for c in r2] == [(2, 64, 1), (3, 64, 1), (2, 128, 1), (4, 128, 2), (1, 64, 3)]
    wk = R.walk(65537)
    assert wk.gx % 8 == 1 and 8 * -(-wk.gx // 8) - wk.gx == 7                   # the XCD map leaves seven slots idle
    assert wk.tiles(255) == [255, 512] and wk.tiles(256) == [256] and wk.M - 512 * 128 == 1
    # rounds 3: the issue's row count gives every walker three tiles; 128 rows fewer put a walker with two next to them
    r3 = [by[n] for n in ("r3_128x128", "r3_192x192", "r3s_128x128", "r3s_192x192")]
    assert [(c.M, c.KT, c.ny) for c in r3] == [(131201, 2, 1), (131201, 3, 3), (131073, 2, 1), (131073, 3, 3)]
    assert {len(R.walk(131201).tiles(w)) for w in range(342)} == {3}
    assert [len(R.walk(131073).tiles(w)) for w in (340, 341)] == [3, 2] and R.walk(131073).gx % 8 == 6
    # the position decode
    conv = [by[n] for n in ("s2_1x1_c64", "s2_1x1_c128", "s2_3x3_c64", "s2_3x3_c128", "s1_3x3_c64", "s1_3x3_c128")]
    assert all(c.M == 66248 and c.nimg == 2 and not c.plain and (c.geo.Ho, c.geo.Wo) == (182, 182) for c in conv)
    assert [(c.taps, c.stride, c.H, c.KT) for c in conv] == [(1, 2, 363, 1), (1, 2, 363, 2), (9, 2, 363, 9), (9, 2, 363, 18), (9, 1, 182, 9), (9, 1, 182, 18)]
    wk = R.walk(66248)
    assert wk.gx % 8 == 3 and any(c.ny >= 2 for c in conv)
    assert 182 * 182 // 128 < wk.gx                # two images: their seam lies in a first tile; the three-image cases put the second one later
    n3 = [by[n] for n in ("s2_3x3_c64_n3", "s1_3x3_c64_n3")]
    wk = R.walk(3 * 182 * 182)
    seam = 2 * 182 * 182
    assert all(c.M == wk.M and c.nimg == 3 and c.KT == 9 for c in n3) and seam // 128 >= wk.gx and seam % 128 != 0
    # prologues and epilogues: every form, at KT >= 2; both tile widths under PRO_BN_BWD
    pro = [c for c in R.CASES if c.pro is not None and not c.epi]
    assert {(c.pro, c.Cin, c.N) for c in pro} == {(p, ci, n) for p in ("aff", 0, 2, 3) for ci, n in ((128, 64), (256, 128))}
    epi = [c for c in R.CASES if c.epi and c.pro is None]
    assert {c.epi for c in epi} == {"stats", "resid_bits", "resid", "resid_s2", "relu_bwd", "bias", "bias_resid_relu"} and all(c.KT >= 2 for c in epi)
    assert by["stats_r3"].M == by["relu_bwd_r3"].M == 131201 and by["stats_xcd"].ny == 2
    assert by["resid_s2"].M == 2 * 363 * 363 and by["resid_s2"].res_hw == (363, 363) and by["resid_s2"].plain
    pairs = {(c.pro, c.epi, c.BN) for c in R.CASES if c.pro is not None and c.epi} | {(None, "resid_bits", 128)}
    assert pairs == {("aff", "stats", 128), (3, "relu_bwd", 64), (3, "relu_bwd", 128), (2, "relu_bwd", 64), (2, "relu_bwd", 128), (None, "resid_bits", 128)}
    assert by["none_resid_bits_128x256"].BN == 128


def test_generator_gives_the_same_integers_in_both_types_and_every_value_of_its_range():
    c = R.CASES[0]
    a, b = R.operands(c, torch.bfloat16, True), R.operands(c, torch.float16, True)
    assert torch.equal(a.x.double(), b.x.double()) and torch.equal(a.w.double(), b.w.double())
    assert sorted(a.x.double().unique().tolist()) == [-2.0, -1.0, 0.0, 1.0, 2.0]
    counts = torch.bincount((a.x.double() + 2).long().view(-1), minlength=5).double() / a.x.numel()
    assert float((counts - 0.2).abs().max()) < 2e-3
    assert not torch.equal(R.operands(c, torch.bfloat16, True, seed=1).x, a.x)
    r = R.operands(c, torch.bfloat16, False)
    assert abs(float(r.x.float().mean())) < 2e-3 and abs(float(r.x.float().std()) - 1) < 5e-3
    assert abs(float((r.x[:-1].float() * r.x[1:].float()).mean())) < 2e-3                # neighbours do not correlate


def test_fp16_bn_backward_prologue_rounds_once():
    "The fp16 restatement against the twice-rounded one: equal on integers, one fp16 unit apart on a rare tie, never further from the exact value."
    f16 = torch.float16
    # a g + t = 1 + 2^-11 + 2^-30: rounded to fp32 it is the fp16 tie 1 + 2^-11 (-> 1, to even); rounded once it lies above the tie
    g, z = torch.ones((1, 8), dtype=f16), torch.zeros((1, 8), dtype=f16)
    coef3 = torch.cat([torch.ones(8), torch.full((8,), 2.0 ** -11 + 2.0 ** -30), torch.zeros(8)])
    assert R.pro_bn_bwd(g, z, coef3, 0, f16).tolist() == [[1.0] * 8]
    assert R.pro_bn_bwd_f16(g, z, coef3, 0).tolist() == [[1.0 + 2.0 ** -10] * 8]
    v = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(2.0 ** -25), 3 * 2.0 ** -25, 2.0 ** -25 + 2.0 ** -40, 65504.0, 0.0], dtype=torch.float64)
    assert R.round_f16_once(v).tolist() == [1.0, 1.0 + 2.0 ** -9, -0.0, 2.0 ** -23, 2.0 ** -24, 65504.0, 0.0]
    gen = torch.Generator().manual_seed(11)
    M, Cc = 4096, 64
    g, z = torch.randn((M, Cc), generator=gen).to(f16), torch.randn((M, Cc), generator=gen).to(f16)
    coef3 = torch.cat([torch.rand(Cc, generator=gen) + 0.5, torch.randn(Cc, generator=gen) * 0.05, torch.randn(Cc, generator=gen) * 0.05])
    fwd = torch.cat([torch.rand(Cc, generator=gen) + 0.5, torch.randn(Cc, generator=gen) * 0.3])
    bits = R.pack_bits(torch.rand((M, Cc), generator=gen) > 0.4)
    for mode in (0, 2, 3):
        once, twice = R.pro_bn_bwd_f16(g, z, coef3, mode, fwd, bits), R.pro_bn_bwd(g, z, coef3, mode, f16, fwd, bits)
        assert torch.equal(once, once.to(f16).double())
        differ = once != twice
        assert float(differ.double().mean()) < 2e-3 and bool(((once - twice).abs()[differ] <= 2 * R.half_ulp(twice, f16)[differ] * 2).all())
        keep = {0: torch.ones((M, Cc), dtype=torch.bool), 2: R._fma32(z.float(), fwd[:Cc], fwd[Cc:]) > R.ALIVE[f16], 3: R.unpack_bits(bits, M, Cc)}[mode]
        inner = R._fma32(coef3[2 * Cc:], z.float(), coef3[Cc:2 * Cc]).double()
        exact = coef3[:Cc].double() * (g.double() * keep) + inner
        assert bool(((once - exact).abs() <= R.half_ulp(exact, f16)).all())            # half a unit, with nothing added
    gi, zi = torch.randint(-2, 3, (M, Cc), generator=gen).to(f16), torch.randint(-2, 3, (M, Cc), generator=gen).to(f16)
    ci = torch.cat([torch.randint(1, 3, (Cc,), generator=gen), torch.randint(-1, 2, (2 * Cc,), generator=gen)]).float()
    assert torch.equal(R.pro_bn_bwd_f16(gi, zi, ci, 3, None, bits), R.pro_bn_bwd(gi, zi, ci, 3, f16, None, bits))


def _exact_in_both_types(t):
    return torch.equal(t, t.round()) and torch.equal(t.to(torch.bfloat16).double(), t) and torch.equal(t.to(torch.float16).double(), t)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_integer_operands_are_exact_and_every_sum_stays_below_2_to_24(case):
    """What the GPU test's equality rests on.  Operands: integers exact in bf16 and fp16, the same in both types.  Accumulators: bounded by
    peak(|X'|) peak(|W|) K.  The cases that keep column sums: the output itself is formed here and every per-walker partial of both sums
    -- in any order: the sum of the terms' magnitudes -- is an integer below 2^24."""
    op = R.operands(case, torch.bfloat16, True)
    xt = R.transformed(case, op, torch.bfloat16)
    assert xt.shape == (case.geo.rows, case.Cin) and op.w.shape == (case.N, case.taps, case.Cin)
    assert _exact_in_both_types(xt) and _exact_in_both_types(op.w.double())
    assert float(xt.abs().max()) <= R.XT_PEAK[case.pro] and float(op.w.double().abs().max()) <= R.W_PEAK
    if case.pro is not None:
        # ... and fp16 stages the same values: the same fp32 arithmetic on the same integers, a last rounding that is exact in both types
        # (above), and under relu_mode 2 the same mask from either type's threshold; restated on every 37th row as well
        sl = slice(0, None, 37)
        bits = op.xbits.view(case.geo.rows, -1)[sl].reshape(-1) if op.xbits is not None else None
        sub = op._replace(x=op.x[sl].to(torch.float16), z=op.z[sl].to(torch.float16) if op.z is not None else None, xbits=bits)
        assert torch.equal(R.transformed(case, sub, torch.float16), xt[sl])
        if case.pro == 2:
            t = R._fma32(op.z.float(), op.fwd[:case.Cin], op.fwd[case.Cin:])
            assert torch.equal(t > R.ALIVE[torch.bfloat16], t > R.ALIVE[torch.float16])
        if case.pro == "aff":
            assert bool((xt >= 0).all()) and 0.2 < float((xt == 0).double().mean()) < 0.8
        if case.pro == 3:
            assert 0.55 < float(R.unpack_bits(op.xbits, case.geo.rows, case.Cin).double().mean()) < 0.65
        if case.pro == 2:
            assert 0.2 < float((t > R.ALIVE[torch.bfloat16]).double().mean()) < 0.8
    K = case.taps * case.Cin
    peak = R.XT_PEAK[case.pro] * R.W_PEAK * K + 2 * R.E_PEAK               # accumulator + bias + residual, in any order
    assert peak < 2 ** 24
    for t in (op.bias, op.R, op.zp, op.est):
        assert t is None or (_exact_in_both_types(t.double()) and float(t.double().abs().max()) <= R.E_PEAK)
    if case.epi not in ("stats", "relu_bwd"):
        return
    wk = R.walk(case.M)
    for dtype in DTYPES:
        ex = R.expected(case, op, dtype, xt)
        assert torch.equal(ex.acc, ex.acc.round()) and float(ex.acc.abs().max()) <= peak
        if case.epi == "relu_bwd":
            assert not bool(ex.keep.logical_not().any()) and 0.2 < float(ex.alive.double().mean()) < 0.8
        s, q = R.partial_terms(case, ex, ex.y)
        for t in (s, q):
            assert torch.equal(t, t.round())
            assert float(R.walker_sums(t.abs(), wk).max()) < 2 ** 24, case.name


@pytest.mark.parametrize("dtype", DTYPES)
def test_real_relu_backward_coefficients_leave_almost_nothing_near_the_threshold(dtype):
    "From the reference alone: with the real-valued generator the elements the GPU test may leave out are at most 1e-4 of a case."
    for case in (c for c in R.CASES if c.real and c.epi == "relu_bwd"):
        _, _, _, zp, est = R.epilogue_operands(case, dtype, False)
        rb = R.relu_bwd(torch.zeros((case.M, case.N), dtype=torch.float64), zp, est, dtype)
        assert float(rb.near.double().mean()) <= 1e-4 and 0.3 < float(rb.alive.double().mean()) < 0.7
