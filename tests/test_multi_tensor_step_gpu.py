"""GPU: the multi-tensor optimizer-side kernels (csrc/optim.hip, adam.hip, clip.hip, accum.hip, ema.hip, rn_multi.hpp) on the two paths
every real R50 / R101 step takes and the element-level tests with their 46 tensors of at most 4098 elements do not: tensors larger
than one pass of the step kernels' capped grid (rn::step_grid: 1024 blocks x 256 threads x 4 elements = 1 048 576 elements), and
more tensors than one kernel-argument table holds (48 SGD, 40 Adam, 160 accumulate / EMA update, 120 EMA swap, 224 clip).

Two kinds of assertion.  Against torch, at the bars the existing files set: the SGD bars of test_grad_clip_gpu._check_update,
test_master_adam_gpu._check_state for Adam, the torch restatements of test_grad_accum_gpu.py / test_weight_ema_gpu.py bit for bit,
the norm at test_norm_against_float64's bar.  And split invariance, bit for bit: these updates are element-independent, so the same
elements submitted as smaller tensors (one grid pass each) or in smaller calls (one table each) must give the same bits -- no
tolerance; a wrong stride, a skipped or doubled vector, a table slot filled from the wrong tensor fails it."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from test_grad_accum_gpu import _restated, _window
from test_grad_clip_gpu import BIG, _norm_call, _ulp
from test_master_adam_gpu import _check_state, _grads, _make
from test_weight_ema_gpu import _restate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ["f32", "bf16", "f16"]
CHUNK = 16384

# ---- A. the step kernels past one grid pass -------------------------------------------------------------------------------------
# just under the cap, the cap, the cap plus a scalar tail, 2.25 passes, 2.25 passes with a tail of 3 -- next to small tensors, so
# that the grid is sized by the largest and its short rows run too
PASS = 1024 * 256 * 4
BIG_SIZES = [1, PASS - 4, 3, PASS, 4097, PASS + 1, 2_359_296, 2_359_299]
PIECE = 262_144                                  # a multiple of 8 elements: every piece of every array stays 16-byte aligned
STEPS = 3                                        # the first-step branch and the steady one
STEP_CONFIGS = {
    "sgd": dict(momentum=0.9, weight_decay=1e-2),
    "sgd_no_momentum": dict(momentum=0.0, weight_decay=1e-2),
    "sgd_nesterov": dict(momentum=0.9, nesterov=True, weight_decay=1e-2),
    "adam": dict(weight_decay=0.05),
    "adamw": dict(weight_decay=0.1),
}


def _w(p):
    return p.master if hasattr(p, "master") else p.data


def _optimizers(kind, mine, ref):
    "(ours over ``mine`` in ONE parameter group -- all of them reach one call --, torch's single-tensor fp32 one over ``ref``)"
    from pytorch_retinanet_amd.optim import MasterAdam, MasterAdamW, MasterSGD
    kw = STEP_CONFIGS[kind]
    if kind.startswith("sgd"):
        return MasterSGD(mine, lr=0.05, **kw), (torch.optim.SGD(ref, lr=0.05, foreach=False, **kw) if ref is not None else None)
    cls, tcls = (MasterAdam, torch.optim.Adam) if kind == "adam" else (MasterAdamW, torch.optim.AdamW)
    return cls(mine, lr=1e-3, **kw), (tcls(ref, lr=1e-3, foreach=False, **kw) if ref is not None else None)


def _state_keys(kind):
    if kind.startswith("sgd"):
        return () if STEP_CONFIGS[kind]["momentum"] == 0.0 else ("momentum_buffer",)
    return ("exp_avg", "exp_avg_sq")


def _pieces(p):
    "Independent copies of ``p``'s master (and 16-bit copy), cut into parameters of at most PIECE elements; [(parameter, offset)]."
    w, out = _w(p).detach().clone(), []
    c16 = p.data.detach().clone() if hasattr(p, "master") else None
    for o in range(0, w.numel(), PIECE):
        if c16 is not None:
            q = torch.nn.Parameter(c16[o:o + PIECE])
            q.master = w[o:o + PIECE]
        else:
            q = torch.nn.Parameter(w[o:o + PIECE])
        assert _w(q).data_ptr() % 16 == 0 and q.data.data_ptr() % 16 == 0
        out.append((q, o))
    return out


def _check_sgd(mode, mine, ref, dt16):
    "test_grad_clip_gpu._check_update's SGD bars"
    rtol, atol = (2e-4, 2e-5) if mode == "f16" else (2e-5, 1e-6)
    for p, r in zip(mine, ref):
        torch.testing.assert_close(_w(p), r.detach(), rtol=rtol, atol=atol)
        if hasattr(p, "master"):
            assert torch.equal(p.data, p.master.to(dt16))


def _assert_same_bits(kind, opt, mine, others, where):
    """``others[i]``: [(parameter, its optimizer)], together the elements of ``mine[i]`` in order: masters, every state tensor and
    the 16-bit copies equal bit for bit."""
    for i, (p, parts) in enumerate(zip(mine, others)):
        cat = lambda f: torch.cat([f(q, o).reshape(-1) for q, o in parts])
        assert torch.equal(_w(p).reshape(-1), cat(lambda q, o: _w(q))), f"{where}: master {i} (n={p.numel()})"
        for k in _state_keys(kind):
            assert torch.equal(opt.state[p][k].reshape(-1), cat(lambda q, o: o.state[q][k])), f"{where}: {k} {i} (n={p.numel()})"
        if hasattr(p, "master"):
            assert torch.equal(p.data.reshape(-1), cat(lambda q, o: q.data)), f"{where}: 16-bit copy {i} (n={p.numel()})"


@pytest.fixture(scope="module", params=list(itertools.product(STEP_CONFIGS, MODES)), ids=lambda km: f"{km[0]}-{km[1]}")
def big_run(request):
    """STEPS steps over BIG_SIZES of: our optimizer; a second instance of it over the same elements cut into pieces of at most PIECE
    elements (each piece one grid pass); torch's optimizer on fp32 copies.  One run serves both tests of a case."""
    kind, mode = request.param
    mine, ref, dt16 = _make(BIG_SIZES, mode, seed=11)
    opt, ropt = _optimizers(kind, mine, ref)
    cut = [_pieces(p) for p in mine]
    opt2, _ = _optimizers(kind, [q for parts in cut for q, _ in parts], None)
    for s in range(STEPS):
        for p, r, g, parts in zip(mine, ref, _grads(mine, s), cut):
            p.grad, r.grad = g, g.float()
            for q, o in parts:
                q.grad = g[o:o + PIECE]
        opt.step()
        opt2.step()
        ropt.step()
    torch.cuda.synchronize()
    yield kind, mode, dt16, mine, ref, opt, ropt, [[(q, opt2) for q, _ in parts] for parts in cut]


def test_large_tensors_step_equals_torch(big_run):
    kind, mode, dt16, mine, ref, opt, ropt, _ = big_run
    if kind.startswith("sgd"):
        _check_sgd(mode, mine, ref, dt16)
        if not _state_keys(kind):                                   # momentum 0: the optimizer keeps no buffer and passes null entries
            assert all(opt.state[p]["momentum_buffer"] is None for p in mine)
    else:
        _check_state(opt, ropt, mine, ref, 1e-3, dt16, l2=STEP_CONFIGS[kind]["weight_decay"] if kind == "adam" else 0.0, steps=STEPS)
        assert opt.group_steps() == [float(STEPS)]


def test_large_tensors_step_equals_the_same_elements_in_pieces_bit_for_bit(big_run):
    kind, mode, dt16, mine, ref, opt, ropt, cut = big_run
    assert max(len(parts) for parts in cut) == 10 and sum(len(parts) for parts in cut) <= 40        # (pieces: one launch, one pass)
    _assert_same_bits(kind, opt, mine, cut, f"{kind} {mode}")


def test_sgd_without_momentum_takes_null_buffers_but_not_a_null_table():
    """momentum == 0: rn_sgd_master_step reads no momentum buffer, so the ENTRIES of ``momenta`` may be null (what MasterSGD passes);
    the array itself may not (RN_EINVAL, nothing moves)."""
    from pytorch_retinanet_amd._lib import RN_BF16, lib
    n = 4097
    w = torch.randn(n, device=DEV)
    g = torch.randn(n, device=DEV)
    before = w.clone()
    stream = torch.cuda.current_stream().cuda_stream
    args = lambda moms: ((C.c_void_p * 1)(w.data_ptr()), moms, (C.c_void_p * 1)(g.data_ptr()), (C.c_void_p * 1)(0), (C.c_int64 * 1)(n), 1, 0,
                         RN_BF16, 0.5, 0.0, 0.0, 0.0, 0, 1, None, None, None, stream)
    assert lib.rn_sgd_master_step(*args(None)) == -1                   # RN_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(w, before)
    assert lib.rn_sgd_master_step(*args((C.c_void_p * 1)(0))) == 0
    torch.cuda.synchronize()
    assert torch.equal(w, before - 0.5 * g)
    a = args((C.c_void_p * 1)(0))
    assert lib.rn_sgd_master_step(*a[:9], 0.9, *a[10:]) == -1          # with a momentum the null entry is refused
    torch.cuda.synchronize()
    assert torch.equal(w, before - 0.5 * g)


# ---- B. more tensors than one table ---------------------------------------------------------------------------------------------
# 230 tensors; a multi-chunk tensor is the last slot of a full table for SGD (48), accumulate / EMA update (160) and the clip (224),
# and the list ends in the partly filled last table
MANY = [(1, 3, 7, 8, 1023, 4097)[i % 6] for i in range(230)]
for _i in (47, 159, 223):
    MANY[_i] = CHUNK + 5
MANY[229] = 40_000


def _slices(n, k):
    return [slice(o, min(o + k, n)) for o in range(0, n, k)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["sgd", "adam", "adamw"])
def test_many_tensors_step_equals_torch_and_optimizers_of_at_most_40(kind, mode):
    mine, ref, dt16 = _make(MANY, mode, seed=12)
    few, _, _ = _make(MANY, mode, seed=12)                              # the same tensors again, for instances of <= 40 (one table each)
    opt, ropt = _optimizers(kind, mine, ref)
    opts = [(sl, _optimizers(kind, few[sl], None)[0]) for sl in _slices(len(few), 40)]
    for s in range(STEPS):
        for p, q, r, g in zip(mine, few, ref, _grads(mine, s)):
            p.grad, q.grad, r.grad = g, g.clone(), g.float()
        opt.step()
        for _, o in opts:
            o.step()
        ropt.step()
    torch.cuda.synchronize()
    if kind == "sgd":
        _check_sgd(mode, mine, ref, dt16)
    else:
        _check_state(opt, ropt, mine, ref, 1e-3, dt16, l2=STEP_CONFIGS[kind]["weight_decay"] if kind == "adam" else 0.0, steps=STEPS)
        assert opt.group_steps() == [float(STEPS)]
    owner = [o for sl, o in opts for _ in range(sl.stop - sl.start)]
    _assert_same_bits(kind, opt, mine, [[(q, o)] for q, o in zip(few, owner)], f"{kind} {mode}")


@pytest.mark.parametrize("mode", MODES)
def test_many_tensors_accumulate_equals_its_restatement_and_calls_of_at_most_100(mode):
    from pytorch_retinanet_amd.optim import GradAccumulator
    n = 3
    params, _, _ = _make(MANY, mode, seed=13)
    grad_sets = [_grads(params, k) for k in range(n)]
    want = _restated(grad_sets, n)
    acc, acc2 = GradAccumulator(n), GradAccumulator(n)
    _window(acc, params, grad_sets)                                     # (creates the accumulators and the block)
    for k, gs in enumerate(grad_sets):                                  # the same window, each call in groups of at most 100 tensors
        for p, g in zip(params, gs):
            p.grad = g
        assert [acc2.accumulate(params[sl]) for sl in _slices(len(params), 100)] == [100, 100, 30]
        acc2.advance(k == n - 1)
    views, views2 = acc.grad_views(), acc2.grad_views()
    for a in views.values():
        a.fill_(float("nan"))                                           # pos == 0 overwrites: nothing of this survives
    _window(acc, params, grad_sets)
    torch.cuda.synchronize()
    for i, (p, r) in enumerate(zip(params, want)):
        assert torch.equal(views[p], r), (i, p.numel(), float((views[p] - r).abs().max()))
        assert torch.equal(views2[p], r), (i, p.numel())
    assert acc.position == 0 and float(acc.found_inf()) == 0.0
    assert acc.stats() == {"windows": 2, "nonfinite": 0, "micro_batches": 2 * n}


def _carved(sizes, fill, dtype=torch.float32):
    "One sentinel-filled buffer and a 16-byte aligned view of it per size, at least 8 sentinel elements in front of, between and behind them."
    offs, off = [], 8
    for n in sizes:
        offs.append(off)
        off = (off + n + 7) // 8 * 8 + 8
    buf = torch.full((off,), fill, device=DEV, dtype=dtype)
    inside = torch.zeros(off, dtype=torch.bool, device=DEV)
    for o, n in zip(offs, sizes):
        inside[o:o + n] = True
    views = [buf[o:o + n] for o, n in zip(offs, sizes)]
    assert all(v.data_ptr() % 16 == 0 for v in views)
    return buf, inside, views


def _ema_groups(call, tables, sizes, k):
    "``call`` once per group of at most ``k`` tensors: (pointer arrays of the group's slice of every table, its sizes, its length)"
    for sl in _slices(len(sizes), k):
        m = sl.stop - sl.start
        call(*[(C.c_void_p * m)(*[t.data_ptr() if t is not None else 0 for t in tab[sl]]) for tab in tables], (C.c_int64 * m)(*sizes[sl]), m)


@pytest.mark.parametrize("mode", MODES)
def test_many_tensors_ema_update_equals_its_restatement_and_calls_of_at_most_100(mode):
    from pytorch_retinanet_amd._lib import check, lib
    from pytorch_retinanet_amd.optim import WeightEMA
    decay, warmup = 0.9998, 10.0
    params, _, _ = _make(MANY, mode, seed=14)
    masters = [_w(p) for p in params]
    ema = WeightEMA(decay, warmup)
    buf, inside, emas = _carved(MANY, -77.0)
    for p, a in zip(params, emas):
        a.fill_(float("nan"))                                           # the first update overwrites: nothing of this survives
        ema.preallocate(p, a)
    buf2, _, emas2 = _carved(MANY, -77.0)                               # the same updates through the C ABI in groups of at most 100
    block = torch.zeros(8, dtype=torch.float64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    check(lib.rn_ema_set(block.data_ptr(), decay, warmup, 0, stream), "rn_ema_set")
    gen = torch.Generator(device=DEV).manual_seed(15)
    want = [None] * len(params)
    for t in range(3):
        for w in masters:
            w.copy_(torch.randn(w.shape, device=DEV, generator=gen))
        want = [_restate(a, w, t, decay, warmup) for a, w in zip(want, masters)]
        assert ema.update(params) == len(params)
        _ema_groups(lambda e, w, ns, m: check(lib.rn_ema_update(e, w, ns, m, block.data_ptr(), None, stream), "rn_ema_update"),
                    (emas2, masters), MANY, 100)
        check(lib.rn_ema_advance(block.data_ptr(), None, stream), "rn_ema_advance")
        torch.cuda.synchronize()
        for i, (a, b, r) in enumerate(zip(emas, emas2, want)):
            assert torch.equal(a.view(torch.int32), r.view(torch.int32)), (t, i, a.numel(), float((a - r).abs().max()))
            assert torch.equal(b.view(torch.int32), r.view(torch.int32)), (t, i, b.numel())
        assert bool((buf[~inside] == -77.0).all()) and bool((buf2[~inside] == -77.0).all())
    assert ema.stats() == {"updates": 3, "skipped": 0} and int(block.view(torch.int64)[2]) == 3


@pytest.mark.parametrize("mode", MODES)
def test_many_tensors_ema_swap_exchanges_twice_is_identity_and_calls_of_at_most_100(mode):
    from pytorch_retinanet_amd._lib import check, lib
    from pytorch_retinanet_amd.optim import WeightEMA, _dt16
    params, _, dt16 = _make(MANY, mode, seed=16)
    masters = [_w(p) for p in params]
    ema = WeightEMA(0.5)
    ema.update(params)
    gen = torch.Generator(device=DEV).manual_seed(17)
    for p, w in zip(params, masters):
        w.copy_(torch.randn(w.shape, device=DEV, generator=gen))
        if hasattr(p, "master"):
            p.data.copy_(w)
    averages = [ema.average_of(p) for p in params]
    old_w, old_a, old_16 = [w.clone() for w in masters], [a.clone() for a in averages], [p.data.clone() for p in params]
    assert any(not torch.equal(w, a) for w, a in zip(old_w, old_a))
    # the same exchange on copies through the C ABI in groups of at most 100 (sentinels around every copy)
    (wbuf, inside, w2), (abuf, _, a2) = _carved(MANY, -77.0), _carved(MANY, -77.0)
    cbuf, _, c2 = _carved(MANY, 123.0, dt16 or torch.bfloat16)
    for dst, src in zip(w2 + a2, old_w + old_a):
        dst.copy_(src)
    c2 = [c if hasattr(p, "master") else None for c, p in zip(c2, params)]
    stream = torch.cuda.current_stream().cuda_stream
    _ema_groups(lambda e, w, c, ns, m: check(lib.rn_ema_swap(e, w, c, ns, m, _dt16(dt16), stream), "rn_ema_swap"), (a2, w2, c2), MANY, 100)
    ema.swap(params)
    torch.cuda.synchronize()
    for i, (p, w, a, ow, oa) in enumerate(zip(params, masters, averages, old_w, old_a)):
        assert torch.equal(w.view(torch.int32), oa.view(torch.int32)) and torch.equal(a.view(torch.int32), ow.view(torch.int32)), (i, w.numel())
        assert torch.equal(w2[i].view(torch.int32), oa.view(torch.int32)) and torch.equal(a2[i].view(torch.int32), ow.view(torch.int32)), (i, w.numel())
        if hasattr(p, "master"):
            assert torch.equal(p.data, w.to(dt16)) and torch.equal(c2[i], w.to(dt16)), (i, w.numel())
    assert bool((wbuf[~inside] == -77.0).all()) and bool((abuf[~inside] == -77.0).all())
    used16 = torch.zeros_like(inside)
    for c in (c for c in c2 if c is not None):
        o = (c.data_ptr() - cbuf.data_ptr()) // 2
        used16[o:o + c.numel()] = True
    assert bool((cbuf[~used16] == 123.0).all())
    ema.swap(params)
    torch.cuda.synchronize()
    for p, w, a, ow, oa, o16 in zip(params, masters, averages, old_w, old_a, old_16):
        assert torch.equal(w.view(torch.int32), ow.view(torch.int32)) and torch.equal(a.view(torch.int32), oa.view(torch.int32))
        assert torch.equal(p.data, o16)
        if hasattr(p, "master"):
            assert torch.equal(p.data, w.to(dt16))


@pytest.mark.parametrize("mode", MODES)
def test_many_tensors_norm_against_float64_and_bit_equal_over_five_calls(mode):
    """The 230 gradients and one of BIG elements: 231 tensors (224 + 7: the second launch's partial sums start behind the first's) in
    388 chunks.  The norm at test_norm_against_float64's bar, the coefficient bit-equal to GradClip.coef, both bit-equal over five
    calls.  (Not compared with split calls: the order of the sum may depend on the slots.)"""
    from pytorch_retinanet_amd.optim import GradClip
    mine, _, _ = _make(MANY + [BIG], mode, seed=18)
    grads = _grads(mine, 4)
    ref = float(torch.linalg.vector_norm(torch.cat([g.double().flatten() for g in grads])))
    ps = [torch.nn.Parameter(torch.zeros(g.shape, device=DEV)) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = g.float()
    torch_norm = float(torch.nn.utils.clip_grad_norm_(ps, 1e30))
    max_norm = 0.5
    clip = GradClip(max_norm)
    seen = set()
    for _ in range(5):
        total, coef = _norm_call(clip, grads)
        seen.add(clip._block.view(torch.int32)[1:3].cpu().numpy().tobytes())
    err_t, err_k = abs(torch_norm - ref), abs(total - ref)
    bar = max(2.0 * err_t, 16.0 * _ulp(ref))
    print(f"norm[{mode}] float64 {ref!r}: torch fp32 error {err_t:.3e}, kernel error {err_k:.3e}, bar {bar:.3e} (ulp {_ulp(ref):.3e})")
    assert err_k <= bar, (mode, ref, torch_norm, total)
    assert coef < 1.0 and np.float32(coef).tobytes() == np.float32(GradClip.coef(total, max_norm)).tobytes(), (total, coef)
    assert len(seen) == 1
    assert clip.stats() == {"calls": 5, "clipped": 5, "nonfinite": 0}
