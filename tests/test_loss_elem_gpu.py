"""GPU: the loss kernel (K3, csrc/loss.hip) element by element against the float64 restatement of ``loss_elem_ref.py``, at EVERY logit:
every finite fp16 and bf16 bit pattern, an fp32 list (all bf16 values, a 1/256 grid over [-100, 100], random bit patterns, the edges of
the format), constant images that isolate one logit's loss term, the regression branch over the same value lists, and +-Inf logits.

``matches``, ``num_fg`` and the flag words are built by hand (``loss_elem_ref.sweep_roles``): the matcher is not under test and is not
called.  Every output lies in an allocation whose tail is a guard pattern that must come back untouched, and starts as a NaN pattern
(0xFF bytes), so an element the kernel did not write shows.  The library is called through its C entry points -- ``_ex`` (finalize
launch), ``_fin`` (in-kernel finalize) and ``_rp`` (the three forms, and the gradient prescale) -- as ``ops.loss_fwd_bwd_levels`` calls
them, with the test's own output buffers.

Tolerances are the derived bounds of ``loss_elem_ref.py`` (written out there, step by step from bg_elem / focal_elem / reg_row) plus
half a unit in the last place of the output dtype; there is no free relative tolerance and no factor fitted to a measurement.  Elements
whose reference magnitude falls under the smallest normal fp32 along the kernel's chain of products ("under the floor") must have the
right sign or be zero and stay under twice the floor; they are counted, and must lie in the logit region the derivation predicts.

Loss sums: element bounds added up + n u sum|terms| for the longest fp32 addition chain (``chain_length``: a lane adds the PF * VEC =
8 (fp32) or 16 (16-bit) terms of a group in fp32; everything between groups is double; wave sums and the total are rounded to fp32
once each: n = 14 / 22 -- "a few dozen" at most, whatever the shape) + the 2^-32 fixed point of the workgroup partials.  Where the
terms leave the range of that arithmetic -- a lane's group can exceed FLT_MAX, or the |terms| add up to 2^31, the fixed point's range --
the sum may be +Inf or NaN (bf16 and fp32 sweeps hold logits up to 3.4e38): then only the gradients are checked in that launch.

Largest measured err / (bound + half ulp) on the MI355X (256 CUs) and, in brackets, the elements under the floor summed over a test's
launches.  The four configurations (chunks through ``_ex``, chunks through ``_fin``, list, repair pass) gave the same figures to three
digits in every row, so one column stands for all; the bound was not scaled to any of them:
  class gradients, sweeps     f16 1.000 [104 514]   f16 with prescale 2^14 0.999 [102 664]   bf16 0.999 [142 087]
                              f32 K = 8 0.511 [355 165]   f32 K = 3 0.506 [157 939]   (16 bit: nearly all of it is the output rounding)
  class gradients, per logit  f32 0.197 [4 029]   bf16 0.986   f16 0.954   f32 gamma = 0: 0.299 [504]   f32 gamma = 1.5: 0.178 [3 022]
  class loss sums             f16 sweeps 0.036 (3 images: 0.046); bf16 / f32 sweeps: no finite sum (logits up to 3.4e38, see above);
                              per logit f32 0.124, bf16 / f16 0.075, gamma = 0: 0.270, gamma = 1.5: 0.075
  box gradients               beta = 0.1: f16 0.986  bf16 0.972  f32 0.285;  beta = 0: f16 0.613  bf16 0.327  f32 0.083; signs left out at
                              beta = 0: 1 of 86 088 (f16), 0 (bf16, f32)
  regression sums             f16 0.039 (repair pass 0.043) at beta = 0.1, 0.035 at beta = 0; bf16 / f32: no finite sum
One derivation step was corrected by the first run (gamma = 0, logit -90): below z = -80 bg_elem computes the element AT the clamp, so a
background gradient under the floor may be as large as its value there (``loss_elem_ref.cls_floor``).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import loss_elem_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096
FMT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
VEC = {"f32": 4, "bf16": 8, "f16": 8}
FLT_MAX = float(np.finfo(np.float32).max)
CHUNKS, REPAIR, LIST = 0, 1, 2
# (name, form, entry point)
CONFIGS = [("chunks", CHUNKS, "ex"), ("chunks+fin", CHUNKS, "fin"), ("list", LIST, "rp"), ("repair", REPAIR, "rp")]
CONFIGS_PRESCALE = [("chunks", CHUNKS, "rp"), ("list", LIST, "rp"), ("repair", REPAIR, "rp")]


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


class _Out:
    "An output of ``n`` elements of ``dtype`` inside an allocation of 0xFF bytes (a NaN in all three formats) with a GUARD-byte tail."

    def __init__(self, n: int, dtype):
        self.n, self.dtype, self.nbytes = n, dtype, n * torch.empty((), dtype=dtype).element_size()
        self.buf = torch.empty((self.nbytes + GUARD,), dtype=torch.uint8, device=DEV)

    def reset(self):
        self.buf.fill_(0xFF)
        return self.buf.data_ptr()

    def take(self, what: str) -> np.ndarray:
        assert bool((self.buf[self.nbytes:] == 0xFF).all()), f"{what}: written behind its end"
        got = self.buf[:self.nbytes].view(self.dtype).to(torch.float64).cpu().numpy()
        return got


class _Problem:
    """One K3 problem on the device: head outputs of ``fmt`` ([B,A,K], [B,A,4] float32 arrays holding representable values), the GT
    arrays and hand-made match results; ``launch`` runs one entry point into guarded outputs and returns (loss[2], gcls, gbox) float64."""

    def __init__(self, fmt, cls, box, anchors, gt_boxes, gt_labels, gt_off, matches, num_fg, special, params):
        from pytorch_retinanet_amd import ops
        self.fmt, (self.B, self.A, self.K) = fmt, cls.shape
        dt = FMT[fmt]
        self.cls, self.box = _dev(cls, dt), _dev(box, dt)
        assert np.array_equal(self.cls.float().cpu().numpy(), cls, equal_nan=True), "the logits must be representable in the I/O dtype"
        self.anchors, self.gt_boxes = _dev(anchors.astype(np.float32)), _dev(np.asarray(gt_boxes, dtype=np.float32).reshape(-1, 4))
        self.gt_labels, self.gt_off = _dev(np.asarray(gt_labels, dtype=np.int64)), _dev(np.asarray(gt_off, dtype=np.int32))
        self.matches, self.num_fg = _dev(matches.astype(np.int64)), _dev(np.asarray(num_fg, dtype=np.int32))
        self.special = _dev(special.view(np.int64))
        assert tuple(self.special.shape) == (self.B, (self.A + 63) // 64)
        self.params = params
        self.g_cls, self.g_box, self.loss = _Out(self.B * self.A * self.K, dt), _Out(self.B * self.A * 4, dt), _Out(2, torch.float32)
        self.state = ops.new_match_state(torch.device(DEV))

    def set_matches(self, matches, num_fg, special, gt_labels=None, gt_off=None):
        self.matches.copy_(_dev(matches.astype(np.int64)))
        self.num_fg.copy_(_dev(np.asarray(num_fg, dtype=np.int32)))
        self.special.copy_(_dev(special.view(np.int64)))
        if gt_labels is not None:
            self.gt_labels.copy_(_dev(np.asarray(gt_labels, dtype=np.int64)))
        if gt_off is not None:
            self.gt_off.copy_(_dev(np.asarray(gt_off, dtype=np.int32)))

    def launch(self, form: int, entry: str, prescale=None, with_special: bool = True):
        from pytorch_retinanet_amd._lib import lib, check, RN_F32, RN_BF16, RN_F16
        code = {"f32": RN_F32, "bf16": RN_BF16, "f16": RN_F16}[self.fmt]
        arr = lambda p: (C.c_void_p * 1)(p)
        ws_bytes = int(lib.rn_loss_workspace_bytes(self.B, self.A, self.K))
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=DEV)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        head = (arr(self.cls.data_ptr()), arr(self.box.data_ptr()), (C.c_int64 * 1)(self.A), 1, code, self.B, self.K, self.anchors.data_ptr(),
                0, self.gt_boxes.data_ptr(), self.gt_labels.data_ptr(), self.gt_off.data_ptr(), self.matches.data_ptr(),
                self.special.data_ptr() if with_special else None, self.num_fg.data_ptr(), C.byref(self.params))
        tail = (self.loss.reset(), arr(self.g_cls.reset()), arr(self.g_box.reset()), ws.data_ptr(), ws_bytes)
        if entry == "ex":
            assert form == CHUNKS and prescale is None
            check(lib.rn_loss_fwd_bwd_levels_ex(*head, *tail, stream, None, None), "rn_loss_fwd_bwd_levels_ex")
        elif entry == "fin":
            assert form == CHUNKS and prescale is None
            check(lib.rn_loss_fwd_bwd_levels_fin(*head, *tail, self.state.data_ptr(), stream, None, None), "rn_loss_fwd_bwd_levels_fin")
        else:
            check(lib.rn_loss_fwd_bwd_levels_rp(*head, None if prescale is None else prescale.data_ptr(), form, *tail, self.state.data_ptr(),
                                                stream, None, None), "rn_loss_fwd_bwd_levels_rp")
        torch.cuda.synchronize()
        return (self.loss.take("loss"), self.g_cls.take("grad_cls").reshape(self.B, self.A, self.K),
                self.g_box.take("grad_box").reshape(self.B, self.A, 4))


def _params(gamma=2.0, beta=0.1):
    from pytorch_retinanet_amd import ops
    return ops.make_loss_params(0.25, gamma, beta)


def _n_partials(B, A, K, vec):
    "Workgroup partials of a launch: at most one per 4 waves of 128 vectors, plus the repair kernel's (4 strips of 512 rows each)."
    return -(-(B * A * K // vec + 1) // 512) + -(-B * -(-A // 512) // 4) + 1


class _Stats:
    "Largest err / (bound + half ulp) and the floor counts of one test, per configuration; printed, so a run can be recorded."

    def __init__(self, what):
        self.what, self.ratio, self.floor, self.sum_ratio, self.sums = what, {}, {}, {}, {}

    def grad(self, name, ratio, n_floor):
        self.ratio[name] = max(self.ratio.get(name, 0.0), ratio)
        self.floor[name] = self.floor.get(name, 0) + n_floor

    def total(self, name, ratio):
        self.sum_ratio[name] = max(self.sum_ratio.get(name, 0.0), ratio)
        self.sums[name] = self.sums.get(name, 0) + 1

    def report(self):
        for name in self.ratio:
            print(f"RATIO {self.what} [{name}]: grad err/bound {self.ratio[name]:.3f}, under the floor {self.floor[name]}, "
                  f"sum err/bound {self.sum_ratio.get(name, float('nan')):.3f} over {self.sums.get(name, 0)} finite sums")


def _check_cls(got, r, fmt, what):
    "Every class gradient against the reference ``r``; -> (largest err / (bound + half ulp), elements under the floor)."
    assert not np.isnan(got).any(), f"{what}: {int(np.isnan(got).sum())} gradient elements were not written (or are NaN)"
    dead = np.broadcast_to(r.dead[:, :, None], got.shape)
    assert not got[dead].any(), f"{what}: ignored rows and images without GT must be exactly zero"
    fl, lim = R.cls_floor(r)
    assert R.floor_region(r)[fl].all(), f"{what}: an element under the floor lies outside the predicted logit region"
    bound = R.cls_grad_bound(r)
    bound = bound + R.half_ulp(np.abs(r.gcls) + bound, fmt)
    err = np.abs(got - r.gcls)
    ok = ~fl & ~dead
    ratio = float((err[ok] / bound[ok]).max())
    if ratio > 1.0:
        i = np.unravel_index(np.argmax(np.where(ok, err / np.where(bound > 0, bound, 1.0), 0.0)), got.shape)
        raise AssertionError(f"{what}: class gradient err / bound = {ratio:.3f} at {i}: z = {r.z[i]!r}, positive = {bool(r.pos[i])}, "
                             f"got {got[i]!r}, want {r.gcls[i]!r}, bound {bound[i]!r}")
    lim = lim + R.half_ulp(lim, fmt)
    with np.errstate(invalid="ignore"):
        bad = fl & ((np.abs(got) > lim) | (got * np.where(r.pos, -1.0, 1.0) < 0))
    assert not bad.any(), f"{what}: {int(bad.sum())} elements under the floor have the wrong sign or exceed twice the floor"
    return ratio, int(fl.sum())


def _check_cls_sum(got: float, r, fmt, what):
    "The class loss sum; -> err / bound, or None where the terms leave the range of the kernel's sums (see the module docstring)."
    vec = VEC[fmt]
    live = ~np.broadcast_to((r.scale == 0)[:, None, None], r.z.shape)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        foc = np.ones_like(r.p) if r.params.gamma == 0.0 else r.p ** r.params.gamma
        bg_raw = np.where(live, foc * R.softplus(r.z), 0.0)                       # what phase A adds for EVERY element
        bg = bg_raw * r.params.alpha * r.scale[:, None, None]
        terms = np.abs(bg).sum() + np.abs(r.term[r.pos]).sum()
        top = np.sort(bg_raw.reshape(-1))[-R.PF * vec:].sum()                     # the most one lane's group can hold
    assert not np.isnan(got) or not np.isfinite(terms) or top >= FLT_MAX or terms >= 2.0 ** 31, f"{what}: the class loss is NaN"
    if not np.isfinite(terms) or top >= FLT_MAX or terms >= 2.0 ** 31:
        assert not np.isfinite(got) or got >= 0.0, f"{what}: class loss {got!r}"
        return None
    tf, tb = R.term_floor(r)
    eb = np.where(tf, tb, R.cls_term_bound(r))
    bound = R.sum_bound(eb, terms, R.chain_length(vec), _n_partials(r.B, r.A, r.K, vec))
    ratio = abs(got - r.loss_cls) / bound
    assert ratio <= 1.0, f"{what}: class loss {got!r}, want {r.loss_cls!r}: err / bound = {ratio:.3f} (bound {bound!r})"
    return ratio



# ---------------------------------------------------------------- (a) - (c): the sweeps of the class branch
def _sweep(fmt, K, values, configs, stats, prescale=1.0, dead_image=False, seed=3):
    """``values`` (float32, representable in ``fmt``) in a seeded permutation through cls [2, 4099, K] (a third image without GT with
    ``dead_image``), as many tensors as it takes, each through the K + 2 launches of the role rotation and every configuration; the
    reference of a launch is computed once and shared by the configurations.  Fails unless every value has been a background element, a
    positive element and an element of an ignored row at least once."""
    B, A = (3 if dead_image else 2), 4099
    per = 2 * A * K
    perm = np.random.default_rng(seed).permutation(values.size)
    anchors, gt = R.sweep_anchors(A), np.concatenate([R.sweep_gt()] * 2)
    gt_off = [0, 8, 16] + ([16] if dead_image else [])
    pres = None if prescale == 1.0 else _dev(np.array([prescale], dtype=np.float32))
    box = np.random.default_rng(seed + 1).normal(0, 0.5, (B, A, 4)).astype(np.float32).astype(np.float16).astype(np.float32)   # (exact in all three)
    seen = np.zeros((3, values.size), dtype=np.int64)                               # background / positive / ignored
    pref = R.Params.of(_params())
    for c0 in range(0, values.size, per):
        idx = perm[c0:c0 + per]
        flat = np.zeros(per, dtype=np.float32)
        flat[:idx.size] = values[idx]
        cls = flat.reshape(2, A, K)
        if dead_image:
            cls = np.concatenate([cls, cls[:1]])
        prob = None
        for j in range(K + 2):
            m, nf, lab, sp = R.sweep_roles(B, A, K, j)
            if prob is None:
                prob = _Problem(fmt, cls, box, anchors, gt, lab[:16], gt_off, m, nf, sp, _params())
            else:
                prob.set_matches(m, nf, sp)
            r = R.reference(cls, box, anchors, gt, lab[:16], gt_off, m, nf, pref, prescale)
            if dead_image:
                assert r.dead[2].all() and r.scale[2] == 0
            role = np.where(r.pos[:2], 1, np.where(r.dead[:2, :, None], 2, 0)).reshape(-1)[:idx.size]
            for k in range(3):
                np.add.at(seen[k], idx[role == k], 1)
            for name, form, entry in configs:
                what = f"{fmt} K={K} tensor {c0 // per} launch {j} {name}" + (f" prescale {prescale}" if pres is not None else "")
                loss, gc, gb = prob.launch(form, entry, pres, with_special=(entry != "ex" or j % 2 == 0))
                ratio, n_floor = _check_cls(gc, r, fmt, what)
                stats.grad(name, ratio, n_floor)
                sr = _check_cls_sum(float(loss[0]), r, fmt, what)
                if sr is not None:
                    stats.total(name, sr)
                assert not gb[~r.matched].any() and not np.isnan(gb).any(), f"{what}: box gradient rows"
    missed = (seen == 0).sum(1)
    assert not missed.any(), f"values that never were background / positive / ignored: {missed.tolist()}"
    print(f"COVERAGE {fmt} K={K}: {values.size} values, least visits as background / positive / ignored: {seen.min(1).tolist()}")


@pytest.mark.parametrize("fmt", ["f16", "bf16"])
def test_class_gradients_at_every_16bit_logit(fmt):
    "(a, b) every finite bit pattern of the dtype in every role, every form; the third image without GT rides along in the list form."
    stats = _Stats(f"sweep {fmt}")
    v = R.finite_patterns(fmt)
    assert v.size == (63488 if fmt == "f16" else 65280)
    _sweep(fmt, 8, v, CONFIGS, stats)
    _sweep(fmt, 8, v, [("list, 3 images", LIST, "rp")], stats, dead_image=True)
    stats.report()


def test_class_gradients_at_every_fp16_logit_with_a_prescale():
    "(a) fp16 once more with grad_prescale = 2^14: the small gradients are representable, so they are compared instead of flushed."
    stats = _Stats("sweep f16 prescale 2^14")
    _sweep("f16", 8, R.finite_patterns("f16"), CONFIGS_PRESCALE, stats, prescale=2.0 ** 14)
    stats.report()


@pytest.mark.parametrize("K", [8, 3])
def test_class_gradients_over_the_fp32_list(K):
    "(c) all bf16 values, the 1/256 grid over [-100, 100], 20 000 random bit patterns and the edges of fp32; K = 3 is narrower than a vector."
    stats = _Stats(f"sweep f32 K={K}")
    _sweep("f32", K, R.f32_sweep_values(), CONFIGS, stats)
    stats.report()


# ---------------------------------------------------------------- (d): per-logit loss values
LOGITS = [-90.0, -80.0, -79.0, -60.0, -44.0, -40.0, -30.0, -29.0, -20.0, -15.0, -10.0, -7.0, -4.6, -3.6, -2.0, -1.0, -0.5, 0.0, 0.5, 1.0,
          2.0, 3.6, 5.0, 7.0, 10.0, 15.0, 20.0, 30.0, 45.0, 60.0, 80.0, 90.0]


@pytest.mark.parametrize("fmt,gamma", [("f32", 2.0), ("bf16", 2.0), ("f16", 2.0), ("f32", 0.0), ("f32", 1.5)])
def test_loss_term_of_each_logit(fmt, gamma):
    """(d) cls [32, 64, 8]: image i holds the constant logit LOGITS[i]; launch i gives image i alone a GT box (equal to one anchor, matched
    by hand, num_fg = 1; one more row ignored), so the returned sum is that image's: 510 background terms and one positive term of ONE
    logit -- a systematic per-element bias cannot average out.  Chains: 512 elements per image are one group of one wave in fp32
    (8 fp32 additions per lane), and in 16 bit a group spans two images and every term is added in double: no fp32 chain is longer
    than ``chain_length`` (14 / 22).  The gradients of image i are checked too (gamma != 2: __powf)."""
    assert len(LOGITS) == 32
    B, A, K = 32, 64, 8
    vals = torch.tensor(LOGITS, dtype=torch.float32).to(FMT[fmt]).float().numpy()
    cls = np.broadcast_to(vals[:, None, None], (B, A, K)).copy()
    anchors = R.sweep_anchors(A)
    box = np.random.default_rng(4).normal(0, 0.5, (B, A, 4)).astype(np.float32).astype(np.float16).astype(np.float32)
    params = _params(gamma)
    pref = R.Params.of(params)
    stats = _Stats(f"per-logit {fmt} gamma={gamma}")
    prob = None
    for i in range(B):
        r0, r1 = (7 * i) % A, (7 * i + 13) % A
        m = np.full((B, A), -1, dtype=np.int64)
        m[i, r0], m[i, r1] = 0, -2
        gt, lab, off = anchors[r0:r0 + 1], [1 + i % K], [0] * (i + 1) + [1] * (B - i)
        nf, sp = np.ones(B, dtype=np.int32), R.special_words(m)
        if prob is None:
            prob = _Problem(fmt, cls, box, anchors, gt, lab, off, m, nf, sp, params)
        else:
            prob.gt_boxes.copy_(_dev(gt))
            prob.set_matches(m, nf, sp, lab, off)
        r = R.reference(cls, box, anchors, gt, lab, off, m, nf, pref)
        assert r.pos.sum() == 1 and (r.scale > 0).sum() == 1 and r.pos[i, r0, i % K]
        for name, form, entry in CONFIGS:
            what = f"{fmt} gamma={gamma} logit {vals[i]} {name}"
            loss, gc, gb = prob.launch(form, entry)
            ratio, n_floor = _check_cls(gc, r, fmt, what)
            stats.grad(name, ratio, n_floor)
            sr = _check_cls_sum(float(loss[0]), r, fmt, what)
            assert sr is not None, what
            stats.total(name, sr)
            print(f"TERM {what}: sum {float(loss[0])!r} want {r.loss_cls!r} err/bound {sr:.3f}")
    stats.report()


# ---------------------------------------------------------------- (e): the regression branch
@pytest.mark.parametrize("beta", [0.1, 0.0])
@pytest.mark.parametrize("fmt", ["f16", "bf16", "f32"])
def test_box_gradients_at_every_prediction(fmt, beta):
    """(e) box [2, 4099, 4]: the matched rows' predictions run through every finite 16-bit pattern (fp32: the list of the class sweep)
    against GT / anchor pairs whose targets have both signs and all sizes (gw / aw from 0 to 40); every gradient element and the
    regression sum; unmatched rows exactly zero.  beta = 0: signs the reference cannot decide are left out, at most 0.1 %."""
    values = R.f32_sweep_values() if fmt == "f32" else R.finite_patterns(fmt)
    B, A, K = 2, 4099, 8
    anchors, gt = R.sweep_anchors(A), np.concatenate([R.sweep_gt()] * B)
    lab, off = np.tile(np.arange(1, 9), 2), [0, 8, 16]
    cls = np.full((B, A, K), -4.625, dtype=np.float32)
    params = _params(2.0, beta)
    pref = R.Params.of(params)
    stats = _Stats(f"box {fmt} beta={beta}")
    n_parts = R.box_problem(values, 0)[3]
    left_out = total = 0
    for part in range(n_parts):
        box, m, nf, _ = R.box_problem(values, part)
        prob = _Problem(fmt, cls, box, anchors, gt, lab, off, m, nf, R.special_words(m), params)
        r = R.reference(cls, box, anchors, gt, lab, off, m, nf, pref)
        bound, und = R.box_grad_bound(r)
        bound = bound + R.half_ulp(np.abs(r.gbox) + bound, fmt)
        m4 = np.broadcast_to(r.matched[:, :, None], r.d.shape)
        left_out, total = left_out + int(und.sum()), total + int(m4.sum())
        with np.errstate(over="ignore"):
            raw = np.abs(r.d) if beta < 1e-5 else np.where(np.abs(r.d) < pref.beta, 0.5 * r.d * r.d / pref.beta, np.abs(r.d) - 0.5 * pref.beta)
            raw = np.where(m4, raw, 0.0)
            terms = float(np.abs(r.term_box).sum())
            wide = np.sort(raw.reshape(-1))[-4:].sum() >= FLT_MAX or terms >= 2.0 ** 31
        for name, form, entry in CONFIGS:
            what = f"box {fmt} beta={beta} part {part} {name}"
            loss, gc, gb = prob.launch(form, entry)
            assert not np.isnan(gb).any(), f"{what}: box gradient elements were not written"
            assert not gb[~m4].any(), f"{what}: unmatched rows must be exactly zero"
            ok = m4 & ~und
            ratio = float((np.abs(gb - r.gbox)[ok] / bound[ok]).max())
            assert ratio <= 1.0, f"{what}: box gradient err / bound = {ratio:.3f}"
            stats.grad(name, ratio, 0)
            if wide:
                assert not np.isfinite(loss[1]) or loss[1] >= 0.0
            else:
                sb = R.sum_bound(R.box_term_bound(r), terms, R.REG_CHAIN, _n_partials(B, A, K, VEC[fmt]))
                sr = abs(float(loss[1]) - r.loss_reg) / sb
                assert sr <= 1.0, f"{what}: regression loss {float(loss[1])!r}, want {r.loss_reg!r}: err / bound = {sr:.3f}"
                stats.total(name, sr)
    assert left_out <= 1e-3 * total, f"{left_out} of {total} signs undecidable"
    print(f"LEFT OUT box {fmt} beta={beta}: {left_out} of {total}")
    stats.report()


# ---------------------------------------------------------------- (f): +-Inf logits
@pytest.mark.parametrize("fmt", ["f32", "bf16", "f16"])
def test_infinite_background_logits(fmt):
    """(f) A +Inf background logit: class loss +Inf, the finite gradient alpha * scale at that element, every other element unchanged.
    A -Inf background logit (z is clamped at -80 in bg_elem): gradient exactly 0, a finite loss -- the sum without that element."""
    B, A, K = 2, 259, 8
    rng = np.random.default_rng(6)
    cls = torch.tensor(rng.normal(-2.0, 2.0, (B, A, K)), dtype=torch.float32).to(FMT[fmt]).float().numpy()
    box = rng.normal(0, 0.5, (B, A, 4)).astype(np.float32).astype(np.float16).astype(np.float32)
    anchors, gt = R.sweep_anchors(A), np.concatenate([R.sweep_gt()] * B)
    m, nf, lab, sp = R.sweep_roles(B, A, K, 0)
    off = [0, 8, 16]
    params = _params()
    pref = R.Params.of(params)
    at = (1, int(np.nonzero(m[1] == -1)[0][5]), 5)                                  # an element of a background row
    for name, form, entry in CONFIGS:
        base = _Problem(fmt, cls, box, anchors, gt, lab[:16], off, m, nf, sp, params).launch(form, entry)
        for inf in (np.inf, -np.inf):
            c2 = cls.copy()
            c2[at] = inf
            loss, gc, gb = _Problem(fmt, c2, box, anchors, gt, lab[:16], off, m, nf, sp, params).launch(form, entry)
            r = R.reference(c2, box, anchors, gt, lab[:16], off, m, nf, pref)
            what = f"{fmt} {name} logit {inf}"
            others = np.ones(gc.shape, dtype=bool)
            others[at] = False
            assert np.array_equal(gc[others], base[1][others]) and np.array_equal(gb, base[2]) and loss[1] == base[0][1], what
            if inf > 0:
                assert loss[0] == np.inf, f"{what}: class loss {loss[0]!r}"
                want = pref.alpha / (float(nf[1]) * B)
                assert abs(gc[at] - want) <= (R.GMUL_U + 2) * R.U * want + R.half_ulp(want, fmt), f"{what}: gradient {gc[at]!r}, want {want!r}"
            else:
                assert gc[at] == 0.0 and np.isfinite(loss[0]), f"{what}: gradient {gc[at]!r}, class loss {loss[0]!r}"
                sr = _check_cls_sum(float(loss[0]), r, fmt, what)
                assert sr is not None and r.term[at] == 0.0
