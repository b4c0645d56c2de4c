"""CPU tests of tests/loss_elem_ref.py, the float64 restatement of the loss kernel that test_loss_elem_gpu.py measures K3 against:
against the C oracle (within the oracle's own fp32 accuracy), against float64 torch autograd of the formula written directly,
against the asymptotics worked out by hand, and -- with an fp32 re-enactment of bg_elem / focal_elem in correctly rounded numpy
operations -- a check that the derived bounds are not already broken by arithmetic that is BETTER than the hardware's."""
import numpy as np
import pytest
import torch

import loss_elem_ref as R
import synth


# ---------------------------------------------------------------- against the C oracle
@pytest.mark.parametrize("A,K,B,gamma,beta", [(777, 3, 3, 2.0, 0.1), (1001, 7, 2, 1.5, 0.0)])
def test_reference_against_the_oracle(oracle_lib, A, K, B, gamma, beta):
    "Shapes, parameters and tolerances of test_hip_parity.test_loss_ragged_shapes_and_params: the oracle's peer is held to what its peer is."
    rng = np.random.default_rng(5)
    anc = np.sort(rng.uniform(0, 300, (A, 2, 2)).astype(np.float32), axis=1).reshape(A, 4)
    cls, box = synth.head_outputs(rng, B, A, K, cls_mean=-1.0, cls_std=2.0, box_std=0.5)
    gtb, gtl = zip(*[synth.gt_boxes(rng, 6, 300, 300, num_classes=K, wh_lo=30, wh_hi=200) for _ in range(B)])
    m, nf = oracle_lib.iou_match(anc, list(gtb))
    assert (m >= 0).sum() > 10
    po = oracle_lib.default_loss_params(0.25, gamma, beta)
    o = oracle_lib.loss_fwd_bwd(cls, box, anc, list(gtb), list(gtl), m, po)
    off = np.concatenate([[0], np.cumsum([len(g) for g in gtb])])
    r = R.reference(cls, box, anc, np.concatenate(gtb), np.concatenate(gtl), off, m, nf, R.Params.of(po))
    tol = dict(rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose([r.loss_cls, r.loss_reg], o["loss"], **tol)
    np.testing.assert_allclose(r.gcls, o["gcls"], **tol)
    np.testing.assert_allclose(r.gbox, o["gbox"], **tol)


# ---------------------------------------------------------------- against float64 autograd
def _autograd(cls, box, anc, gtb, gtl, off, m, nf, p: R.Params):
    B, A, K = cls.shape
    x = torch.tensor(cls, dtype=torch.float64, requires_grad=True)
    y = torch.tensor(box, dtype=torch.float64, requires_grad=True)
    total_c = total_r = 0.0
    for b in range(B):
        T = int(off[b + 1] - off[b])
        if T == 0:
            continue
        z = x[b] + p.logit_shift
        keep = torch.tensor(m[b] != -2)
        fg = torch.tensor(m[b] >= 0)
        t = torch.zeros((A, K), dtype=torch.float64)
        rows = np.nonzero(m[b] >= 0)[0]
        lab = gtl[off[b] + m[b][rows]] - 1
        t[rows, lab] = 1.0
        bce = -(t * torch.nn.functional.logsigmoid(z) + (1 - t) * torch.nn.functional.logsigmoid(-z))
        q = torch.where(t > 0, torch.sigmoid(-z), torch.sigmoid(z))
        w = (torch.where(t > 0, torch.tensor(p.alpha_pos, dtype=torch.float64), torch.tensor(p.alpha, dtype=torch.float64))
             * (q ** p.gamma if p.gamma else torch.ones_like(q))).detach()
        total_c = total_c + (w * bce)[keep].sum() / max(int(nf[b]), 1) / B
        g = torch.tensor(gtb[off[b] + np.maximum(m[b], 0)], dtype=torch.float64)
        a = torch.tensor(anc, dtype=torch.float64)
        aw, ah = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
        tgt = torch.stack([((g[:, 0] + g[:, 2]) / 2 - (a[:, 0] + a[:, 2]) / 2) / aw * p.reg_w[0],
                           ((g[:, 1] + g[:, 3]) / 2 - (a[:, 1] + a[:, 3]) / 2) / ah * p.reg_w[1],
                           torch.log((g[:, 2] - g[:, 0]) / aw + p.log_eps) * p.reg_w[2],
                           torch.log((g[:, 3] - g[:, 1]) / ah + p.log_eps) * p.reg_w[3]], 1)
        n = (y[b] - tgt).abs()
        l = n if p.beta < 1e-5 else torch.where(n < p.beta, 0.5 * n * n / p.beta, n - 0.5 * p.beta)
        total_r = total_r + l[fg].sum() / max(int(nf[b]), 1) / B
    gx, gy = torch.autograd.grad(total_c + total_r, [x, y])
    return float(total_c.detach()), float(total_r.detach()), gx.numpy(), gy.numpy()


@pytest.mark.parametrize("gamma,beta", [(2.0, 0.1), (1.5, 0.0), (0.0, 0.5)])
def test_reference_against_float64_autograd(gamma, beta):
    "Logits spanning [-100, 100], box residuals on both sides of beta, an image without GT, ignored rows: to about 1e-12."
    rng = np.random.default_rng(11)
    B, A, K = 3, 301, 5
    anc = R.sweep_anchors(A)
    gtb = np.concatenate([R.sweep_gt(), R.sweep_gt()[::-1]]).astype(np.float64)
    gtl = rng.integers(1, K + 1, 16)
    off = np.array([0, 8, 8, 16])
    m = rng.integers(-2, 8, (B, A))
    nf = (m >= 0).sum(1)
    cls = rng.uniform(-100, 100, (B, A, K))
    p = R.Params.make(0.25, gamma, beta)
    r0 = R.reference(cls, np.zeros((B, A, 4)), anc, gtb, gtl, off, m, nf, p)
    box = r0.tgt + rng.choice([-3.0, -0.5, -0.01, 0.01, 0.5, 3.0], (B, A, 4)) * max(beta, 0.1) * rng.uniform(0.5, 1.5, (B, A, 4))
    r = R.reference(cls, box, anc, gtb, gtl, off, m, nf, p, prescale=1.0)
    lc, lr, gx, gy = _autograd(cls, box, anc.astype(np.float64), gtb, gtl, off, m, nf, p)
    np.testing.assert_allclose([r.loss_cls, r.loss_reg], [lc, lr], rtol=1e-12)
    np.testing.assert_allclose(r.gcls, gx, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(r.gbox, gy, rtol=1e-12, atol=1e-300)
    assert not r.gcls[1].any() and not r.gbox[1].any() and not r.gcls[m == -2].any()
    r2 = R.reference(cls, box, anc, gtb, gtl, off, m, nf, p, prescale=2.0 ** 14)
    assert np.array_equal(r2.gcls, r.gcls * 2.0 ** 14) and np.array_equal(r2.gbox, r.gbox * 2.0 ** 14) and r2.loss_cls == r.loss_cls


# ---------------------------------------------------------------- asymptotics by hand
def _one(x, pos, gamma=2.0, nf=3):
    "One image of one row of one class, logit x; matched to a GT box of label 1 when ``pos``."
    p = R.Params.make(0.25, gamma, 0.1)
    m = np.array([[0 if pos else -1]])
    return R.reference(np.array([[[x]]]), np.zeros((1, 1, 4)), R.sweep_anchors(1), R.sweep_gt()[:1], [1], [0, 1], m, [nf], p), 1.0 / nf


def test_reference_asymptotics():
    r, s = _one(60.0, False)
    assert r.gcls[0, 0, 0] == pytest.approx(0.25 * s, rel=1e-15)                                  # background, z -> +inf: alpha * scale
    assert r.term[0, 0, 0] == pytest.approx(0.25 * s * 61.0, rel=1e-15)                           # ... and the term alpha * scale * z
    for x in (-30.0, -60.0, -100.0):
        r, s = _one(x, False)
        assert r.gcls[0, 0, 0] == pytest.approx(0.25 * s * np.exp(3 * (x + 1.0)), rel=1e-12)      # z -> -inf: alpha * scale * e^{3z}
        assert r.term[0, 0, 0] == pytest.approx(0.25 * s * np.exp(3 * (x + 1.0)), rel=1e-12)      # bce ~ e^z too
        r, s = _one(x, True)
        assert r.gcls[0, 0, 0] == pytest.approx(-0.75 * s, rel=1e-12)                             # positive, z -> -inf: -(1 - alpha) * scale
        assert r.term[0, 0, 0] == pytest.approx(0.75 * s * -(x + 1.0), rel=1e-12)
    r, s = _one(0.0 - 1.0, False, gamma=1.5)                                                      # z = 0: p = 1/2
    assert r.gcls[0, 0, 0] == pytest.approx(0.25 * s * 0.5 ** 2.5, rel=1e-15)
    r, _ = _one(np.inf, False)
    assert r.term[0, 0, 0] == np.inf and r.loss_cls == np.inf and r.gcls[0, 0, 0] == pytest.approx(0.25 / 3)
    r, _ = _one(-np.inf, False)
    assert r.term[0, 0, 0] == 0.0 and r.gcls[0, 0, 0] == 0.0


def test_half_ulp_and_special_words():
    assert R.half_ulp(1.0, "f32") == 2.0 ** -24 and R.half_ulp(1.5, "f16") == 2.0 ** -11 and R.half_ulp(3.9, "bf16") == 2.0 ** -7
    assert R.half_ulp(0.0, "f16") == 2.0 ** -25 and R.half_ulp(1e-6, "f16") == 2.0 ** -25 and R.half_ulp(1e-40, "f32") == 2.0 ** -150
    m = np.full((2, 130), -1)
    m[0, 0], m[0, 63], m[1, 64], m[1, 129] = 3, -2, 0, -2
    w = R.special_words(m)
    assert w.shape == (2, 3) and w[0].tolist() == [1 | 1 << 63, 0, 0] and w[1].tolist() == [0, 1, 2]


def test_role_rotation_covers_every_element_in_every_role():
    for K in (8, 3):
        B, A = 2, 4099
        pos, ign, bg = (np.zeros((B, A, K), dtype=int) for _ in range(3))
        for j in range(K + 2):
            m, nf, lab, sp = R.sweep_roles(B, A, K, j)
            code = np.where(m >= 0, lab.reshape(B, 8)[np.arange(B)[:, None], np.maximum(m, 0)] - 1, -1)
            onehot = code[:, :, None] == np.arange(K)
            pos += onehot
            ign += (m == -2)[:, :, None]
            bg += (m != -2)[:, :, None] & ~onehot
            assert np.array_equal(nf, (m >= 0).sum(1)) and (m >= 0).any() and (m == -1).any() and len(set(lab[:8])) == K
        assert (pos == 1).all() and (ign == 1).all() and (bg == K).all()


# ---------------------------------------------------------------- the bounds against an fp32 re-enactment
def _f(x):
    return np.asarray(x, dtype=np.float32)


def _enact_bg(x, p: R.Params):
    "bg_elem, gamma = 2, every step one correctly rounded fp32 operation (the hardware's exp / rcp / log are worse: 1 ulp)."
    z = np.maximum(_f(x) + _f(p.logit_shift), _f(-80.0))
    with np.errstate(over="ignore", under="ignore"):
        den = _f(1.0) + _f(np.exp2((z * _f(-1.4426950408889634)).astype(np.float64)))
        ps = _f(1.0 / den.astype(np.float64))
        w = ps * ps
        bce = _f(_f(np.log2(den.astype(np.float64))).astype(np.float64) * np.float64(_f(0.6931471805599453)) + z.astype(np.float64))
        return w * bce, w * ps


def _enact_pos(x, p: R.Params):
    "focal_elem with pos = true, gamma = 2, in correctly rounded fp32 operations."
    z = _f(x) + _f(p.logit_shift)
    az = np.abs(z)
    with np.errstate(over="ignore", under="ignore"):
        e = _f(np.exp2((-az * _f(1.4426950408889634)).astype(np.float64)))
        den = _f(1.0) + e
        r = _f(1.0 / den.astype(np.float64))
        er = e * r
        om = np.where(z >= 0, er, r)
        w = (om * om) * _f(p.alpha_pos)
        l1p = _f(np.log2(den.astype(np.float64))) * _f(0.6931471805599453) + (e - (den - _f(1.0))) * r
        bce = np.maximum(-z, _f(0.0)) + l1p
        return w * bce, -(w * om)


def test_bounds_hold_for_correctly_rounded_fp32_arithmetic():
    """The fp32 sweep list through the re-enactment: every gradient and loss term within its bound (or under the floor, and then only
    in the predicted logit region).  A bound that fails HERE is wrong whatever the hardware does."""
    p = R.Params.make()
    x = R.f32_sweep_values()
    x = x[np.abs(x) < 3e38]                                       # (x + 1 overflows numpy's float32 with a warning; the GPU test keeps them)
    nf, B = 7, 2
    for pos in (False, True):
        m = np.full((1, x.size), 0 if pos else -1)
        r = R.reference(x.reshape(1, -1, 1), np.zeros((1, x.size, 4)), R.sweep_anchors(x.size), R.sweep_gt()[:1], [1], [0, 1], m, [nf], p)
        r.scale[:] = 1.0 / (nf * B)                               # as if it were one image of two
        r.gcls *= 0.5
        r.term *= 0.5
        wb, g = _enact_pos(x, p) if pos else _enact_bg(x, p)
        scale = _f(_f(1.0) / _f(nf)) * _f(1.0 / B)
        mult = scale if pos else _f(p.alpha) * scale
        with np.errstate(under="ignore", over="ignore", invalid="ignore"):
            got_g = (g * mult).astype(np.float64).reshape(r.gcls.shape)
            got_t = (wb.astype(np.float64) * np.float64(mult)).reshape(r.term.shape)
        fl, lim = R.cls_floor(r)
        assert fl.any() and R.floor_region(r)[fl].all()
        bound = R.cls_grad_bound(r) + R.half_ulp(r.gcls, "f32")
        assert (np.abs(got_g - r.gcls)[~fl] <= bound[~fl]).all()
        assert (np.abs(got_g[fl]) <= lim[fl] + R.half_ulp(lim[fl], "f32")).all() and (got_g[fl] * r.gcls[fl] >= 0).all()
        tf, tb = R.term_floor(r)
        ok = np.isfinite(r.term) & ~tf
        assert (np.abs(got_t - r.term)[ok] <= R.cls_term_bound(r)[ok]).all()
        assert (np.abs(got_t[tf] - r.term[tf]) <= tb[tf]).all()


# ---------------------------------------------------------------- the regression sweep's inputs
@pytest.mark.parametrize("fmt", ["f16", "bf16", "f32"])
def test_pure_l1_sweep_leaves_few_signs_undecidable(fmt):
    "beta = 0: the elements whose sign the float64 reference alone cannot decide stay under the cap of 0.1 % of the matched elements."
    values = R.f32_sweep_values() if fmt == "f32" else R.finite_patterns(fmt)
    p = R.Params.make(0.25, 2.0, 0.0)
    B, A = 2, 4099
    gt = np.concatenate([R.sweep_gt()] * B)
    n_parts = R.box_problem(values, 0)[3]
    for part in range(n_parts):
        box, m, nf, _ = R.box_problem(values, part)
        r = R.reference(np.zeros((B, A, 1)), box, R.sweep_anchors(A), gt, np.ones(16, dtype=np.int64), [0, 8, 16], m, nf, p)
        _, und = R.box_grad_bound(r)
        assert und.sum() <= 1e-3 * r.matched.sum() * 4, (part, int(und.sum()))
        t = r.tgt[r.matched]
        assert (t > 1).any() and (t < -1).any() and (np.abs(t) < 0.02).any() and (t[:, 2] < -15).any() and not (t == 0).any()
