"""The loss kernel (K3, csrc/loss.hip) restated element by element in float64, numpy only, and the error bounds its tests use.

Semantics (the list at the top of csrc/loss.hip and include/retinanet_hip.h):
  Q1  every logit is shifted: z = x + logit_shift
  Q2  reversed alpha: a background element (t = 0) weighs alpha, the positive element of a matched row 1 - alpha
  Q3  the focal weight is detached: d term / dx = w * (sigmoid(z) - t), w = alpha_t * (t ? 1 - p : p) ** gamma
  Q7  rows with match code -2 (and any other negative code but -1) contribute nothing; an image without GT contributes nothing
  Q8  each image is divided by max(num_fg, 1), then the images are averaged: scale_b = 1 / (max(num_fg_b, 1) * B)
  Q10 smooth-L1 with ``beta``: 0.5 d^2 / beta below beta, |d| - beta / 2 from it on; pure L1 when beta < 1e-5
  Q11 the size targets are log(gw / aw + log_eps)

``reference`` takes the STORED head outputs (already rounded to the I/O dtype) as float64 and the parameters as the fp32 values the
kernel receives (``Params.of``), so nothing but the kernel's own arithmetic separates the two.

The bounds.  u = 2^-24 is the relative error of one fp32 rounding.  v_exp_f32, v_rcp_f32 and v_log_f32 are accurate to 1 ulp = 2 u,
logf to 1 ulp, and loss.hip is compiled without the correctly-rounded-divide switch, so an fp32 division counts 2.5 ulp = 5 u.  FMA
contraction only removes roundings.  Every formula below is derived from the operation sequence it names, next to the formula; they
are the ONLY place tolerances for the element tests live, and none of them was fitted to a measurement.
"""
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
FLT_MIN = 2.0 ** -126                  # smallest normal fp32
LN2 = float(np.log(2.0))
DIV_U = 5.0                            # an fp32 division that is not correctly rounded: 2.5 ulp
PF = 2                                 # wave-iterations per group of the streaming pass (launch_loss)
LOSS_WAVES = 4
# rounding of alpha * ((1 / nf) * inv_B): the division, inv_B itself (rounded on the host), two products
GMUL_U = DIV_U + 3.0
# rounding of (1 / nf) * inv_B
SCALE_U = DIV_U + 2.0


@dataclass(frozen=True)
class Params:
    "rn_loss_params as the kernel sees it: every field already an fp32 value (held in a Python float)."
    alpha: float
    gamma: float
    beta: float
    logit_shift: float
    log_eps: float
    reg_w: tuple

    @staticmethod
    def of(p) -> "Params":
        "From anything with the six fields (the ctypes structs of the library and of the oracle included)."
        f = lambda v: float(np.float32(v))
        return Params(f(p.alpha), f(p.gamma), f(p.beta), f(p.logit_shift), f(p.log_eps), tuple(f(v) for v in p.reg_w))

    @staticmethod
    def make(alpha=0.25, gamma=2.0, beta=0.1, logit_shift=1.0, log_eps=1e-8, reg_w=(1.0, 1.0, 1.0, 1.0)) -> "Params":
        return Params.of(SimpleNamespace(alpha=alpha, gamma=gamma, beta=beta, logit_shift=logit_shift, log_eps=log_eps, reg_w=reg_w))

    @property
    def alpha_pos(self) -> float:
        return float(np.float32(1.0 - self.alpha))          # the host computes (float)(1.0 - (double)alpha)


def softplus(z):
    "log(1 + e^z) without overflow; softplus(-inf) = 0, softplus(+inf) = +inf."
    z = np.asarray(z, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def reference(cls, box, anchors, gt_boxes, gt_labels, gt_off, matches, num_fg, params: Params, prescale: float = 1.0):
    """cls [B,A,K], box [B,A,4] (float64 views of the stored values); anchors [A,4] or [B,A,4]; gt_boxes [sum T,4]; gt_labels
    [sum T] (1-based); gt_off [B+1]; matches [B,A] (-1 background, -2 ignored, >= 0 the GT index inside the image); num_fg [B].
    -> namespace with, per class element [B,A,K]: z, p = sigmoid(z), q = 1 - p, pos / dead masks, the probability ``qt`` the focal
    weight is taken of, ``w`` = alpha_t * qt^gamma, ``bce``, ``term`` (its share of the class loss) and ``gcls`` (its gradient, times
    ``prescale``); per box element [B,A,4]: ``tgt``, ``d`` = pred - tgt, ``term_box``, ``gbox``, ``matched`` [B,A]; ``scale`` [B];
    and the two sums ``loss_cls`` and ``loss_reg``."""
    cls = np.asarray(cls, dtype=np.float64)
    box = np.asarray(box, dtype=np.float64)
    B, A, K = cls.shape
    anchors = np.broadcast_to(np.asarray(anchors, dtype=np.float64), (B, A, 4))
    gt_boxes = np.asarray(gt_boxes, dtype=np.float64).reshape(-1, 4)
    gt_labels = np.asarray(gt_labels, dtype=np.int64).reshape(-1)
    gt_off = np.asarray(gt_off, dtype=np.int64)
    matches = np.asarray(matches, dtype=np.int64)
    T = gt_off[1:] - gt_off[:-1]
    live = T > 0                                                                   # Q7
    scale = np.where(live, 1.0 / (np.maximum(np.asarray(num_fg, dtype=np.int64), 1) * float(B)), 0.0)   # Q8
    matched = (matches >= 0) & live[:, None]
    dead = ((matches < -1) | ~live[:, None])                                        # ignored rows, and all rows of an image without GT
    gi = np.where(matched, gt_off[:-1, None] + np.maximum(matches, 0), 0)
    code = np.where(matched, gt_labels[gi] - 1 if gt_labels.size else 0, -1)
    pos = matched[:, :, None] & (np.arange(K)[None, None, :] == code[:, :, None])

    z = cls + params.logit_shift                                                   # Q1
    sp_pos, sp_neg = softplus(z), softplus(-z)
    p, q = np.exp(-sp_neg), np.exp(-sp_pos)                                         # sigmoid(z), 1 - sigmoid(z): no cancellation
    qt = np.where(pos, q, p)
    with np.errstate(under="ignore"):
        foc = np.ones_like(qt) if params.gamma == 0.0 else qt ** params.gamma
    w = foc * np.where(pos, params.alpha_pos, params.alpha)                         # Q2, Q3
    bce = np.where(pos, sp_neg, sp_pos)                                             # (1 - t) z - log sigmoid(z)
    sc = scale[:, None, None]
    with np.errstate(invalid="ignore", under="ignore"):
        term = np.where(w == 0.0, 0.0, w * bce) * sc                                # (0 * inf at a -inf logit: the weight wins)
        gcls = np.where(pos, -(w * q), w * p) * sc * prescale
    term = np.where(dead[:, :, None], 0.0, term)
    gcls = np.where(dead[:, :, None], 0.0, gcls)

    g = gt_boxes[gi] if gt_boxes.size else np.zeros((B, A, 4))
    with np.errstate(divide="ignore", invalid="ignore"):
        gcx, gcy, gw, gh = (g[..., 0] + g[..., 2]) / 2, (g[..., 1] + g[..., 3]) / 2, g[..., 2] - g[..., 0], g[..., 3] - g[..., 1]
        acx, acy = (anchors[..., 0] + anchors[..., 2]) / 2, (anchors[..., 1] + anchors[..., 3]) / 2
        aw, ah = anchors[..., 2] - anchors[..., 0], anchors[..., 3] - anchors[..., 1]
        rw = params.reg_w
        tgt = np.stack([(gcx - acx) / aw * rw[0], (gcy - acy) / ah * rw[1],
                        np.log(gw / aw + params.log_eps) * rw[2], np.log(gh / ah + params.log_eps) * rw[3]], -1)   # Q11
    m4 = matched[:, :, None]
    tgt = np.where(m4, tgt, 0.0)
    d = np.where(m4, box - tgt, 0.0)
    n = np.abs(d)
    if params.beta < 1e-5:                                                          # Q10
        l, gu = n, np.sign(d)
    else:
        l = np.where(n < params.beta, 0.5 * n * n / params.beta, n - 0.5 * params.beta)
        gu = np.where(n < params.beta, d / params.beta, np.sign(d))
    term_box = np.where(m4, l, 0.0) * sc
    gbox = np.where(m4, gu, 0.0) * sc * prescale
    geo = SimpleNamespace(gcx=gcx, gcy=gcy, gw=gw, gh=gh, acx=acx, acy=acy, aw=aw, ah=ah)
    with np.errstate(invalid="ignore"):
        loss_cls, loss_reg = float(term.sum()), float(term_box.sum())
    return SimpleNamespace(B=B, A=A, K=K, params=params, prescale=float(prescale), z=z, p=p, q=q, pos=pos, dead=dead, matched=matched,
                           qt=qt, w=w, bce=bce, term=term, gcls=gcls, scale=scale, tgt=tgt, d=d, term_box=term_box, gbox=gbox, geo=geo,
                           loss_cls=loss_cls, loss_reg=loss_reg)


# ---------------------------------------------------------------- output rounding
_FMT = {"f32": (24, -126), "f16": (11, -14), "bf16": (8, -126)}          # significand bits, smallest normal exponent


def half_ulp(x, fmt: str):
    "Half the spacing of ``fmt`` at |x| (the subnormal spacing below the smallest normal): the one rounding of an output to its dtype."
    bits, emin = _FMT[fmt]
    ax = np.abs(np.asarray(x, dtype=np.float64))
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.where(ax > 0, ax, 1.0)))
    e = np.maximum(np.where(ax > 0, e, emin), emin)
    return 0.5 * np.exp2(e - (bits - 1))


# ---------------------------------------------------------------- class branch
def _eps_exp(az):
    """Relative error of E = exp(-z) (bg_elem: v_exp_f32(z * -log2e); focal_elem: __expf(-|z|), the same two instructions), in u:
    z = fl(x + shift) moves the exponent by |z| u, the rounded constant log2e and the product's rounding by |z| u each -- an absolute
    error of 3 |z| log2e u in the base-2 exponent, times ln 2 -- and v_exp_f32 adds 1 ulp = 2 u."""
    return 3.0 * az + 2.0


def _eps_pow(gamma: float, eps_q, qt):
    """Relative error, in u, of qt^gamma given the relative error eps_q of qt.  gamma = 2: q * q, one rounding.  gamma = 0: the
    constant 1.  Else __powf = v_exp_f32(gamma * v_log_f32(q)): the log is off by 1 ulp of |log2 q| and the product by another half,
    3 |gamma log2 q| u absolute in the exponent, times ln 2; v_exp_f32 adds 2 u; the input error is amplified gamma times."""
    if gamma == 2.0:
        return 2.0 * eps_q + 1.0
    if gamma == 0.0:
        return np.zeros_like(eps_q)
    with np.errstate(divide="ignore"):
        l2 = np.abs(np.log2(np.where(qt > 0, qt, 1.0)))
    return gamma * eps_q + 3.0 * LN2 * gamma * l2 + 2.0


def cls_rel_errors(ref):
    """(eps_qt, eps_w) in u per class element: the relative errors of the probability the focal weight is taken of and of the weight.
    Background (bg_elem): den = 1 + E (1 u), ps = v_rcp_f32(den) (2 u); d ln ps / d ln E = -q, so eps_ps = q eps_E + 3.
    Positive (focal_elem): e = exp(-|z|), den = 1 + e (1 u), r = rcp (2 u), om = e * r or r (1 u); d ln om / d ln e = +-p either way,
    so eps_om = p eps_e + 4; the weight is then multiplied by alpha_pos (its own rounding and the product's: 2 u)."""
    eE = _eps_exp(np.abs(ref.z))
    eps_q = np.where(ref.pos, ref.p * eE + 4.0, ref.q * eE + 3.0)
    eps_w = _eps_pow(ref.params.gamma, eps_q, ref.qt) + np.where(ref.pos, 2.0, 0.0)
    return eps_q, eps_w


def cls_grad_bound(ref):
    """|kernel - reference| allowed for every class gradient, before the output rounding (``half_ulp``).
    Background: g = (w * ps) * gmul_g -- eps_w + eps_ps, the product (1 u), gmul_g = alpha * ((1 / nf) * inv_B) * gs (GMUL_U + 1) and
    the last product (1 u).  For gamma = 2 this is (9 q |z| + 6 q + 21) u |g|: three factors of ps, each carrying E's 3 |z| u.
    Positive: grad = -(w * om) * (scale * gs) -- eps_w + eps_om + 1, scale * gs (SCALE_U + 1) and the last product (1 u):
    (9 p |z| + 6 p + 25) u |g| for gamma = 2.  Dead elements are exact zeros: bound 0."""
    eps_q, eps_w = cls_rel_errors(ref)
    rel = eps_w + eps_q + 1.0 + np.where(ref.pos, SCALE_U + 2.0, GMUL_U + 2.0)
    return rel * U * np.abs(ref.gcls)


def bce_bound(ref):
    """Absolute error of the bce value, per element.
    Background: bce = fma(v_log_f32(den), ln2, z), true value softplus(z).  With sp = softplus: the log and the rounded ln2 cost
    3 u ln(den) = 3 sp(-z) u; den carries q eps_E' + 1 (eps_E' = 2 |z| + 2: the part of E's error that is not z's own rounding);
    z's rounding moves softplus by p |z| u; the fma rounds once: sp(z) u.  Towards z -> -inf this is (5 |z| + 3) u ABSOLUTE on a
    value of e^z: the cancellation the kernel accepts, harmless because p^gamma multiplies it.
    Positive: bce = max(-z, 0) + l1p, l1p = log(den) ln2 + (e - (den - 1)) r (the correction restores the bits 1 + e lost, leaving
    second-order terms): 5 u l1p (log 2 u, ln2 1 u, product, sum), e's error times d log1p / de = min(p, q), z's rounding q |z| u and
    the last sum sp(-z) u."""
    az = np.abs(ref.z)
    l1p = softplus(-az)
    with np.errstate(invalid="ignore"):
        bg = 3.0 * softplus(-ref.z) + ref.q * (2.0 * az + 2.0) + 1.0 + softplus(ref.z) + ref.p * az
        ps = ref.q * az + 5.0 * l1p + np.minimum(ref.p, ref.q) * (2.0 * az + 2.0) + softplus(-ref.z)
    return np.where(ref.pos, ps, bg) * U


def cls_term_bound(ref):
    """|kernel - reference| allowed for one element's share of the class loss: the weight times the bce error, plus the relative
    errors of the weight, of the product w * bce (1 u) and of the image multiplier (GMUL_U, or SCALE_U for a positive), on the term."""
    _, eps_w = cls_rel_errors(ref)
    sc = ref.scale[:, None, None]
    with np.errstate(invalid="ignore", over="ignore"):
        b = ref.w * sc * bce_bound(ref) + (eps_w + 1.0 + np.where(ref.pos, SCALE_U, GMUL_U)) * U * np.abs(ref.term)
    return np.where(ref.dead[:, :, None] | (ref.w == 0.0), 0.0, b)


def cls_floor(ref):
    """Elements whose reference magnitude falls below the smallest normal fp32 somewhere along the kernel's chain of products -- the
    probability qt, the weight qt^gamma, weight * qt, and that times the image multiplier and the prescale -- where the kernel's
    intermediate underflows (or is cut by the clamp of z at -80) and only the sign and an upper limit can be asked for.
    -> (mask, limit): |gradient| <= limit = 2 * FLT_MIN * max(1, multiplier) there.  The derivation predicts the region: qt^3 * mult
    < 2^-126 needs qt small, that is z very negative for a background element and very positive for a positive one
    (``floor_region``).  The clamp: below z = -80 bg_elem computes the element AT z = -80, so a background gradient may also be as large
    as the value there, multiplier * sigmoid(-80)^(gamma + 1) (with that point's relative error, (gamma + 1) (3 * 80 + 5) + 30 u).  For
    gamma = 2 that is 6e-105, nothing; for gamma = 0 it is 1.8e-35 * multiplier where the reference holds e^z * multiplier < 2^-126:
    an absolute error of 1.8e-35 on a gradient, which is what the clamp was chosen to cost."""
    sc = ref.scale[:, None, None]
    mult = np.where(ref.pos, 1.0, ref.params.alpha) * sc * ref.prescale
    with np.errstate(under="ignore"):
        foc = np.ones_like(ref.qt) if ref.params.gamma == 0.0 else ref.qt ** ref.params.gamma
        chain = np.minimum.reduce([ref.qt, foc, foc * ref.qt, foc * ref.qt * mult * np.where(ref.pos, ref.params.alpha_pos, 1.0)])
    mask = (chain < FLT_MIN) & ~ref.dead[:, :, None] & (mult > 0)
    g1 = ref.params.gamma + 1.0
    at_clamp = mult * float(np.exp(-softplus(80.0))) ** g1 * (1.0 + (g1 * 245.0 + 30.0) * U)
    return mask, np.maximum(2.0 * FLT_MIN * np.maximum(1.0, mult), np.where(ref.pos, 0.0, at_clamp))


def floor_region(ref):
    """The logit region ``cls_floor`` may flag, from qt ~ e^{-|z|} on the small side: qt^(gamma + 1) * min(1, mult) < 2^-126 (or
    qt < 2^-126 for gamma = 0) <=> |z| > -ln(2^-126 / min(1, mult)) / (gamma + 1), on the negative side for a background element,
    on the positive side for a positive one.  -> boolean array: True where an element MAY be under the floor."""
    sc = ref.scale[:, None, None]
    mult = np.minimum(1.0, np.where(ref.pos, ref.params.alpha_pos, ref.params.alpha) * sc * ref.prescale)
    with np.errstate(divide="ignore"):
        zlim = -np.log(FLT_MIN / np.where(mult > 0, mult, 1.0)) / (ref.params.gamma + 1.0) - np.log(2.0)   # (qt <= e^{-|z|} < 2 qt)
    return np.where(ref.pos, ref.z > zlim, ref.z < -zlim)


def term_floor(ref):
    """Class loss terms whose weight (or weight * bce * multiplier) is below the smallest normal fp32: the kernel's product is a
    subnormal or zero.  -> (mask, bound).  Either the weight itself has underflowed -- then |kernel term| <= FLT_MIN * (bce + its error)
    * multiplier, and the reference is no larger -- or it is normal and ``cls_term_bound`` holds up to the underflow of the later
    products: the bound is the sum of the two, |reference| + 2 * FLT_MIN * max(1, bce) * max(1, multiplier) + cls_term_bound."""
    sc = ref.scale[:, None, None]
    mult = np.where(ref.pos, 1.0, ref.params.alpha) * sc
    with np.errstate(under="ignore", invalid="ignore", over="ignore"):
        foc = np.ones_like(ref.qt) if ref.params.gamma == 0.0 else ref.qt ** ref.params.gamma
        chain = np.minimum.reduce([ref.qt, foc, foc * ref.bce, np.abs(ref.term)])
        bound = np.abs(ref.term) + 2.0 * FLT_MIN * np.maximum(1.0, np.where(np.isfinite(ref.bce), ref.bce, 1.0)) * np.maximum(1.0, mult)
    mask = (chain < FLT_MIN) & ~ref.dead[:, :, None] & (mult > 0)
    return mask, bound + cls_term_bound(ref)


def chain_length(vec: int) -> int:
    """The longest fp32 addition chain a class loss term passes through (loss_stream_kernel): a lane adds the PF * VEC terms of a
    group in fp32 (acc_g) -- groups, the wave reduction and the ignored-row removals are in double --, the wave's sum is rounded to
    fp32 once, the LOSS_WAVES wave sums are added in fp32, and the fixed-point total is rounded to fp32 once."""
    return PF * vec + 1 + LOSS_WAVES + 1


REG_CHAIN = 4 + 8 + 6 + LOSS_WAVES + 1   # a row's 4 terms, <= 8 rows per lane (512-row strips), the 6-level wave reduction, waves, final


def sum_bound(elem_bounds, terms, n_chain: int, n_partials: int) -> float:
    """|kernel sum - reference sum| allowed: the element bounds added up, n_chain * u relative to the sum of |terms| that went through
    the fp32 chain (``terms`` includes what is added and taken out again: the background term of a positive or ignored element), and
    half a unit of the 2^-32 fixed point per workgroup partial."""
    return float(np.sum(elem_bounds) + n_chain * U * np.sum(np.abs(terms)) + n_partials * 2.0 ** -33)


# ---------------------------------------------------------------- regression branch
def box_d_bound(ref):
    """Absolute error of d = pred - tgt per box element (reg_row), [B,A,4]; 0 at unmatched rows.
    Centres: gcx = (g.x + g.z) / 2 and acx each carry 1 u of themselves, their difference 1 u, so the numerator is off by
    (|gcx| + |acx| + |gcx - acx|) u -- the cancellation of two large coordinates is paid here --; then / aw (aw: 1 u, the division
    DIV_U) and * reg_w (1 u): (DIV_U + 2) u |tgt|.
    Sizes: gw / aw carries 1 + 1 + DIV_U, adding log_eps one more: the argument of logf is off by (DIV_U + 3) u relative, which
    is that much ABSOLUTE in the log; logf itself 1 ulp = 2 u |log|; * reg_w 1 u.
    The subtraction pred - tgt rounds once: u |d|."""
    g, rw = ref.geo, ref.params.reg_w
    with np.errstate(divide="ignore", invalid="ignore"):
        c = [np.abs(rw[0]) * (np.abs(g.gcx) + np.abs(g.acx) + np.abs(g.gcx - g.acx)) / g.aw,
             np.abs(rw[1]) * (np.abs(g.gcy) + np.abs(g.acy) + np.abs(g.gcy - g.acy)) / g.ah]
        s = [np.abs(rw[2]) * (DIV_U + 3.0) * np.ones_like(g.aw), np.abs(rw[3]) * (DIV_U + 3.0) * np.ones_like(g.ah)]
    t = np.abs(ref.tgt)
    b = np.stack([c[0] + (DIV_U + 2.0) * t[..., 0], c[1] + (DIV_U + 2.0) * t[..., 1], s[0] + 3.0 * t[..., 2], s[1] + 3.0 * t[..., 3]], -1)
    b = (b + np.abs(ref.d)) * U
    return np.where(ref.matched[:, :, None], b, 0.0)


def box_grad_bound(ref):
    """-> (bound, undecidable) per box element.  beta >= 1e-5: the gradient is clip(d / beta, -1, 1) * scale * gs, continuous in d,
    so d's error costs at most d_bound / beta (never more than 2; nothing where |d| - d_bound > beta), the division DIV_U u, scale * gs and the last product SCALE_U + 2.
    beta < 1e-5 (pure L1): the gradient is sign(d); where |d| <= d_bound the sign cannot be decided and the element is left out."""
    db = box_d_bound(ref)
    sc = ref.scale[:, None, None] * ref.prescale
    if ref.params.beta < 1e-5:
        und = ref.matched[:, :, None] & (np.abs(ref.d) <= db)
        return (SCALE_U + 2.0) * U * np.abs(ref.gbox), und
    far = np.abs(ref.d) - db > ref.params.beta                      # beyond beta whatever the error: the sign, exactly
    b = np.where(far, 0.0, np.minimum(db / ref.params.beta, 2.0)) * sc + (DIV_U + SCALE_U + 2.0) * U * np.abs(ref.gbox)
    return b, np.zeros(ref.d.shape, dtype=bool)


def box_term_bound(ref):
    """Per box element's share of the regression loss: smooth-L1 is 1-Lipschitz in d (d_bound), its own arithmetic is at most three
    roundings and one division, and the row's sum is multiplied by scale (SCALE_U + 1)."""
    return box_d_bound(ref) * ref.scale[:, None, None] + (DIV_U + 3.0 + SCALE_U + 1.0) * U * np.abs(ref.term_box)


# ---------------------------------------------------------------- inputs shared by the CPU and the GPU tests (numpy only)
def finite_patterns(fmt: str) -> np.ndarray:
    "Every finite value of a 16-bit format, as float32 (exact), in bit-pattern order: 63 488 for f16, 65 280 for bf16."
    bits = np.arange(65536, dtype=np.uint32)
    v = bits.astype(np.uint16).view(np.float16).astype(np.float32) if fmt == "f16" else (bits << 16).astype(np.uint32).view(np.float32)
    return v[np.isfinite(v)]


def f32_sweep_values(seed: int = 32) -> np.ndarray:
    """The fp32 logit list: every bf16 value, a grid over [-100, 100] in steps of 1/256, 20 000 seeded random finite bit patterns,
    +-0, the smallest and largest subnormals and normals, +-3.4e38."""
    rng = np.random.default_rng(seed)
    rnd = rng.integers(0, 2 ** 32, 40000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    rnd = rnd[np.isfinite(rnd)][:20000]
    edge = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000,
                     0x7f7fffff, 0xff7fffff], dtype=np.uint32).view(np.float32)
    grid = (np.arange(-25600, 25601, dtype=np.float64) / 256.0).astype(np.float32)
    return np.concatenate([finite_patterns("bf16"), grid, rnd, edge, np.array([3.4e38, -3.4e38], dtype=np.float32)])


def sweep_anchors(A: int) -> np.ndarray:
    "A anchors [A,4] fp32 of four widths and four heights on a lattice of eighths (every coordinate exact in fp32)."
    a = np.arange(A)
    cx, cy = 50.0 + (a % 61) * 5.25, 40.0 + (a % 53) * 7.5
    w, h = np.array([8.0, 16.0, 37.5, 100.0])[a % 4], np.array([12.0, 100.0, 20.25, 64.0])[(a // 4) % 4]
    return np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(np.float32)


def sweep_gt() -> np.ndarray:
    """Eight GT boxes [8,4] fp32: large and small, far and near, a width of exactly 0 and one of a single fp32 spacing (gw / aw ~ 1e-7:
    log_eps decides the target), sizes within 2 % of an anchor's (targets near 0, never AT 0: a pure-L1 sign must stay decidable), and
    centres off the anchors' lattice by sixteenths, so that targets of both signs occur and none is 0."""
    g = np.array([[10.0625, 20.0625, 300.0, 400.0], [100.0625, 100.0625, 108.0, 112.0], [100.0, 50.0625, 100.0, 90.0],
                  [100.0, 50.0625, 100.00001, 90.0], [60.0625, 60.0625, 60.0625 + 37.5 * (1 + 1 / 64), 60.0625 + 20.25 * (1 - 1 / 64)],
                  [200.5625, 33.3125, 216.5, 133.25], [900.0625, 700.0625, 1000.0, 764.0], [0.0625, 0.0625, 8.0, 12.0]], dtype=np.float32)
    return g


def sweep_roles(B: int, A: int, K: int, j: int):
    """Launch ``j`` of the role rotation, period K + 2: row a of image b has v = (a + j + 3 b) mod (K + 2); v < K: matched to a GT box
    of label v + 1; v = K: ignored; v = K + 1: background.  Over the K + 2 launches every element is once the positive element, once in
    an ignored row and K times a background element.  (K launches cannot do that on fixed data: a row has to be matched K times, once per
    label, and ignored once.)  -> (matches [B,A] i64, num_fg [B] i32, gt_labels [B*8] i64, special [B, ceil(A/64)] u64)."""
    a = np.arange(A)
    matches = np.empty((B, A), dtype=np.int64)
    labels = np.empty((B, 8), dtype=np.int64)
    for b in range(B):
        labels[b] = (np.arange(8) + b) % K + 1
        v = (a + j + 3 * b) % (K + 2)
        t = (v - b) % K                                           # labels[b][t] == v + 1
        t = np.where((t + K < 8) & ((a // 7) % 2 == 1), t + K, t)  # ... and so is labels[b][t + K]
        matches[b] = np.where(v < K, t, np.where(v == K, -2, -1))
    num_fg = (matches >= 0).sum(1).astype(np.int32)
    return matches, num_fg, labels.reshape(-1), special_words(matches)


def special_words(matches: np.ndarray) -> np.ndarray:
    "The flag words of ops.iou_match: bit (a & 63) of word a >> 6 of image b is set where matches[b, a] != -1.  [B, ceil(A/64)] uint64."
    B, A = matches.shape
    W = (A + 63) // 64
    bits = np.zeros((B, W * 64), dtype=np.uint64)
    bits[:, :A] = matches != -1
    return (bits.reshape(B, W, 64) << np.arange(64, dtype=np.uint64)[None, None, :]).sum(2, dtype=np.uint64)


def box_problem(values: np.ndarray, part: int, B: int = 2, A: int = 4099, seed: int = 9):
    """Launch ``part`` of the regression sweep: seven rows in eight are matched (GT index (a + b) mod 8), and the matched rows' 4 * 7/8 *
    B * A predictions are the next slice of the seeded permutation of ``values`` (wrapping around); unmatched rows hold a constant.
    -> (box [B,A,4] float32, matches, num_fg, n_parts)."""
    perm = np.random.default_rng(seed).permutation(values.size)
    a = np.arange(A)
    matches = np.stack([np.where((a + b) % 8 == 7, np.where(a % 16 < 8, -1, -2), (a + 3 * b) % 8) for b in range(B)]).astype(np.int64)
    m = matches >= 0
    per = int(m.sum()) * 4
    n_parts = -(-values.size // per)
    idx = perm[(part * per + np.arange(per)) % values.size]
    box = np.full((B, A, 4), 0.5, dtype=np.float32)
    box[m] = values[idx].reshape(-1, 4)
    return box, matches, m.sum(1).astype(np.int32), n_parts
