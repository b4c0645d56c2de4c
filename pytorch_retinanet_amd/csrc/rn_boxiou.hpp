// Steps 1 and 2 of rn_box_iou_loss's rule (include/retinanet_hip.h): the standard decode of a row's four deltas with RN_BOX_XFORM_CLIP,
// then its IoU with the GT box.  ONE copy for boxloss.hip (which goes on to the penalty and the gradient) and qfl.hip (whose quality
// target is the IoU): both are built without FMA contraction, so both get the same bits.  Also the row loads / stores of four I/O
// elements both kernels use.
#pragma once
#include "rn_common.hpp"

#include <math.h>

namespace rn {

template <int DT> struct box4;                    // one row of four I/O elements <-> float[4] (as loss.hip's)
template <> struct box4<RN_F32> {
    static __device__ __forceinline__ void ld(const void *p, int64_t row, float (&f)[4]) {
        const f32x4 v = ((const f32x4 *)p)[row];
        f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
    }
    static __device__ __forceinline__ void st(void *p, int64_t row, const float (&f)[4]) {
        f32x4 v; v.x = f[0]; v.y = f[1]; v.z = f[2]; v.w = f[3];
        ((f32x4 *)p)[row] = v;
    }
};
template <> struct box4<RN_BF16> {
    static __device__ __forceinline__ void ld(const void *p, int64_t row, float (&f)[4]) {
        const u32x2 v = ((const u32x2 *)p)[row];
        f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
        f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
    }
    static __device__ __forceinline__ void st(void *p, int64_t row, const float (&f)[4]) {
        u32x2 v; v.x = dt<RN_BF16>::pk(f[0], f[1]); v.y = dt<RN_BF16>::pk(f[2], f[3]);
        ((u32x2 *)p)[row] = v;
    }
};
template <> struct box4<RN_F16> {
    static __device__ __forceinline__ void ld(const void *p, int64_t row, float (&f)[4]) {
        const u32x2 v = ((const u32x2 *)p)[row];
        f[0] = half_lo(v.x); f[1] = half_hi(v.x); f[2] = half_lo(v.y); f[3] = half_hi(v.y);
    }
    static __device__ __forceinline__ void st(void *p, int64_t row, const float (&f)[4]) {
        u32x2 v; v.x = dt<RN_F16>::pk(f[0], f[1]); v.y = dt<RN_F16>::pk(f[2], f[3]);
        ((u32x2 *)p)[row] = v;
    }
};

// What steps 1 and 2 leave behind: the decoded box, the selections of every min / max and the IoU.
struct BoxIou {
    float aw, ah, cx, cy, w, h, px1, py1, px2, py2;
    bool clip_w, clip_h;                          // the slot was above the clip: its gradient is zero
    bool sx2, sx1, sy2, sy1;                      // the PREDICTED coordinate was selected (strict comparison; a tie goes to the GT box)
    bool pw, ph, pu;                              // iw0 > 0, ih0 > 0, union > 0
    float iw, ih, inter, uni, iou;
};

static __device__ __forceinline__ BoxIou box_decode_iou(const f32x4 g, const f32x4 an, const float (&d)[4], const float (&reg_w)[4])
{
    BoxIou r;
    // 1. decode
    const float t0 = d[0] / reg_w[0], t1 = d[1] / reg_w[1], t2 = d[2] / reg_w[2], t3 = d[3] / reg_w[3];
    const float acx = (an.x + an.z) / 2.0f, acy = (an.y + an.w) / 2.0f;
    r.aw = an.z - an.x; r.ah = an.w - an.y;
    r.cx = r.aw * t0 + acx; r.cy = r.ah * t1 + acy;
    r.clip_w = t2 > RN_BOX_XFORM_CLIP; r.clip_h = t3 > RN_BOX_XFORM_CLIP;
    const float sw = r.clip_w ? RN_BOX_XFORM_CLIP : t2, sh = r.clip_h ? RN_BOX_XFORM_CLIP : t3;
    r.w = r.aw * expf(sw); r.h = r.ah * expf(sh);
    const float hw = r.w / 2.0f, hh = r.h / 2.0f;
    r.px1 = r.cx - hw; r.py1 = r.cy - hh; r.px2 = r.cx + hw; r.py2 = r.cy + hh;
    // 2. IoU (the predicted coordinate is selected -- and takes the derivative -- only on a strict comparison; a tie goes to the GT box)
    r.sx2 = r.px2 < g.z; r.sx1 = r.px1 > g.x; r.sy2 = r.py2 < g.w; r.sy1 = r.py1 > g.y;
    const float iw0 = (r.sx2 ? r.px2 : g.z) - (r.sx1 ? r.px1 : g.x), ih0 = (r.sy2 ? r.py2 : g.w) - (r.sy1 ? r.py1 : g.y);
    r.pw = iw0 > 0.0f; r.ph = ih0 > 0.0f;
    r.iw = r.pw ? iw0 : 0.0f; r.ih = r.ph ? ih0 : 0.0f;
    r.inter = r.iw * r.ih;
    r.uni = (r.w * r.h + (g.z - g.x) * (g.w - g.y)) - r.inter;
    r.pu = r.uni > 0.0f;
    r.iou = r.pu ? r.inter / r.uni : 0.0f;
    return r;
}

}  // namespace rn
