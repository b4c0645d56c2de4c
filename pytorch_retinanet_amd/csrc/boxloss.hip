// IoU-type box regression losses (GIoU, DIoU) on the matched rows: rn_box_iou_loss.  The rule, step by step with its roundings, is
// in include/retinanet_hip.h; losses.box_iou_loss_reference restates it in torch.  Built without FMA contraction.
//
// The call runs BEHIND K3 (loss.hip), which has already written grad_box for every row (zeros for background / ignored rows, the
// smooth-L1 gradients for matched ones) and out_loss[1].  It walks the matcher's flag words (rn_rowwalk.hpp: the launch shape and the
// sum), recomputes the loss of the matched rows and overwrites those rows' gradients and out_loss[1].  Nothing else is touched.
//
// A listed row is a chain of two dependent loads, match -> (GT box, anchor, deltas): nothing is loaded before the match is known, so
// an ignored row costs its match alone.
#include "rn_boxiou.hpp"
#include "rn_rowwalk.hpp"

namespace {

using rn::box4;

// Steps 1-4 of the rule for one matched row (1 and 2: rn::box_decode_iou): returns l, writes dl / dd[j] (unscaled).
__device__ __forceinline__ float iou_row(const rn::f32x4 g, const rn::f32x4 an, const float (&d)[4], const float (&reg_w)[4],
                                         const int kind, float (&grad)[4])
{
    // 1. decode and 2. IoU: rn_boxiou.hpp (shared with qfl.hip)
    const rn::BoxIou q = rn::box_decode_iou(g, an, d, reg_w);
    const float aw = q.aw, ah = q.ah, cx = q.cx, cy = q.cy, w = q.w, h = q.h, px1 = q.px1, py1 = q.py1, px2 = q.px2, py2 = q.py2;
    const bool clip_w = q.clip_w, clip_h = q.clip_h, sx2 = q.sx2, sx1 = q.sx1, sy2 = q.sy2, sy1 = q.sy1, pw = q.pw, ph = q.ph, pu = q.pu;
    const float iw = q.iw, ih = q.ih, uni = q.uni, iou = q.iou;
    // 3. penalty (enclosing box: again the predicted coordinate only on a strict comparison)
    const bool ex2p = px2 > g.z, ex1p = px1 < g.x, ey2p = py2 > g.w, ey1p = py1 < g.y;
    const float ew = (ex2p ? px2 : g.z) - (ex1p ? px1 : g.x), eh = (ey2p ? py2 : g.w) - (ey1p ? py1 : g.y);
    float pen = 0.0f;
    // d l / d(inter), d(union), d(ew), d(eh), d(cx), d(cy) as they come out of steps 2 and 3
    float g_uni = pu ? iou / uni : 0.0f;                     // l = 1 - inter / union + pen
    float g_inter = pu ? -1.0f / uni : 0.0f;
    float g_ew = 0.0f, g_eh = 0.0f, g_cx = 0.0f, g_cy = 0.0f;
    if (kind == RN_BOX_LOSS_GIOU) {
        const float c = ew * eh;
        if (c > 0.0f) {
            pen = (c - uni) / c;
            g_uni -= 1.0f / c;
            const float g_c = uni / (c * c);
            g_ew = g_c * eh; g_eh = g_c * ew;
        }
    } else {
        const float c2 = ew * ew + eh * eh;
        const float dxc = cx - (g.x + g.z) / 2.0f, dyc = cy - (g.y + g.w) / 2.0f;
        const float rho2 = dxc * dxc + dyc * dyc;
        if (c2 > 0.0f) {
            pen = rho2 / c2;
            const float g_c2 = -rho2 / (c2 * c2);
            g_ew = g_c2 * (2.0f * ew); g_eh = g_c2 * (2.0f * eh);
            g_cx = (2.0f * dxc) / c2; g_cy = (2.0f * dyc) / c2;
        }
    }
    // 4. gradient: union = (w h + area_g) - inter
    g_inter -= g_uni;
    const float g_iw = pw ? g_inter * ih : 0.0f, g_ih = ph ? g_inter * iw : 0.0f;
    const float g_px2 = (sx2 ? g_iw : 0.0f) + (ex2p ? g_ew : 0.0f), g_px1 = -((sx1 ? g_iw : 0.0f) + (ex1p ? g_ew : 0.0f));
    const float g_py2 = (sy2 ? g_ih : 0.0f) + (ey2p ? g_eh : 0.0f), g_py1 = -((sy1 ? g_ih : 0.0f) + (ey1p ? g_eh : 0.0f));
    g_cx += g_px1 + g_px2; g_cy += g_py1 + g_py2;
    const float g_w = g_uni * h + (g_px2 - g_px1) / 2.0f, g_h = g_uni * w + (g_py2 - g_py1) / 2.0f;
    grad[0] = (g_cx * aw) / reg_w[0];
    grad[1] = (g_cy * ah) / reg_w[1];
    grad[2] = clip_w ? 0.0f : (g_w * w) / reg_w[2];
    grad[3] = clip_h ? 0.0f : (g_h * h) / reg_w[3];
    return (1.0f - iou) + pen;
}

struct BoxIouOp {
    rn::WalkArgs w;
    int32_t kind;
    float loss_weight;

    template <int DT, bool WRITE_GRAD>
    __device__ __forceinline__ void row(const rn::WalkRow &row, const float gs, double &acc) const
    {
        int64_t pm = -1;
        if (row.ok) pm = w.match(row);
        if (row.ok && pm >= 0) {
            const rn::f32x4 g = w.gt_boxes[w.gt_row(row, pm)];
            const rn::f32x4 an = w.anchor(row);
            float d[4], gb[4];
            box4<DT>::ld(row.lv.box, row.r, d);
            const float l = iou_row(g, an, d, w.reg_w, kind, gb);
            acc += (double)l * (double)row.scale;
            if (WRITE_GRAD) {
                const float gmul = (loss_weight * row.scale) * gs;
#pragma unroll
                for (int j = 0; j < 4; ++j) gb[j] *= gmul;
                box4<DT>::st(row.lv.grad, row.r, gb);
            }
        }
    }
};

}  // namespace

RN_API size_t rn_box_iou_loss_workspace_bytes(int B, int64_t A) { return rn::walk_workspace_bytes(B, A); }

RN_API int rn_box_iou_loss(const void *const *box_levels, const int64_t *level_anchors, int L, int dtype, int B,
                           const float *anchors, int64_t anchor_bstride, const float *gt_boxes, const int32_t *gt_off,
                           const int64_t *matches, const uint64_t *special_rows, const int32_t *num_fg,
                           const float *reg_w, int kind, float loss_weight, const float *grad_prescale,
                           float *out_loss, void *const *grad_box_levels, void *workspace, size_t workspace_bytes, void *stream)
{
    if (kind != RN_BOX_LOSS_GIOU && kind != RN_BOX_LOSS_DIOU) return RN_EINVAL;
    if (!(loss_weight > 0.0f) || !(loss_weight < INFINITY)) return RN_EINVAL;
    BoxIouOp op{};
    int blocks = 0;
    const int rc = rn::walk_fill(op.w, blocks, nullptr, box_levels, level_anchors, L, dtype, B, anchors, anchor_bstride, gt_boxes, nullptr,
                                 gt_off, matches, special_rows, num_fg, reg_w, grad_prescale, out_loss, grad_box_levels, workspace,
                                 workspace_bytes);
    if (rc != RN_OK) return rc;
    op.kind = kind; op.loss_weight = loss_weight;
    return rn::walk_launch<1, false>(op, blocks, dtype, grad_box_levels != nullptr, loss_weight, out_loss, (hipStream_t)stream);
}
