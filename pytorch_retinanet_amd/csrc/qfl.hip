// Quality Focal Loss on the matched rows' label elements: rn_quality_focal_loss.  The rule, step by step with its roundings, is in
// include/retinanet_hip.h; losses.box_quality_reference / losses.quality_focal_loss_reference restate it in torch.  Built without
// FMA contraction; steps 1-2 of the box rule (the quality) are rn_boxiou.hpp's, the code boxloss.hip runs.
//
// The call runs BEHIND a K3 call (loss.hip) with alpha = 1, gamma = beta: K3 has then written QFL's negative term for every
// background element, and a zero loss and a zero gradient for the label element of every matched row.  This call walks the matcher's
// flag words (rn_rowwalk.hpp: the launch shape and the sum, as rn_box_iou_loss), computes the soft-target term of those label
// elements, adds their sum to out_loss[0] and stores that one class gradient element per matched row.  Nothing else is touched.
//
// A listed row is one chain match -> (GT box, label) -> logit; the loads that do not hang on the match (anchor, deltas) go out with
// it, the GT box and the label go out together.
#include "rn_boxiou.hpp"
#include "rn_rowwalk.hpp"

namespace {

using rn::box4;

// Steps 2 and 3 of the rule for one label element: returns l, writes dl / dx (unscaled).
__device__ __forceinline__ float qfl_elem(const float x, const float q, const float beta, const float logit_shift, float &grad)
{
    const float z = x + logit_shift;
    const float e = expf(-fabsf(z));                   // exp(-|z|) in (0,1]
    const float r = 1.0f / (1.0f + e);
    const float sigma = z >= 0.0f ? r : e * r;         // sigmoid(z): no overflow, and no 1 - x for a small sigma
    const float bce = (fmaxf(z, 0.0f) - q * z) + log1pf(e);
    const float d = sigma - q;
    const float w = beta == 2.0f ? d * d : (beta == 0.0f ? 1.0f : powf(fabsf(d), beta));
    grad = w * d;                                      // the weight is a constant of the derivative (K3's quirk Q3)
    return w * bce;
}

struct QflOp {
    rn::WalkArgs w;
    int32_t K;
    float beta, logit_shift;

    template <int DT, bool WRITE_GRAD>
    __device__ __forceinline__ void row(const rn::WalkRow &row, const float gs, double &acc) const
    {
        // the loads of a listed row that do not hang on its match go out WITH the match (an ignored row pays for them in vain)
        int64_t pm = -1;
        rn::f32x4 an = {0.0f, 0.0f, 1.0f, 1.0f};
        float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (row.ok) {
            pm = w.match(row);
            an = w.anchor(row);
            box4<DT>::ld(row.lv.box, row.r, d);
        }
        if (row.ok && pm >= 0) {
            const int64_t gi = w.gt_row(row, pm);
            const rn::f32x4 g = w.gt_boxes[gi];                                         // the GT box and the label: one round trip
            const int64_t c = w.gt_labels[gi] - 1;
            if (c >= 0 && c < (int64_t)K) {                                             // (a label outside 1..K: the row adds and writes nothing)
                const int64_t e = row.r * (int64_t)K + c;
                const float x = rn::dt<DT>::ld(row.lv.cls, e);
                const float q = rn::box_decode_iou(g, an, d, w.reg_w).iou;
                float gr;
                const float l = qfl_elem(x, q, beta, logit_shift, gr);
                acc += (double)l * (double)row.scale;
                if (WRITE_GRAD) rn::dt<DT>::st(row.lv.grad, e, (gr * row.scale) * gs);   // (one element: rows of an odd K start at odd offsets)
            }
        }
    }
};

}  // namespace

RN_API size_t rn_quality_focal_loss_workspace_bytes(int B, int64_t A) { return rn::walk_workspace_bytes(B, A); }

RN_API int rn_quality_focal_loss(const void *const *cls_levels, const void *const *box_levels, const int64_t *level_anchors, int L,
                                 int dtype, int B, int K, const float *anchors, int64_t anchor_bstride, const float *gt_boxes,
                                 const int64_t *gt_labels, const int32_t *gt_off, const int64_t *matches,
                                 const uint64_t *special_rows, const int32_t *num_fg, const float *reg_w, float beta,
                                 float logit_shift, const float *grad_prescale, float *out_loss, void *const *grad_cls_levels,
                                 void *workspace, size_t workspace_bytes, void *stream)
{
    if (!cls_levels || K < 1) return RN_EINVAL;
    if (!(beta >= 0.0f) || !(beta < INFINITY) || !(fabsf(logit_shift) < INFINITY)) return RN_EINVAL;
    QflOp op{};
    int blocks = 0;
    const int rc = rn::walk_fill(op.w, blocks, cls_levels, box_levels, level_anchors, L, dtype, B, anchors, anchor_bstride, gt_boxes,
                                 gt_labels, gt_off, matches, special_rows, num_fg, reg_w, grad_prescale, out_loss, grad_cls_levels,
                                 workspace, workspace_bytes);
    if (rc != RN_OK) return rc;
    op.K = K; op.beta = beta; op.logit_shift = logit_shift;
    return rn::walk_launch<0, true>(op, blocks, dtype, grad_cls_levels != nullptr, 0.0f, out_loss, (hipStream_t)stream);
}
