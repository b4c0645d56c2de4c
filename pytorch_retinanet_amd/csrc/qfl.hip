// Quality Focal Loss on the matched rows' label elements: rn_quality_focal_loss.  The rule, step by step with its roundings, is in
// include/retinanet_hip.h; losses.box_quality_reference / losses.quality_focal_loss_reference restate it in torch.  Built without
// FMA contraction; steps 1-2 of the box rule (the quality) are rn_boxiou.hpp's, the code boxloss.hip runs.
//
// The call runs BEHIND a K3 call (loss.hip) with alpha = 1, gamma = beta: K3 has then written QFL's negative term for every
// background element, and a zero loss and a zero gradient for the label element of every matched row.  This call walks the matcher's
// flag words, computes the soft-target term of those label elements -- one element of about 0.3 % of the rows at the train shape --
// adds their sum to out_loss[0] and stores that one class gradient element per matched row.  Nothing else is touched.
//
// Shape: rn_box_iou_loss's.  One wave owns a strip of 64 flag words (4 096 rows) of ONE image per pass, one word per lane; the set
// bits are compacted into a per-wave LDS list that is worked off 64 rows at a time, one row per lane.  Latency-bound: per 64 listed
// rows one chain match -> (GT box, label) -> logit; the loads that do not hang on the match (anchor, deltas) go out with it, the GT
// box and the label go out together.  No bandwidth figure applies.
//
// Sum: every workgroup writes ONE double into its own slot of the workspace (always, zero included: no slot needs clearing), and a
// one-wave kernel behind it adds the slots in a fixed order onto out_loss[0].  No atomics, so two calls give the same bits.
#include "rn_boxiou.hpp"

namespace {

constexpr int QF_WAVES = 4;                       // waves per workgroup: one strip each per pass
constexpr int QF_BLOCK = QF_WAVES * RN_WAVE;
constexpr int QF_WORDS = RN_WAVE;                 // flag words per strip (one per lane)
constexpr int QF_ROWS = QF_WORDS * 64;            // rows per strip: 4 096, the capacity of a wave's list (offsets fit 16 bits)
constexpr int QF_MAX_BLOCKS = 128;                // grid cap: 512 strips per pass, as rn_box_iou_loss

using rn::box4;

struct QflLevel { const void *cls, *box; void *gcls; int64_t base, A_l; };

struct QflArgs {
    QflLevel lv[RN_MAX_LEVELS];
    int32_t L, B, K;
    int64_t A, W;                    // anchors per image, flag words per image
    const rn::f32x4 *anchors;
    int64_t anchor_bstride4;         // anchors (of four floats) between images; 0 = shared
    const rn::f32x4 *gt_boxes;
    const int64_t *gt_labels;
    const int32_t *gt_off;
    const int64_t *matches;
    const unsigned long long *special;
    const int32_t *num_fg;
    float reg_w[4];
    float beta, logit_shift, inv_B;
    const float *gscale;             // nullable
    double *partials;                // [gridDim.x]
    int32_t strips_per_image, total_strips;
};

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

template <int DT, bool WRITE_GRAD>
__global__ __launch_bounds__(QF_BLOCK) void quality_focal_loss_kernel(const QflArgs a)
{
    __shared__ unsigned short s_rows[QF_WAVES][QF_ROWS];      // flagged rows of the wave's strip (offsets from its first anchor)
    __shared__ double s_part[QF_WAVES];
    const int lane = threadIdx.x & (RN_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const float gs = a.gscale ? *a.gscale : 1.0f;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int64_t K = a.K;
    double acc = 0.0;
#pragma unroll 1
    for (int strip = (int)blockIdx.x * QF_WAVES + wave; strip < a.total_strips; strip += (int)gridDim.x * QF_WAVES) {
        const int b = strip / a.strips_per_image;
        const int64_t w0 = (int64_t)(strip - b * a.strips_per_image) * QF_WORDS;
        const int t0 = a.gt_off[b], T = a.gt_off[b + 1] - t0;
        unsigned long long word = 0ull;
        if (T > 0 && w0 + lane < a.W) word = a.special[(int64_t)b * a.W + w0 + lane];     // (an image without GT has no matched row)
        unsigned long long nz = __ballot(word != 0ull);
        if (!nz) continue;
        const int nf = a.num_fg[b];
        const float scale = (1.0f / (float)(nf > 1 ? nf : 1)) * a.inv_B;
        int n = 0;
        while (nz) {
            const int it = __ffsll((long long)nz) - 1;
            nz &= nz - 1;
            const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(word & 0xffffffffull), it);
            const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(word >> 32), it);
            const unsigned long long m = ((unsigned long long)hi << 32) | lo;
            if ((m >> lane) & 1ull) s_rows[wave][n + __popcll(m & below)] = (unsigned short)(it * 64 + lane);
            n += __popcll(m);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll 1
        for (int i0 = 0; i0 < n; i0 += RN_WAVE) {
            const bool have = i0 + lane < n;
            const int64_t ag = w0 * 64 + (have ? (int64_t)s_rows[wave][i0 + lane] : 0);
            const bool ok = have && ag < a.A;                                           // (bits past A in the last word, if any, are not rows)
            const void *clsp = a.lv[0].cls, *boxp = a.lv[0].box;
            void *gclsp = a.lv[0].gcls;
            int64_t base = 0, A_l = 1;
#pragma unroll 1
            for (int l = 0; l < a.L; ++l) {                                             // (l is wave-uniform: the level table stays in scalar registers)
                const bool in = ag >= a.lv[l].base && ag < a.lv[l].base + a.lv[l].A_l;
                if (in) { clsp = a.lv[l].cls; boxp = a.lv[l].box; gclsp = a.lv[l].gcls; base = a.lv[l].base; A_l = a.lv[l].A_l; }
            }
            const int64_t r = (int64_t)b * A_l + (ag - base);                           // row inside the level tensor
            // the loads of a listed row that do not hang on its match go out WITH the match (an ignored row pays for them in vain)
            int64_t pm = -1;
            rn::f32x4 an = {0.0f, 0.0f, 1.0f, 1.0f};
            float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (ok) {
                pm = a.matches[(int64_t)b * a.A + ag];                                  // (read through the flag words only)
                an = a.anchors[(int64_t)b * a.anchor_bstride4 + ag];
                box4<DT>::ld(boxp, r, d);
            }
            const bool matched = ok && pm >= 0;
            if (matched) {
                const int64_t gi = (int64_t)t0 + (pm < (int64_t)T ? pm : (int64_t)(T - 1));   // clamped into the image's rows
                const rn::f32x4 g = a.gt_boxes[gi];                                     // the GT box and the label: one round trip
                const int64_t c = a.gt_labels[gi] - 1;
                if (c >= 0 && c < K) {                                                  // (a label outside 1..K: the row adds and writes nothing)
                    const int64_t e = r * K + c;
                    const float x = rn::dt<DT>::ld(clsp, e);
                    const float q = rn::box_decode_iou(g, an, d, a.reg_w).iou;
                    float gr;
                    const float l = qfl_elem(x, q, a.beta, a.logit_shift, gr);
                    acc += (double)l * (double)scale;
                    if (WRITE_GRAD) rn::dt<DT>::st(gclsp, e, (gr * scale) * gs);
                }
            }
        }
        // the list is rewritten by the next strip: every lane has read its entries before any lane writes
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    const double accw = rn::wave_sum_d(acc);
    if (lane == 0) s_part[wave] = accw;
    __syncthreads();
    if (threadIdx.x == 0) {
        double c = 0.0;
#pragma unroll
        for (int w = 0; w < QF_WAVES; ++w) c += s_part[w];
        a.partials[blockIdx.x] = c;                                                     // every workgroup, every call: no stale slot
    }
}

// One wave: lane i adds slots i, i + 64, ... in order, then the fixed butterfly; the total goes ONTO out_loss[0] (K3's value).
__global__ __launch_bounds__(RN_WAVE) void quality_focal_loss_sum_kernel(const double *__restrict__ partials, const int n,
                                                                        float *__restrict__ out_loss)
{
    double s = 0.0;
    for (int i = (int)threadIdx.x; i < n; i += RN_WAVE) s += partials[i];
    s = rn::wave_sum_d(s);
    if (threadIdx.x == 0) out_loss[0] = (float)((double)out_loss[0] + s);
}

int grid_blocks(const int B, const int64_t A, int &strips_per_image, int &total_strips)
{
    const int64_t W = (A + 63) / 64;
    const int64_t spi = (W + QF_WORDS - 1) / QF_WORDS, total = spi * B;
    if (total > 0x7fffffff) return 0;
    strips_per_image = (int)spi; total_strips = (int)total;
    const int64_t blocks = (total + QF_WAVES - 1) / QF_WAVES;
    return (int)(blocks < QF_MAX_BLOCKS ? blocks : QF_MAX_BLOCKS);
}

template <int DT>
void launch(const QflArgs &a, const int blocks, const bool write_grad, hipStream_t s)
{
    if (write_grad) quality_focal_loss_kernel<DT, true><<<blocks, QF_BLOCK, 0, s>>>(a);
    else quality_focal_loss_kernel<DT, false><<<blocks, QF_BLOCK, 0, s>>>(a);
}

}  // namespace

RN_API size_t rn_quality_focal_loss_workspace_bytes(int B, int64_t A)
{
    if (B <= 0 || A <= 0) return 0;
    int spi = 0, total = 0;
    const int blocks = grid_blocks(B, A, spi, total);
    return (size_t)blocks * sizeof(double);
}

RN_API int rn_quality_focal_loss(const void *const *cls_levels, const void *const *box_levels, const int64_t *level_anchors, int L,
                                 int dtype, int B, int K, const float *anchors, int64_t anchor_bstride, const float *gt_boxes,
                                 const int64_t *gt_labels, const int32_t *gt_off, const int64_t *matches,
                                 const uint64_t *special_rows, const int32_t *num_fg, const float *reg_w, float beta,
                                 float logit_shift, const float *grad_prescale, float *out_loss, void *const *grad_cls_levels,
                                 void *workspace, size_t workspace_bytes, void *stream)
{
    if (!cls_levels || !box_levels || !level_anchors || !anchors || !gt_off || !matches || !special_rows || !num_fg || !reg_w ||
        !out_loss || !workspace)
        return RN_EINVAL;
    if (L <= 0 || L > RN_MAX_LEVELS || B <= 0 || K < 1 || anchor_bstride < 0 || (anchor_bstride & 3)) return RN_EINVAL;
    if (dtype != RN_F32 && dtype != RN_BF16 && dtype != RN_F16) return RN_EINVAL;
    if (!(beta >= 0.0f) || !(beta < INFINITY) || !(fabsf(logit_shift) < INFINITY)) return RN_EINVAL;
    for (int j = 0; j < 4; ++j)
        if (!(reg_w[j] > 0.0f) || !(reg_w[j] < INFINITY)) return RN_EINVAL;
    const size_t box_align = dtype == RN_F32 ? 16 : 8, cls_align = dtype == RN_F32 ? 4 : 2;
    QflArgs a{};
    int64_t A = 0;
    for (int l = 0; l < L; ++l) {
        if (level_anchors[l] < 0) return RN_EINVAL;
        if (level_anchors[l] > 0 && (!cls_levels[l] || !box_levels[l] || (grad_cls_levels && !grad_cls_levels[l]))) return RN_EINVAL;
        if (!rn::aligned(box_levels[l], box_align) || !rn::aligned(cls_levels[l], cls_align) ||
            (grad_cls_levels && !rn::aligned(grad_cls_levels[l], cls_align)))
            return RN_EALIGN;
        a.lv[l] = QflLevel{cls_levels[l], box_levels[l], grad_cls_levels ? grad_cls_levels[l] : nullptr, A, level_anchors[l]};
        A += level_anchors[l];
    }
    if (A <= 0) return RN_EINVAL;
    if (anchor_bstride != 0 && anchor_bstride < A * 4) return RN_EINVAL;
    if (!rn::aligned(anchors, 16) || !rn::aligned(gt_boxes, 16) || !rn::aligned(gt_labels, 8) || !rn::aligned(matches, 8) ||
        !rn::aligned(special_rows, 8) || !rn::aligned(gt_off, 4) || !rn::aligned(num_fg, 4) || !rn::aligned(out_loss, 4) ||
        !rn::aligned(grad_prescale, 4) || !rn::aligned(workspace, 16))
        return RN_EALIGN;
    int spi = 0, total = 0;
    const int blocks = grid_blocks(B, A, spi, total);
    if (blocks <= 0) return RN_EINVAL;
    if (workspace_bytes < (size_t)blocks * sizeof(double)) return RN_EWORKSPACE;
    a.L = L; a.B = B; a.K = K;
    a.A = A; a.W = (A + 63) / 64;
    a.anchors = (const rn::f32x4 *)anchors;
    a.anchor_bstride4 = anchor_bstride / 4;
    a.gt_boxes = (const rn::f32x4 *)gt_boxes;       // (may be null, as gt_labels, when no image has GT: then no flag word is read)
    a.gt_labels = gt_labels;
    a.gt_off = gt_off;
    a.matches = matches;
    a.special = (const unsigned long long *)special_rows;
    a.num_fg = num_fg;
    for (int j = 0; j < 4; ++j) a.reg_w[j] = reg_w[j];
    a.beta = beta; a.logit_shift = logit_shift;
    a.inv_B = 1.0f / (float)B;
    a.gscale = grad_prescale;
    a.partials = (double *)workspace;
    a.strips_per_image = spi; a.total_strips = total;
    hipStream_t s = (hipStream_t)stream;
    const bool wg = grad_cls_levels != nullptr;
    if (dtype == RN_F32) launch<RN_F32>(a, blocks, wg, s);
    else if (dtype == RN_BF16) launch<RN_BF16>(a, blocks, wg, s);
    else launch<RN_F16>(a, blocks, wg, s);
    RN_LAUNCH_CHECK();
    quality_focal_loss_sum_kernel<<<1, RN_WAVE, 0, s>>>(a.partials, blocks, out_loss);
    RN_LAUNCH_CHECK();
    return RN_OK;
}
