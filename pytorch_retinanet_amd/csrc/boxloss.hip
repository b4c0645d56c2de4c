// IoU-type box regression losses (GIoU, DIoU) on the matched rows: rn_box_iou_loss.  The rule, step by step with its roundings, is
// in include/retinanet_hip.h; losses.box_iou_loss_reference restates it in torch.  Built without FMA contraction.
//
// The call runs BEHIND K3 (loss.hip), which has already written grad_box for every row (zeros for background / ignored rows, the
// smooth-L1 gradients for matched ones) and out_loss[1].  It walks the matcher's flag words, recomputes the loss of the matched rows
// -- about 0.3 % of the rows at the train shape -- and overwrites those rows' gradients and out_loss[1].  Nothing else is touched.
//
// Shape: one wave owns a strip of 64 flag words (4 096 rows) of ONE image per pass, one word per lane.  The set bits of the strip are
// compacted into a per-wave LDS list, and the list is worked off 64 rows at a time, one row per lane: matches -> (GT box, anchor,
// deltas) -> the four gradients.  The chain of dependent loads therefore runs once per 64 matched rows, not once per flag word.
// Latency-bound: a few thousand rows, each a chain of two dependent loads; no bandwidth figure applies.
//
// Sum: every workgroup writes ONE double into its own slot of the workspace (always, zero included: no slot needs clearing), and a
// one-wave kernel behind it adds the slots in a fixed order.  No atomics, so two calls give the same bits.
#include "rn_boxiou.hpp"

namespace {

constexpr int BL_WAVES = 4;                       // waves per workgroup: one strip each per pass
constexpr int BL_BLOCK = BL_WAVES * RN_WAVE;
constexpr int BL_WORDS = RN_WAVE;                 // flag words per strip (one per lane)
constexpr int BL_ROWS = BL_WORDS * 64;            // rows per strip: 4 096, the capacity of a wave's list (offsets fit 16 bits)
constexpr int BL_MAX_BLOCKS = 128;                // grid cap: 512 strips = 2 097 152 rows per pass (the train shape, B = 8, A = 201 600, is 400 strips)

using rn::box4;

struct BoxLossLevel { const void *box; void *gbox; int64_t base, A_l; };

struct BoxLossArgs {
    BoxLossLevel lv[RN_MAX_LEVELS];
    int32_t L, B, kind;
    int64_t A, W;                    // anchors per image, flag words per image
    const rn::f32x4 *anchors;
    int64_t anchor_bstride4;         // anchors (of four floats) between images; 0 = shared
    const rn::f32x4 *gt_boxes;
    const int32_t *gt_off;
    const int64_t *matches;
    const unsigned long long *special;
    const int32_t *num_fg;
    float reg_w[4];
    float loss_weight, inv_B;
    const float *gscale;             // nullable
    double *partials;                // [gridDim.x]
    int32_t strips_per_image, total_strips;
};

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

template <int DT, bool WRITE_GRAD>
__global__ __launch_bounds__(BL_BLOCK) void box_iou_loss_kernel(const BoxLossArgs a)
{
    __shared__ unsigned short s_rows[BL_WAVES][BL_ROWS];      // flagged rows of the wave's strip (offsets from its first anchor)
    __shared__ double s_part[BL_WAVES];
    const int lane = threadIdx.x & (RN_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const float gs = a.gscale ? *a.gscale : 1.0f;
    const unsigned long long below = (1ull << lane) - 1ull;
    double acc = 0.0;
#pragma unroll 1
    for (int strip = (int)blockIdx.x * BL_WAVES + wave; strip < a.total_strips; strip += (int)gridDim.x * BL_WAVES) {
        const int b = strip / a.strips_per_image;
        const int64_t w0 = (int64_t)(strip - b * a.strips_per_image) * BL_WORDS;
        const int t0 = a.gt_off[b], T = a.gt_off[b + 1] - t0;
        unsigned long long word = 0ull;
        if (T > 0 && w0 + lane < a.W) word = a.special[(int64_t)b * a.W + w0 + lane];     // (an image without GT has no matched row)
        unsigned long long nz = __ballot(word != 0ull);
        if (!nz) continue;
        const int nf = a.num_fg[b];
        const float scale = (1.0f / (float)(nf > 1 ? nf : 1)) * a.inv_B;
        const float gmul = (a.loss_weight * scale) * gs;
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
            const void *boxp = a.lv[0].box;
            void *gboxp = a.lv[0].gbox;
            int64_t base = 0, A_l = 1;
#pragma unroll 1
            for (int l = 0; l < a.L; ++l) {                                             // (l is wave-uniform: the level table stays in scalar registers)
                const bool in = ag >= a.lv[l].base && ag < a.lv[l].base + a.lv[l].A_l;
                if (in) { boxp = a.lv[l].box; gboxp = a.lv[l].gbox; base = a.lv[l].base; A_l = a.lv[l].A_l; }
            }
            const int64_t r = (int64_t)b * A_l + (ag - base);                           // row inside the level tensor
            int64_t pm = -1;
            if (ok) pm = a.matches[(int64_t)b * a.A + ag];                              // (read through the flag words only)
            const bool matched = ok && pm >= 0;
            if (matched) {
                const int64_t gi = (int64_t)t0 + (pm < (int64_t)T ? pm : (int64_t)(T - 1));   // clamped into the image's rows
                const rn::f32x4 g = a.gt_boxes[gi];
                const rn::f32x4 an = a.anchors[(int64_t)b * a.anchor_bstride4 + ag];
                float d[4], gb[4];
                box4<DT>::ld(boxp, r, d);
                const float l = iou_row(g, an, d, a.reg_w, a.kind, gb);
                acc += (double)l * (double)scale;
                if (WRITE_GRAD) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) gb[j] *= gmul;
                    box4<DT>::st(gboxp, r, gb);
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
        for (int w = 0; w < BL_WAVES; ++w) c += s_part[w];
        a.partials[blockIdx.x] = c;                                                     // every workgroup, every call: no stale slot
    }
}

// One wave: lane i adds slots i, i + 64, ... in order, then the fixed butterfly; out_loss[1] only.
__global__ __launch_bounds__(RN_WAVE) void box_iou_loss_sum_kernel(const double *__restrict__ partials, const int n, const float loss_weight,
                                                                  float *__restrict__ out_loss)
{
    double s = 0.0;
    for (int i = (int)threadIdx.x; i < n; i += RN_WAVE) s += partials[i];
    s = rn::wave_sum_d(s);
    if (threadIdx.x == 0) out_loss[1] = (float)((double)loss_weight * s);
}

int grid_blocks(const int B, const int64_t A, int &strips_per_image, int &total_strips)
{
    const int64_t W = (A + 63) / 64;
    const int64_t spi = (W + BL_WORDS - 1) / BL_WORDS, total = spi * B;
    if (total > 0x7fffffff) return 0;
    strips_per_image = (int)spi; total_strips = (int)total;
    const int64_t blocks = (total + BL_WAVES - 1) / BL_WAVES;
    return (int)(blocks < BL_MAX_BLOCKS ? blocks : BL_MAX_BLOCKS);
}

template <int DT>
void launch(const BoxLossArgs &a, const int blocks, const bool write_grad, hipStream_t s)
{
    if (write_grad) box_iou_loss_kernel<DT, true><<<blocks, BL_BLOCK, 0, s>>>(a);
    else box_iou_loss_kernel<DT, false><<<blocks, BL_BLOCK, 0, s>>>(a);
}

}  // namespace

RN_API size_t rn_box_iou_loss_workspace_bytes(int B, int64_t A)
{
    if (B <= 0 || A <= 0) return 0;
    int spi = 0, total = 0;
    const int blocks = grid_blocks(B, A, spi, total);
    return (size_t)blocks * sizeof(double);
}

RN_API int rn_box_iou_loss(const void *const *box_levels, const int64_t *level_anchors, int L, int dtype, int B,
                           const float *anchors, int64_t anchor_bstride, const float *gt_boxes, const int32_t *gt_off,
                           const int64_t *matches, const uint64_t *special_rows, const int32_t *num_fg,
                           const float *reg_w, int kind, float loss_weight, const float *grad_prescale,
                           float *out_loss, void *const *grad_box_levels, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!box_levels || !level_anchors || !anchors || !gt_off || !matches || !special_rows || !num_fg || !reg_w || !out_loss || !workspace)
        return RN_EINVAL;
    if (L <= 0 || L > RN_MAX_LEVELS || B <= 0 || anchor_bstride < 0 || (anchor_bstride & 3)) return RN_EINVAL;
    if (dtype != RN_F32 && dtype != RN_BF16 && dtype != RN_F16) return RN_EINVAL;
    if (kind != RN_BOX_LOSS_GIOU && kind != RN_BOX_LOSS_DIOU) return RN_EINVAL;
    if (!(loss_weight > 0.0f) || !(loss_weight < INFINITY)) return RN_EINVAL;
    for (int j = 0; j < 4; ++j)
        if (!(reg_w[j] > 0.0f) || !(reg_w[j] < INFINITY)) return RN_EINVAL;
    const size_t box_align = dtype == RN_F32 ? 16 : 8;
    BoxLossArgs a{};
    int64_t A = 0;
    for (int l = 0; l < L; ++l) {
        if (level_anchors[l] < 0) return RN_EINVAL;
        if (level_anchors[l] > 0 && (!box_levels[l] || (grad_box_levels && !grad_box_levels[l]))) return RN_EINVAL;
        if (!rn::aligned(box_levels[l], box_align) || (grad_box_levels && !rn::aligned(grad_box_levels[l], box_align))) return RN_EALIGN;
        a.lv[l] = BoxLossLevel{box_levels[l], grad_box_levels ? grad_box_levels[l] : nullptr, A, level_anchors[l]};
        A += level_anchors[l];
    }
    if (A <= 0) return RN_EINVAL;
    if (anchor_bstride != 0 && anchor_bstride < A * 4) return RN_EINVAL;
    if (!rn::aligned(anchors, 16) || !rn::aligned(gt_boxes, 16) || !rn::aligned(matches, 8) || !rn::aligned(special_rows, 8) ||
        !rn::aligned(gt_off, 4) || !rn::aligned(num_fg, 4) || !rn::aligned(out_loss, 4) || !rn::aligned(grad_prescale, 4) ||
        !rn::aligned(workspace, 16))
        return RN_EALIGN;
    int spi = 0, total = 0;
    const int blocks = grid_blocks(B, A, spi, total);
    if (blocks <= 0) return RN_EINVAL;
    if (workspace_bytes < (size_t)blocks * sizeof(double)) return RN_EWORKSPACE;
    a.L = L; a.B = B; a.kind = kind;
    a.A = A; a.W = (A + 63) / 64;
    a.anchors = (const rn::f32x4 *)anchors;
    a.anchor_bstride4 = anchor_bstride / 4;
    a.gt_boxes = (const rn::f32x4 *)gt_boxes;       // (may be null when no image has GT: then no flag word is read)
    a.gt_off = gt_off;
    a.matches = matches;
    a.special = (const unsigned long long *)special_rows;
    a.num_fg = num_fg;
    for (int j = 0; j < 4; ++j) a.reg_w[j] = reg_w[j];
    a.loss_weight = loss_weight;
    a.inv_B = 1.0f / (float)B;
    a.gscale = grad_prescale;
    a.partials = (double *)workspace;
    a.strips_per_image = spi; a.total_strips = total;
    hipStream_t s = (hipStream_t)stream;
    const bool wg = grad_box_levels != nullptr;
    if (dtype == RN_F32) launch<RN_F32>(a, blocks, wg, s);
    else if (dtype == RN_BF16) launch<RN_BF16>(a, blocks, wg, s);
    else launch<RN_F16>(a, blocks, wg, s);
    RN_LAUNCH_CHECK();
    box_iou_loss_sum_kernel<<<1, RN_WAVE, 0, s>>>(a.partials, blocks, loss_weight, out_loss);
    RN_LAUNCH_CHECK();
    return RN_OK;
}
