// ATSS anchor matcher (Adaptive Training Sample Selection, Zhang et al., CVPR 2020) -- the second matcher beside K2 (match.hip).
// It fills K2's three outputs (matches, num_fg, the special-row flag words), so K3 and everything around it are unchanged.  The rule
// is written out, rounding by rounding, in include/retinanet_hip.h ("ATSS matcher", steps 1-6); box_utils.atss_matcher restates it.
//
// Four launches, no synchronisation, gt_off read on the device only; the grids are sized by the host's upper bound on the GT rows
// and a workgroup whose row lies beyond gt_off[B] exits:
//   assign_prep_kernel  (rn_assign.hpp) the flag words = 0, num_fg = 0 (unless the caller zeroed it), matches = -1 (unless FLAGGED_ONLY).
//   atss_select_kernel  one workgroup per (GT row, level): the k_l anchors of the level that are smallest under (d2, index).  The key
//                       is 64-bit -- d2's bit pattern (non-negative floats order as unsigned integers) above the anchor's index inside
//                       the level -- so keys are unique and the tie rule is part of the order.  ONE walk over the level's anchors: a key
//                       not above the running threshold is appended to an LDS buffer; when the buffer passes SEL_KMAX entries a radix
//                       select over it (8-bit digits from the top, LDS histogram) finds the k-th smallest key, the buffer is compacted
//                       to the k keys not above it and that key is the new threshold.  The threshold is never below the level's true
//                       k-th key, so the k survivors at the end are the level's k smallest whatever the order of the appends; a rank
//                       sort puts them in ascending order and writes (anchor index, fp32 IoU) records into the workspace.
//   atss_stats_kernel   one wave per GT row: the two serial double sums of step 3 in list order (every lane adds the same values in
//                       the same order, fetched with v_readlane from a 64-candidate register), then the candidates across lanes: a
//                       positive one goes into the [B][A] key table with a 64-bit integer atomicMax of (IoU bits << 32) | ~gt index
//                       -- order-independent, so the same bits on every call -- and every other record's index becomes -1.
//   assign_emit_kernel  (rn_assign.hpp, shared with tal.hip) one thread per record: the record whose key IS the table's entry won
//                       the anchor: it writes matches, sets the flag bit, counts into num_fg and puts the entry back to zero.  The table is zero on entry and zero again on
//                       exit without a clear of its B * A * 8 bytes.
// Compiled without FMA contraction (EXACT in the Makefile): every fp32 and fp64 step below is one correctly rounded operation.
#include "rn_assign.hpp"
#include "rn_common.hpp"
#include "rn_match.hpp"

namespace {

using rn_assign::append;
using rn_assign::centre;
using rn_assign::image_of_row;
using rn_assign::u64;

constexpr int SEL_BLOCK = 1024;
constexpr int SEL_U = 4;                                // anchors per thread and step: four independent 16-byte loads in flight
constexpr int SEL_STEP = SEL_BLOCK * SEL_U;
constexpr int SEL_KMAX = 2048;                          // largest k_l; the buffer is compacted once it holds more
constexpr int SEL_CAP = SEL_KMAX + SEL_STEP;            // (48 KiB of keys: a step appends at most SEL_STEP)
constexpr int SEL_PER = SEL_CAP / SEL_BLOCK;

struct Levels {
    int64_t off[RN_MAX_LEVELS + 1];                     // anchor range of level l inside A
    int k[RN_MAX_LEVELS];                               // k_l = min(topk * cells[l], A_l)
    int koff[RN_MAX_LEVELS];                            // first record of level l in a row's candidate list
    int idx_bytes[RN_MAX_LEVELS];                       // bytes of an index inside the level that can be non-zero
};

// the key of the order (d2, index) of step 2 (the centres of step 1: rn_assign::centre)
__device__ __forceinline__ u64 d2_key(const rn::f32x4 a, const float gcx, const float gcy, const uint32_t i)
{
    const float dx = centre(a.x, a.z) - gcx, dy = centre(a.y, a.w) - gcy;
    const float xx = dx * dx, yy = dy * dy;
    const float d2 = xx + yy;
    return ((u64)__float_as_uint(d2) << 32) | i;
}

// the select's compaction at this kernel's block size (rn_assign.hpp)
__device__ __forceinline__ void shrink(u64 *__restrict__ s_key, int *__restrict__ s_hist, int *__restrict__ s_ctl, u64 *__restrict__ s_thr,
                                       const int n, const int k, const int idx_bytes)
{
    rn_assign::shrink<SEL_BLOCK, SEL_PER>(s_key, s_hist, s_ctl, s_thr, n, k, idx_bytes);
}

__global__ __launch_bounds__(SEL_BLOCK) void atss_select_kernel(
    const rn::f32x4 *__restrict__ anchors, const int64_t anchor_bstride4, const rn::f32x4 *__restrict__ gt,
    const int32_t *__restrict__ gt_off, const int B, const int n_tot, const Levels lv, int32_t *__restrict__ cand_idx,
    float *__restrict__ cand_iou)
{
    __shared__ u64 s_key[SEL_CAP];
    __shared__ int s_hist[256];
    __shared__ int s_ctl[4];                            // [0] keys in the buffer; [1..3] shrink's bin, keys below it, keys in it
    __shared__ u64 s_thr;

    const int tid = threadIdx.x;
    const int r = blockIdx.x, l = blockIdx.y, k = lv.k[l];
    const int row = gt_off[0] + r;
    if (k == 0 || row >= gt_off[B]) return;             // (workgroup-uniform)
    const int b = image_of_row(gt_off, B, row);
    const rn::f32x4 g = gt[row];
    const float gcx = centre(g.x, g.z), gcy = centre(g.y, g.w);
    const rn::f32x4 *__restrict__ an = anchors + (int64_t)b * anchor_bstride4 + lv.off[l];
    const int Al = (int)(lv.off[l + 1] - lv.off[l]);

    if (tid == 0) { s_ctl[0] = 0; s_thr = ~0ull; }
    __syncthreads();
    for (int base = 0; base < Al; base += SEL_STEP) {
        const u64 thr = s_thr;
        rn::f32x4 a[SEL_U];
#pragma unroll
        for (int u = 0; u < SEL_U; ++u) {
            const int i = base + u * SEL_BLOCK + tid;
            a[u] = rn::f32x4{0.f, 0.f, 0.f, 0.f};
            if (i < Al) a[u] = an[i];
        }
#pragma unroll
        for (int u = 0; u < SEL_U; ++u) {
            const int i = base + u * SEL_BLOCK + tid;
            const u64 key = d2_key(a[u], gcx, gcy, (uint32_t)i);
            append(s_key, &s_ctl[0], i < Al && key <= thr, key);
        }
        __syncthreads();
        const int n = s_ctl[0];
        __syncthreads();                                // everyone holds n before the next append moves the counter
        if (n > SEL_KMAX) shrink(s_key, s_hist, s_ctl, &s_thr, n, k, lv.idx_bytes[l]);
    }
    {
        const int n = s_ctl[0];
        __syncthreads();
        if (n > k) shrink(s_key, s_hist, s_ctl, &s_thr, n, k, lv.idx_bytes[l]);
    }
    // the k keys in ascending order: a record's place is the number of smaller keys (every lane reads the same LDS word: a broadcast)
    const float area_g = (g.z - g.x) * (g.w - g.y);
    for (int t = tid; t < k; t += SEL_BLOCK) {
        const u64 key = s_key[t];
        int rank = 0;
        for (int j = 0; j < k; ++j) rank += s_key[j] < key ? 1 : 0;
        const uint32_t i = (uint32_t)key;
        const rn::f32x4 a = an[i];
        const float iou = rn_match::iou_pair(g, area_g, a, (a.z - a.x) * (a.w - a.y));
        const int64_t o = (int64_t)r * n_tot + lv.koff[l] + rank;
        cand_idx[o] = (int32_t)(lv.off[l] + i);
        cand_iou[o] = iou;
    }
}

// steps 3-5 for one GT row per wave
__global__ __launch_bounds__(RN_WAVE) void atss_stats_kernel(
    const rn::f32x4 *__restrict__ anchors, const int64_t anchor_bstride4, const rn::f32x4 *__restrict__ gt,
    const int32_t *__restrict__ gt_off, const int B, const int64_t A, const int n, int32_t *__restrict__ cand_idx,
    const float *__restrict__ cand_iou, u64 *__restrict__ keys)
{
    const int lane = threadIdx.x;
    const int r = blockIdx.x;
    const int row = gt_off[0] + r;
    if (row >= gt_off[B]) return;
    const int b = image_of_row(gt_off, B, row);
    const uint32_t gi = (uint32_t)(row - gt_off[b]);
    const rn::f32x4 g = gt[row];
    const float *__restrict__ iou = cand_iou + (int64_t)r * n;
    int32_t *__restrict__ idx = cand_idx + (int64_t)r * n;

    double sum = 0.0;
    for (int c = 0; c < n; c += RN_WAVE) {
        const float v = c + lane < n ? iou[c + lane] : 0.0f;
        const int m = min(RN_WAVE, n - c);
        for (int j = 0; j < m; ++j) sum += (double)rn_match::lane_f(v, j);
    }
    const double mean = sum / (double)n;
    double ss = 0.0;
    for (int c = 0; c < n; c += RN_WAVE) {
        const float v = c + lane < n ? iou[c + lane] : 0.0f;
        const int m = min(RN_WAVE, n - c);
        for (int j = 0; j < m; ++j) {
            const double d = (double)rn_match::lane_f(v, j) - mean;
            const double dd = d * d;
            ss += dd;
        }
    }
    const double var = n > 1 ? ss / (double)(n - 1) : 0.0;

    for (int c = lane; c < n; c += RN_WAVE) {
        const float v = iou[c];
        const int a_idx = idx[c];
        const double dev = (double)v - mean;
        bool pos = dev >= 0.0 && dev * dev >= var;
        if (pos) {
            const rn::f32x4 a = anchors[(int64_t)b * anchor_bstride4 + a_idx];
            const float acx = centre(a.x, a.z), acy = centre(a.y, a.w);
            const float inside = fminf(fminf(acx - g.x, acy - g.y), fminf(g.z - acx, g.w - acy));
            pos = inside > 0.01f;
        }
        if (pos) rn_assign::table_post(keys, (int64_t)b * A + a_idx, v, gi);
        else idx[c] = -1;
    }
}

// the level layout -> per-level k_l and record offsets.  RN_OK, RN_EINVAL or RN_EUNSUPPORTED.
int layout(const int64_t A, const int64_t *level_off, const int32_t *cells, const int L, const int topk, Levels &lv, int &n_tot)
{
    if (!level_off || !cells || L <= 0 || L > RN_MAX_LEVELS || topk <= 0 || A <= 0 || A > 0x7fffffff) return RN_EINVAL;
    if (level_off[0] != 0 || level_off[L] != A) return RN_EINVAL;
    int64_t n = 0;
    for (int l = 0; l < L; ++l) {
        const int64_t Al = level_off[l + 1] - level_off[l];
        if (Al < 0 || cells[l] <= 0) return RN_EINVAL;
        const int64_t want = (int64_t)topk * cells[l];
        const int64_t k = want < Al ? want : Al;
        if (k > SEL_KMAX) return RN_EUNSUPPORTED;
        lv.off[l] = level_off[l];
        lv.k[l] = (int)k;
        lv.koff[l] = (int)n;
        int nb = 1;
        while (nb < 4 && ((Al - 1) >> (8 * nb)) > 0) ++nb;
        lv.idx_bytes[l] = nb;
        n += k;
    }
    lv.off[L] = A;
    for (int l = L; l < RN_MAX_LEVELS; ++l) { lv.off[l + 1] = A; lv.k[l] = 0; lv.koff[l] = (int)n; lv.idx_bytes[l] = 1; }
    n_tot = (int)n;
    return RN_OK;
}

using rn_assign::align16;

}  // namespace

RN_API size_t rn_atss_match_workspace_bytes(int B, int64_t A, int64_t total_gt, const int64_t *level_off, const int32_t *cells,
                                            int L, int topk)
{
    Levels lv;
    int n_tot = 0;
    if (B <= 0 || total_gt < 0 || layout(A, level_off, cells, L, topk, lv, n_tot) != RN_OK) return 0;
    return align16(sizeof(u64) * (size_t)B * (size_t)A) + 2 * align16(sizeof(int32_t) * (size_t)total_gt * (size_t)n_tot);
}

RN_API int rn_atss_match(const float *anchors, int64_t anchor_bstride, const float *gt_boxes, const int32_t *gt_off, int B, int64_t A,
                         const int64_t *level_off, const int32_t *cells, int L, int topk, int64_t *matches, int32_t *num_fg,
                         uint64_t *special_rows, int64_t total_gt, int flags, void *workspace, size_t workspace_bytes, void *stream)
{
    if (flags & ~(RN_MATCH_NUM_FG_ZEROED | RN_MATCH_FLAGGED_ONLY)) return RN_EINVAL;
    if ((flags & RN_MATCH_FLAGGED_ONLY) && !special_rows) return RN_EINVAL;
    if (!anchors || !gt_off || !matches || !workspace || B <= 0 || B > 65535 || total_gt < 0 || total_gt > 0x7fffffff) return RN_EINVAL;
    if (total_gt > 0 && !gt_boxes) return RN_EINVAL;
    Levels lv;
    int n_tot = 0;
    const int rc = layout(A, level_off, cells, L, topk, lv, n_tot);
    if (rc != RN_OK) return rc;
    if (!rn::aligned(anchors, 16) || (gt_boxes && !rn::aligned(gt_boxes, 16)) || (anchor_bstride & 3) || !rn::aligned(workspace, 16) ||
        (special_rows && !rn::aligned(special_rows, 8)))
        return RN_EALIGN;
    const size_t key_bytes = align16(sizeof(u64) * (size_t)B * (size_t)A);
    const size_t rec_bytes = align16(sizeof(int32_t) * (size_t)total_gt * (size_t)n_tot);
    if (workspace_bytes < key_bytes + 2 * rec_bytes) return RN_EWORKSPACE;
    u64 *keys = (u64 *)workspace;
    int32_t *cand_idx = (int32_t *)((char *)workspace + key_bytes);
    float *cand_iou = (float *)((char *)workspace + key_bytes + rec_bytes);
    u64 *special = (u64 *)special_rows;
    hipStream_t st = (hipStream_t)stream;
    const int prc = rn_assign::launch_prep(B, A, matches, num_fg, special, flags, st);
    if (prc != RN_OK) return prc;
    if (total_gt == 0 || n_tot == 0) return RN_OK;         // no GT rows anywhere: all background
    hipLaunchKernelGGL(atss_select_kernel, dim3((unsigned)total_gt, (unsigned)L), dim3(SEL_BLOCK), 0, st, (const rn::f32x4 *)anchors,
                       anchor_bstride / 4, (const rn::f32x4 *)gt_boxes, gt_off, B, n_tot, lv, cand_idx, cand_iou);
    RN_LAUNCH_CHECK();
    hipLaunchKernelGGL(atss_stats_kernel, dim3((unsigned)total_gt), dim3(RN_WAVE), 0, st, (const rn::f32x4 *)anchors, anchor_bstride / 4,
                       (const rn::f32x4 *)gt_boxes, gt_off, B, A, n_tot, cand_idx, cand_iou, keys);
    RN_LAUNCH_CHECK();
    return rn_assign::launch_emit(total_gt, n_tot, gt_off, B, A, cand_idx, cand_iou, keys, matches, num_fg, special, st);
}
