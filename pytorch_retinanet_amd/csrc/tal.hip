// Task-aligned anchor matcher (TAL: Feng et al., "TOOD", ICCV 2021; the assigner of PP-YOLOE, YOLOv8 and RTMDet-style heads) -- the
// third matcher beside K2 (match.hip) and ATSS (atss.hip).  It fills K2's three outputs (matches, num_fg, the special-row flag
// words), so K3 and everything behind it are unchanged; unlike the other two it READS the head's outputs: per object the positives
// are the topk anchors with the largest score^alpha * IoU^beta among the anchors whose centre lies inside the box.  The rule is
// written out, rounding by rounding, in include/retinanet_hip.h ("Task-aligned matcher", steps 1-5); box_utils.task_aligned_matcher
// restates it.  The decode and the IoU are rn_boxiou.hpp's (the code boxloss.hip and qfl.hip run), the select, the conflict table
// and the emit are rn_assign.hpp's (the code atss.hip runs).
//
// Four launches, no synchronisation, gt_off and the labels read on the device only; the grids are sized by the host's upper bound on
// the GT rows and a workgroup whose row lies beyond gt_off[B] exits:
//   assign_prep_kernel  the flag words = 0, num_fg = 0 (unless the caller zeroed it), matches = -1 (unless FLAGGED_ONLY).
//   tal_select_kernel   one workgroup per (GT row, level).  It visits the RECTANGLE of grid cells under its box, not the level: with
//                       the level's grid width from the host, the first and last column / row whose centre can lie inside the box
//                       come from the level's first anchors (centre of cell (0, 0) and the steps to (0, 1) and (1, 0)), widened by
//                       one cell on every side; every visited anchor is then tested with the rule's own strict comparison, so the
//                       rectangle only bounds the walk and never decides.  (Without a grid width the level is walked whole.)  Per
//                       visited anchor ONE round trip: the anchor, one logit element and the row's four deltas go out together.
//                       A candidate's key is 64-bit -- the complement of the metric's bit pattern (positive floats order as unsigned
//                       integers) above the anchor's index inside the level -- so keys are unique, the smallest key is the largest
//                       metric and the tie rule is part of the order.  Keys not above the running threshold go into an LDS list;
//                       when the list passes LIST_KEYS entries rn_assign's radix select compacts it to the topk smallest and that
//                       key is the new threshold.  The survivors (at most topk) are written as (anchor, metric, IoU) records.
//   tal_merge_kernel    one wave per GT row: the levels' L * topk records -> the row's topk smallest keys, by rank; a selected record
//                       goes into the [B][A] table with the 64-bit atomicMax of (IoU bits << 32) | ~gt index, every other record's
//                       index becomes -1.
//   assign_emit_kernel  the record whose key IS the table's entry won the anchor (rn_assign.hpp).
// No [T, A] matrix, no float atomics; nothing but the once-zeroed table needs a value on entry; two calls give the same bits.
// Latency-bound (a few thousand gathered rows, each one round trip); not tuned.
// Compiled without FMA contraction (EXACT in the Makefile): every fp32 step below is one correctly rounded operation.
#include "rn_assign.hpp"
#include "rn_boxiou.hpp"
#include "rn_rowwalk.hpp"

namespace {

using rn_assign::align16;
using rn_assign::append;
using rn_assign::centre;
using rn_assign::image_of_row;
using rn_assign::u64;

constexpr int TAL_BLOCK = 256;
constexpr int TAL_U = 2;                                // anchors per thread and step: their three loads each go out together
constexpr int TAL_STEP = TAL_BLOCK * TAL_U;
constexpr int TAL_LIST_KEYS = 1024;                     // the list is compacted once it holds more
constexpr int TAL_CAP = TAL_LIST_KEYS + TAL_STEP;       // (12 KiB of keys: a step appends at most TAL_STEP)
constexpr int TAL_PER = TAL_CAP / TAL_BLOCK;
constexpr int TAL_TOPK_MAX = 64;                        // the merge ranks L * topk <= 512 keys in LDS
constexpr int TAL_EXP_MAX = 8;

struct TalArgs {
    rn::WalkLevel lv[RN_MAX_LEVELS];                    // the level's class and box outputs, its first anchor and its anchor count
    int W[RN_MAX_LEVELS];                               // grid locations per grid row; 0 = unknown: the level is walked whole
    int cells[RN_MAX_LEVELS];                           // anchors per grid location
    int idx_bytes[RN_MAX_LEVELS];                       // bytes of an index inside the level that can be non-zero
    int32_t L, B, K, topk, alpha, beta;
    int64_t A;
    const rn::f32x4 *anchors;
    int64_t anchor_bstride4;
    const rn::f32x4 *gt;
    const int64_t *labels;
    const int32_t *gt_off;
    float reg_w[4];
    float logit_shift;
    int32_t *cand_idx;                                  // [rows][L * topk] records: the anchor (-1: none), its IoU and its metric
    float *cand_iou, *cand_m;
};

// step 2 of the rule from the loaded values: the metric m and the IoU u; false = the candidate is dropped
__device__ __forceinline__ bool metric(const TalArgs &a, const rn::f32x4 g, const rn::f32x4 an, const float x, const float (&d)[4],
                                       float &m, float &u)
{
    const float z = x + a.logit_shift;
    const float e = expf(-fabsf(z));                    // the QFL rule's sigmoid (qfl.hip, qfl_elem)
    const float r = 1.0f / (1.0f + e);
    const float s = z >= 0.0f ? r : e * r;
    u = rn::box_decode_iou(g, an, d, a.reg_w).iou;
    m = 1.0f;
    for (int j = 0; j < a.alpha; ++j) m = m * s;
    for (int j = 0; j < a.beta; ++j) m = m * u;
    return m > 0.0f && m < INFINITY && u >= 0.0f;
}

__device__ __forceinline__ u64 metric_key(const float m, const uint32_t i) { return ((u64)(uint32_t)~__float_as_uint(m) << 32) | i; }

// [first, last] of the grid columns (rows) whose centre c0 + j * step can lie strictly inside (lo, hi), widened by one; j in 0..n-1
__device__ __forceinline__ void span(const float c0, const float step, const float lo, const float hi, const int n, int &first, int &last)
{
    first = 0; last = n - 1;
    if (n > 1 && step > 0.0f) {
        const float top = (float)(n - 1);
        first = (int)fminf(fmaxf(floorf((lo - c0) / step), 0.0f), top);
        last = (int)fminf(fmaxf(ceilf((hi - c0) / step), 0.0f), top);
    }
}

template <int DT>
__global__ __launch_bounds__(TAL_BLOCK) void tal_select_kernel(const TalArgs a)
{
    __shared__ u64 s_key[TAL_CAP];
    __shared__ int s_hist[256];
    __shared__ int s_ctl[4];                            // [0] keys in the list; [1..3] shrink's bin, keys below it, keys in it
    __shared__ u64 s_thr;

    const int tid = threadIdx.x;
    const int r = blockIdx.x, l = blockIdx.y, k = a.topk;
    const int row = a.gt_off[0] + r;
    if (row >= a.gt_off[a.B]) return;                   // (workgroup-uniform)
    const int b = image_of_row(a.gt_off, a.B, row);
    const rn::WalkLevel lv = a.lv[l];
    const int64_t out0 = (int64_t)r * (a.L * k) + l * k;
    const rn::f32x4 g = a.gt[row];
    const int64_t c = a.labels[row] - 1;
    const bool finite = fabsf(g.x) < INFINITY && fabsf(g.y) < INFINITY && fabsf(g.z) < INFINITY && fabsf(g.w) < INFINITY;
    if (lv.A_l <= 0 || c < 0 || c >= (int64_t)a.K || !finite || !(g.z > g.x) || !(g.w > g.y)) {   // step 1: no candidates (uniform)
        if (tid < k) a.cand_idx[out0 + tid] = -1;
        return;
    }
    const rn::f32x4 *__restrict__ an = a.anchors + (int64_t)b * a.anchor_bstride4 + lv.base;
    const int Al = (int)lv.A_l;

    // the rectangle under the box: columns xs..xe and rows ys..ye of a W x H grid of `cells` anchors (unknown W: one row of Al cells of 1)
    const int cells = a.W[l] > 0 ? a.cells[l] : 1, W = a.W[l] > 0 ? a.W[l] : Al, H = Al / (W * cells);
    int xs = 0, xe = W - 1, ys = 0, ye = H - 1;
    if (a.W[l] > 0) {
        const rn::f32x4 a00 = an[0], a01 = an[W > 1 ? cells : 0], a10 = an[H > 1 ? W * cells : 0];
        const float cx0 = centre(a00.x, a00.z), cy0 = centre(a00.y, a00.w);
        span(cx0, centre(a01.x, a01.z) - cx0, g.x, g.z, W, xs, xe);
        span(cy0, centre(a10.y, a10.w) - cy0, g.y, g.w, H, ys, ye);
    }
    const int rowlen = (xe - xs + 1) * cells, total = (ye - ys + 1) * rowlen;          // (<= Al)

    if (tid == 0) { s_ctl[0] = 0; s_thr = ~0ull; }
    __syncthreads();
    for (int base = 0; base < total; base += TAL_STEP) {
        const u64 thr = s_thr;
        rn::f32x4 av[TAL_U];
        float x[TAL_U], d[TAL_U][4];
        int idx[TAL_U];
#pragma unroll
        for (int u = 0; u < TAL_U; ++u) {
            const int p0 = base + u * TAL_BLOCK + tid, p = p0 < total ? p0 : 0;
            const int y = p / rowlen, rem = p - y * rowlen;
            const int xc = rem / cells;
            const int i = ((ys + y) * W + xs + xc) * cells + (rem - xc * cells);
            idx[u] = p0 < total && i < Al ? i : -1;
            av[u] = rn::f32x4{0.f, 0.f, 0.f, 0.f};
            x[u] = 0.0f;
            d[u][0] = d[u][1] = d[u][2] = d[u][3] = 0.0f;
            if (idx[u] >= 0) {                          // the three loads of a visited anchor: one round trip
                const int64_t hr = (int64_t)b * lv.A_l + i;
                av[u] = an[i];
                x[u] = rn::dt<DT>::ld(lv.cls, hr * a.K + c);
                rn::box4<DT>::ld(lv.box, hr, d[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < TAL_U; ++u) {
            const float acx = centre(av[u].x, av[u].z), acy = centre(av[u].y, av[u].w);
            bool take = idx[u] >= 0 && acx > g.x && acx < g.z && acy > g.y && acy < g.w;      // step 1: strictly inside
            float m = 0.0f, iou = 0.0f;
            if (take) take = metric(a, g, av[u], x[u], d[u], m, iou);
            const u64 key = metric_key(m, (uint32_t)idx[u]);
            append(s_key, &s_ctl[0], take && key <= thr, key);
        }
        __syncthreads();
        const int n = s_ctl[0];
        __syncthreads();                                // everyone holds n before the next append moves the counter
        if (n > TAL_LIST_KEYS) rn_assign::shrink<TAL_BLOCK, TAL_PER>(s_key, s_hist, s_ctl, &s_thr, n, k, a.idx_bytes[l]);
    }
    int n = s_ctl[0];
    __syncthreads();
    if (n > k) {
        rn_assign::shrink<TAL_BLOCK, TAL_PER>(s_key, s_hist, s_ctl, &s_thr, n, k, a.idx_bytes[l]);
        n = k;
    }
    // the level's records (in no particular order: the merge ranks them); the IoU of a survivor is computed again from the same loads
    if (tid < k) {
        int32_t out = -1;
        float m = 0.0f, iou = 0.0f;
        if (tid < n) {
            const u64 key = s_key[tid];
            const uint32_t i = (uint32_t)key;
            const int64_t hr = (int64_t)b * lv.A_l + i;
            float d[4];
            rn::box4<DT>::ld(lv.box, hr, d);
            iou = rn::box_decode_iou(g, an[i], d, a.reg_w).iou;
            m = __uint_as_float(~(uint32_t)(key >> 32));
            out = (int32_t)(lv.base + i);
        }
        a.cand_idx[out0 + tid] = out;
        a.cand_iou[out0 + tid] = iou;
        a.cand_m[out0 + tid] = m;
    }
}

// steps 3-4 for one GT row per wave: the levels' records -> the row's topk, posted to the table
__global__ __launch_bounds__(RN_WAVE) void tal_merge_kernel(const int32_t *__restrict__ gt_off, const int B, const int64_t A, const int n,
                                                            const int topk, int32_t *__restrict__ cand_idx,
                                                            const float *__restrict__ cand_iou, const float *__restrict__ cand_m,
                                                            u64 *__restrict__ keys)
{
    __shared__ u64 s_key[RN_MAX_LEVELS * TAL_TOPK_MAX];
    const int lane = threadIdx.x;
    const int r = blockIdx.x;
    const int row = gt_off[0] + r;
    if (row >= gt_off[B]) return;
    const int b = image_of_row(gt_off, B, row);
    const uint32_t gi = (uint32_t)(row - gt_off[b]);
    int32_t *__restrict__ idx = cand_idx + (int64_t)r * n;
    for (int c = lane; c < n; c += RN_WAVE) {
        const int32_t i = idx[c];
        s_key[c] = i >= 0 ? metric_key(cand_m[(int64_t)r * n + c], (uint32_t)i) : ~0ull;   // (a record's key is never all ones: m > 0)
    }
    __syncthreads();
    for (int c = lane; c < n; c += RN_WAVE) {
        const u64 key = s_key[c];
        if (key == ~0ull) continue;
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += s_key[j] < key ? 1 : 0;                         // (every lane reads the same word: a broadcast)
        if (rank < topk) rn_assign::table_post(keys, (int64_t)b * A + (uint32_t)key, cand_iou[(int64_t)r * n + c], gi);
        else idx[c] = -1;
    }
}

size_t record_bytes(const int64_t total_gt, const int L, const int topk)
{
    return align16(sizeof(int32_t) * (size_t)total_gt * (size_t)L * (size_t)topk);
}

bool scalars_ok(const int L, const int topk, const int alpha, const int beta)
{
    return L > 0 && L <= RN_MAX_LEVELS && topk > 0 && alpha >= 0 && alpha <= TAL_EXP_MAX && beta >= 0 && beta <= TAL_EXP_MAX;
}

}  // namespace

RN_API int rn_tal_match_list_keys(void) { return TAL_LIST_KEYS; }

RN_API size_t rn_tal_match_workspace_bytes(int B, int64_t A, int64_t total_gt, int L, int topk)
{
    if (B <= 0 || A <= 0 || A > 0x7fffffff || total_gt < 0 || !scalars_ok(L, topk, 0, 0) || topk > TAL_TOPK_MAX) return 0;
    return align16(sizeof(u64) * (size_t)B * (size_t)A) + 3 * record_bytes(total_gt, L, topk);
}

RN_API int rn_tal_match(const void *const *cls_levels, const void *const *box_levels, const int64_t *level_anchors, const int32_t *cells,
                        const int32_t *level_w, int L, int dtype, int B, int K, const float *anchors, int64_t anchor_bstride,
                        const float *gt_boxes, const int64_t *gt_labels, const int32_t *gt_off, int topk, int alpha, int beta,
                        const float *reg_w, float logit_shift, int64_t *matches, int32_t *num_fg, uint64_t *special_rows,
                        int64_t total_gt, int flags, void *workspace, size_t workspace_bytes, void *stream)
{
    if (flags & ~(RN_MATCH_NUM_FG_ZEROED | RN_MATCH_FLAGGED_ONLY)) return RN_EINVAL;
    if ((flags & RN_MATCH_FLAGGED_ONLY) && !special_rows) return RN_EINVAL;
    if (!cls_levels || !box_levels || !level_anchors || !cells || !anchors || !gt_off || !matches || !workspace || !reg_w) return RN_EINVAL;
    if (B <= 0 || B > 65535 || K < 1 || total_gt < 0 || total_gt > 0x7fffffff || anchor_bstride < 0) return RN_EINVAL;
    if (total_gt > 0 && (!gt_boxes || !gt_labels)) return RN_EINVAL;
    if (dtype != RN_F32 && dtype != RN_BF16 && dtype != RN_F16) return RN_EINVAL;
    if (!scalars_ok(L, topk, alpha, beta) || !(fabsf(logit_shift) < INFINITY)) return RN_EINVAL;
    if (topk > TAL_TOPK_MAX) return RN_EUNSUPPORTED;
    for (int j = 0; j < 4; ++j)
        if (!(reg_w[j] > 0.0f) || !(reg_w[j] < INFINITY)) return RN_EINVAL;
    TalArgs a{};
    const size_t box_align = dtype == RN_F32 ? 16 : 8, cls_align = dtype == RN_F32 ? 4 : 2;
    int64_t A = 0;
    for (int l = 0; l < L; ++l) {
        const int64_t Al = level_anchors[l];
        if (Al < 0 || cells[l] <= 0) return RN_EINVAL;
        if (Al > 0 && (!cls_levels[l] || !box_levels[l])) return RN_EINVAL;
        if (!rn::aligned(cls_levels[l], cls_align) || !rn::aligned(box_levels[l], box_align)) return RN_EALIGN;
        const int w = level_w ? level_w[l] : 0;
        if (w < 0 || (w > 0 && Al % ((int64_t)w * cells[l]) != 0)) return RN_EINVAL;      // (a grid of w columns of `cells` anchors)
        a.lv[l] = rn::WalkLevel{cls_levels[l], box_levels[l], nullptr, A, Al};
        a.W[l] = Al > 0 ? w : 0;
        a.cells[l] = cells[l];
        int nb = 1;
        while (nb < 4 && ((Al - 1) >> (8 * nb)) > 0) ++nb;
        a.idx_bytes[l] = nb;
        A += Al;
    }
    if (A <= 0 || A > 0x7fffffff) return RN_EINVAL;
    if (anchor_bstride != 0 && anchor_bstride < A * 4) return RN_EINVAL;
    if (!rn::aligned(anchors, 16) || !rn::aligned(gt_boxes, 16) || !rn::aligned(gt_labels, 8) || (anchor_bstride & 3) ||
        !rn::aligned(workspace, 16) || !rn::aligned(special_rows, 8) || !rn::aligned(matches, 8) || !rn::aligned(gt_off, 4) ||
        !rn::aligned(num_fg, 4))
        return RN_EALIGN;
    const size_t key_bytes = align16(sizeof(u64) * (size_t)B * (size_t)A);
    const size_t rec_bytes = record_bytes(total_gt, L, topk);
    if (workspace_bytes < key_bytes + 3 * rec_bytes) return RN_EWORKSPACE;
    u64 *keys = (u64 *)workspace;
    a.cand_idx = (int32_t *)((char *)workspace + key_bytes);
    a.cand_iou = (float *)((char *)workspace + key_bytes + rec_bytes);
    a.cand_m = (float *)((char *)workspace + key_bytes + 2 * rec_bytes);
    a.L = L; a.B = B; a.K = K; a.topk = topk; a.alpha = alpha; a.beta = beta;
    a.A = A;
    a.anchors = (const rn::f32x4 *)anchors;
    a.anchor_bstride4 = anchor_bstride / 4;
    a.gt = (const rn::f32x4 *)gt_boxes;
    a.labels = gt_labels;
    a.gt_off = gt_off;
    for (int j = 0; j < 4; ++j) a.reg_w[j] = reg_w[j];
    a.logit_shift = logit_shift;
    u64 *special = (u64 *)special_rows;
    hipStream_t st = (hipStream_t)stream;
    const int prc = rn_assign::launch_prep(B, A, matches, num_fg, special, flags, st);
    if (prc != RN_OK) return prc;
    if (total_gt == 0) return RN_OK;                       // no GT rows anywhere: all background
    void (*sel)(const TalArgs) = dtype == RN_F32 ? tal_select_kernel<RN_F32> : (dtype == RN_BF16 ? tal_select_kernel<RN_BF16> : tal_select_kernel<RN_F16>);
    hipLaunchKernelGGL(sel, dim3((unsigned)total_gt, (unsigned)L), dim3(TAL_BLOCK), 0, st, a);
    RN_LAUNCH_CHECK();
    const int n = L * topk;
    hipLaunchKernelGGL(tal_merge_kernel, dim3((unsigned)total_gt), dim3(RN_WAVE), 0, st, gt_off, B, A, n, topk, a.cand_idx, a.cand_iou,
                       a.cand_m, keys);
    RN_LAUNCH_CHECK();
    return rn_assign::launch_emit(total_gt, n, gt_off, B, A, a.cand_idx, a.cand_iou, keys, matches, num_fg, special, st);
}
