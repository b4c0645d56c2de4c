// The walk over the matcher's flagged rows that the sparse losses behind K3 (loss.hip) share: boxloss.hip (GIoU / DIoU) and qfl.hip
// (Quality Focal Loss).  ONE copy of the strip loop, the compaction, the level search, the sums and the host-side checks; a user
// supplies what it does with one listed row (`Op::row`) and its own scalars.
//
// Shape: one wave owns a strip of 64 flag words (4 096 rows) of ONE image per pass, one word per lane.  The set bits of the strip are
// compacted into a per-wave LDS list, and the list is worked off 64 rows at a time, one row per lane, so a row's chain of dependent
// loads (match -> GT row -> ...) runs once per 64 listed rows, not once per flag word.  Latency-bound: a few thousand rows -- about
// 0.3 % of all rows at the train shape -- each a chain of dependent loads; no bandwidth figure applies.  WHERE a row's loads are issued
// is the user's choice (WalkArgs::match / gt_row / anchor are called by `Op::row` when it wants them).
//
// Sum: every workgroup writes ONE double into its own slot of the workspace (always, zero included: no slot needs clearing), and a
// one-wave kernel behind it adds the slots in a fixed order.  No atomics, so two calls give the same bits.
#pragma once
#include "rn_common.hpp"

#include <math.h>

namespace rn {

constexpr int WALK_WAVES = 4;                     // waves per workgroup: one strip each per pass
constexpr int WALK_BLOCK = WALK_WAVES * RN_WAVE;
constexpr int WALK_WORDS = RN_WAVE;               // flag words per strip (one per lane)
constexpr int WALK_ROWS = WALK_WORDS * 64;        // rows per strip: 4 096, the capacity of a wave's list (offsets fit 16 bits)
constexpr int WALK_MAX_BLOCKS = 128;              // grid cap: 512 strips = 2 097 152 rows per pass (the train shape, B = 8, A = 201 600, is 400 strips)

// One level of head outputs: the class and box outputs a user reads (cls: null for a user without class outputs) and the gradient
// tensor it writes (null: value only), with the level's first anchor and its anchor count.
struct WalkLevel { const void *cls, *box; void *grad; int64_t base, A_l; };

// One listed row as `Op::row` gets it.  `lv` is the row's level entry and `r` its row inside the level's tensors.
struct WalkRow {
    int b, t0, T;                    // the image, its first GT row and its GT count
    float scale;                     // 1 / (max(num_fg[b], 1) B)
    int64_t ag;                      // anchor index inside the image
    bool ok;                         // the lane holds a row (the list may end inside the 64; bits past A in the last word are not rows)
    WalkLevel lv;
    int64_t r;
};

struct WalkArgs {
    WalkLevel lv[RN_MAX_LEVELS];
    int32_t L, B;
    int64_t A, W;                    // anchors per image, flag words per image
    const f32x4 *anchors;
    int64_t anchor_bstride4;         // anchors (of four floats) between images; 0 = shared
    const f32x4 *gt_boxes;
    const int64_t *gt_labels;        // (null for a user without class outputs)
    const int32_t *gt_off;
    const int64_t *matches;
    const unsigned long long *special;
    const int32_t *num_fg;
    float reg_w[4];
    float inv_B;
    const float *gscale;             // nullable
    double *partials;                // [gridDim.x]
    int32_t strips_per_image, total_strips;

    // The loads of a row with `ok` set, for `Op::row` to issue where it wants them.
    __device__ __forceinline__ int64_t match(const WalkRow &row) const { return matches[(int64_t)row.b * A + row.ag]; }   // (read through the flag words only)
    __device__ __forceinline__ f32x4 anchor(const WalkRow &row) const { return anchors[(int64_t)row.b * anchor_bstride4 + row.ag]; }
    // The GT row of a match index >= 0, clamped into the image's rows (a stale index past them reads the image's last row).
    __device__ __forceinline__ int64_t gt_row(const WalkRow &row, const int64_t pm) const {
        return (int64_t)row.t0 + (pm < (int64_t)row.T ? pm : (int64_t)(row.T - 1));
    }
};

// The walk of one lane: `fn(row, acc)` once per lane and 64 listed rows (wave-uniformly: every lane is called, `row.ok` says whether
// it holds a row); returns the lane's sum over its strips.
template <class F>
__device__ __forceinline__ double walk_matched_rows(const WalkArgs &a, F fn)
{
    __shared__ unsigned short s_rows[WALK_WAVES][WALK_ROWS];  // flagged rows of the wave's strip (offsets from its first anchor)
    const int lane = threadIdx.x & (RN_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned long long below = (1ull << lane) - 1ull;
    double acc = 0.0;
#pragma unroll 1
    for (int strip = (int)blockIdx.x * WALK_WAVES + wave; strip < a.total_strips; strip += (int)gridDim.x * WALK_WAVES) {
        WalkRow row;
        row.b = strip / a.strips_per_image;
        const int64_t w0 = (int64_t)(strip - row.b * a.strips_per_image) * WALK_WORDS;
        row.t0 = a.gt_off[row.b]; row.T = a.gt_off[row.b + 1] - row.t0;
        unsigned long long word = 0ull;
        if (row.T > 0 && w0 + lane < a.W) word = a.special[(int64_t)row.b * a.W + w0 + lane];   // (an image without GT has no matched row)
        unsigned long long nz = __ballot(word != 0ull);
        if (!nz) continue;
        const int nf = a.num_fg[row.b];
        row.scale = (1.0f / (float)(nf > 1 ? nf : 1)) * a.inv_B;
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
            row.ag = w0 * 64 + (have ? (int64_t)s_rows[wave][i0 + lane] : 0);
            row.ok = have && row.ag < a.A;                                              // (bits past A in the last word, if any, are not rows)
            row.lv = a.lv[0];
            row.lv.base = 0; row.lv.A_l = 1;
#pragma unroll 1
            for (int l = 0; l < a.L; ++l) {                                             // (l is wave-uniform: the level table stays in scalar registers)
                const bool in = row.ag >= a.lv[l].base && row.ag < a.lv[l].base + a.lv[l].A_l;
                if (in) row.lv = a.lv[l];
            }
            row.r = (int64_t)row.b * row.lv.A_l + (row.ag - row.lv.base);              // row inside the level tensor
            fn(row, acc);
        }
        // the list is rewritten by the next strip: every lane has read its entries before any lane writes
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    return acc;
}

// The lanes' sums -> the workgroup's slot: the fixed butterfly per wave, then the waves in order.
__device__ __forceinline__ void walk_block_sum(const double acc, double *__restrict__ partials)
{
    __shared__ double s_part[WALK_WAVES];
    const double accw = wave_sum_d(acc);
    if ((threadIdx.x & (RN_WAVE - 1)) == 0) s_part[threadIdx.x >> 6] = accw;
    __syncthreads();
    if (threadIdx.x == 0) {
        double c = 0.0;
#pragma unroll
        for (int w = 0; w < WALK_WAVES; ++w) c += s_part[w];
        partials[blockIdx.x] = c;                                                       // every workgroup, every call: no stale slot
    }
}

// The main kernel of a user `Op`: a struct that holds the WalkArgs as `w`, the user's own scalars, and
// `template <int DT, bool WRITE_GRAD> __device__ void row(const WalkRow &, float gs, double &acc) const`.
template <class Op, int DT, bool WRITE_GRAD>
__global__ __launch_bounds__(WALK_BLOCK) void matched_rows_kernel(const Op op)
{
    const float gs = op.w.gscale ? *op.w.gscale : 1.0f;
    const double acc = walk_matched_rows(op.w, [&](const WalkRow &row, double &sum) { op.template row<DT, WRITE_GRAD>(row, gs, sum); });
    walk_block_sum(acc, op.w.partials);
}

// One wave: lane i adds slots i, i + 64, ... in order, then the fixed butterfly.  ADD: the total goes ONTO out_loss[SLOT] (K3's
// value); otherwise `weight` times the total replaces it.  One conversion from the double either way.
template <int SLOT, bool ADD>
__global__ __launch_bounds__(RN_WAVE) void matched_rows_sum_kernel(const double *__restrict__ partials, const int n, const float weight,
                                                                  float *__restrict__ out_loss)
{
    double s = 0.0;
    for (int i = (int)threadIdx.x; i < n; i += RN_WAVE) s += partials[i];
    s = wave_sum_d(s);
    if (threadIdx.x == 0) out_loss[SLOT] = (float)(ADD ? (double)out_loss[SLOT] + s : (double)weight * s);
}

static inline int walk_grid_blocks(const int B, const int64_t A, int &strips_per_image, int &total_strips)
{
    const int64_t W = (A + 63) / 64;
    const int64_t spi = (W + WALK_WORDS - 1) / WALK_WORDS, total = spi * B;
    if (total > 0x7fffffff) return 0;
    strips_per_image = (int)spi; total_strips = (int)total;
    const int64_t blocks = (total + WALK_WAVES - 1) / WALK_WAVES;
    return (int)(blocks < WALK_MAX_BLOCKS ? blocks : WALK_MAX_BLOCKS);
}

static inline size_t walk_workspace_bytes(const int B, const int64_t A)
{
    if (B <= 0 || A <= 0) return 0;
    int spi = 0, total = 0;
    return (size_t)walk_grid_blocks(B, A, spi, total) * sizeof(double);
}

// What the entry points check in common, in the order their return codes have, and the WalkArgs filled from it; `blocks` is the
// main kernel's grid.  `cls_levels` / `gt_labels`: null for a user without class outputs (one that has them checks `cls_levels`
// itself first); `grad_levels` (nullable) are then the class outputs' gradients, otherwise the box outputs'.  A user's own scalar
// checks (all RN_EINVAL) go in front of this call.
static inline int walk_fill(WalkArgs &a, int &blocks, const void *const *cls_levels, const void *const *box_levels,
                            const int64_t *level_anchors, const int L, const int dtype, const int B, const float *anchors,
                            const int64_t anchor_bstride, const float *gt_boxes, const int64_t *gt_labels, const int32_t *gt_off,
                            const int64_t *matches, const uint64_t *special_rows, const int32_t *num_fg, const float *reg_w,
                            const float *grad_prescale, const float *out_loss, void *const *grad_levels, void *workspace,
                            const size_t workspace_bytes)
{
    if (!box_levels || !level_anchors || !anchors || !gt_off || !matches || !special_rows || !num_fg || !reg_w || !out_loss || !workspace)
        return RN_EINVAL;
    if (L <= 0 || L > RN_MAX_LEVELS || B <= 0 || anchor_bstride < 0 || (anchor_bstride & 3)) return RN_EINVAL;
    if (dtype != RN_F32 && dtype != RN_BF16 && dtype != RN_F16) return RN_EINVAL;
    for (int j = 0; j < 4; ++j)
        if (!(reg_w[j] > 0.0f) || !(reg_w[j] < INFINITY)) return RN_EINVAL;
    const size_t box_align = dtype == RN_F32 ? 16 : 8, cls_align = dtype == RN_F32 ? 4 : 2;
    const size_t grad_align = cls_levels ? cls_align : box_align;
    a = WalkArgs{};
    int64_t A = 0;
    for (int l = 0; l < L; ++l) {
        const void *cls = cls_levels ? cls_levels[l] : nullptr;
        if (level_anchors[l] < 0) return RN_EINVAL;
        if (level_anchors[l] > 0 && ((cls_levels && !cls) || !box_levels[l] || (grad_levels && !grad_levels[l]))) return RN_EINVAL;
        if (!aligned(box_levels[l], box_align) || !aligned(cls, cls_align) || (grad_levels && !aligned(grad_levels[l], grad_align)))
            return RN_EALIGN;
        a.lv[l] = WalkLevel{cls, box_levels[l], grad_levels ? grad_levels[l] : nullptr, A, level_anchors[l]};
        A += level_anchors[l];
    }
    if (A <= 0) return RN_EINVAL;
    if (anchor_bstride != 0 && anchor_bstride < A * 4) return RN_EINVAL;
    if (!aligned(anchors, 16) || !aligned(gt_boxes, 16) || !aligned(gt_labels, 8) || !aligned(matches, 8) || !aligned(special_rows, 8) ||
        !aligned(gt_off, 4) || !aligned(num_fg, 4) || !aligned(out_loss, 4) || !aligned(grad_prescale, 4) || !aligned(workspace, 16))
        return RN_EALIGN;
    int spi = 0, total = 0;
    blocks = walk_grid_blocks(B, A, spi, total);
    if (blocks <= 0) return RN_EINVAL;
    if (workspace_bytes < (size_t)blocks * sizeof(double)) return RN_EWORKSPACE;
    a.L = L; a.B = B;
    a.A = A; a.W = (A + 63) / 64;
    a.anchors = (const f32x4 *)anchors;
    a.anchor_bstride4 = anchor_bstride / 4;
    a.gt_boxes = (const f32x4 *)gt_boxes;           // (may be null, as gt_labels, when no image has GT: then no flag word is read)
    a.gt_labels = gt_labels;
    a.gt_off = gt_off;
    a.matches = matches;
    a.special = (const unsigned long long *)special_rows;
    a.num_fg = num_fg;
    for (int j = 0; j < 4; ++j) a.reg_w[j] = reg_w[j];
    a.inv_B = 1.0f / (float)B;
    a.gscale = grad_prescale;
    a.partials = (double *)workspace;
    a.strips_per_image = spi; a.total_strips = total;
    return RN_OK;
}

// The two launches of a call: the main kernel of `op`, then the sum kernel onto / into out_loss[SLOT].
template <int SLOT, bool ADD, class Op>
static inline int walk_launch(const Op &op, const int blocks, const int dtype, const bool write_grad, const float weight, float *out_loss,
                              hipStream_t s)
{
    void (*k)(const Op) = nullptr;
    if (dtype == RN_F32) k = write_grad ? matched_rows_kernel<Op, RN_F32, true> : matched_rows_kernel<Op, RN_F32, false>;
    else if (dtype == RN_BF16) k = write_grad ? matched_rows_kernel<Op, RN_BF16, true> : matched_rows_kernel<Op, RN_BF16, false>;
    else k = write_grad ? matched_rows_kernel<Op, RN_F16, true> : matched_rows_kernel<Op, RN_F16, false>;
    k<<<blocks, WALK_BLOCK, 0, s>>>(op);
    RN_LAUNCH_CHECK();
    matched_rows_sum_kernel<SLOT, ADD><<<1, RN_WAVE, 0, s>>>(op.w.partials, blocks, weight, out_loss);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

}  // namespace rn
