// Ragged ground truth into fixed-size device buffers (graph.CapturedTrainStep's GT capacity mode).
//
// A captured train step reads its GT from static buffers: gt_boxes [R][4], gt_labels [R], gt_off [B+1], num_fg [B].  With a
// capacity class per entry (R = B x class) one graph serves every batch whose per-image box counts fit; what changes from batch
// to batch is written here, outside the graph, by ONE launch per 64 images:
//   rn_gt_stage         gathers the per-image boxes / labels (the user's tensors, pointers and counts passed BY VALUE in the kernel
//                       argument table, like rn_copy_many), writes gt_off as the prefix of those counts and clears num_fg --
//                       no host->device copy from pageable memory, no memset node, no synchronisation;
//   rn_gt_scale_packed  the transform's per-image box resize (transform.resize_boxes: fp32 multiply by the fp32 ratio) on a packed
//                       buffer, out of place: inside a graph only the device knows which row belongs to which image (gt_off).
//   rn_gt_flip_scale_many / rn_gt_flip_scale_packed
//                       the same resize after the train-time horizontal flip (augment.RandomHorizontalFlip): for an image whose
//                       device flag is set, x1' = W - x2, x2' = W - x1 in fp32 (the reference's coco_transforms formula, W = the
//                       original width), then the ratio multiply.  The _many form reads the user's per-image tensors (pointers
//                       and counts by value, like rn_gt_stage) and packs them into a fresh buffer; the _packed form is
//                       rn_gt_scale_packed plus widths and flags.  The flags are device data written by rn_hflip_draw inside the
//                       same captured step, so the decision never reaches the host.
//   rn_gt_flip_scale_many_dev / rn_gt_flip_scale_packed_dev
//                       the same two kernels with the ratios read from DEVICE memory (f32[2B] = (rh, rw), written by rn_short_side_draw
//                       inside the same captured step: augment.RandomShortSide) and the flags optional (null: nothing flips).  The
//                       arithmetic on a row is flip_scale either way: bit-identical to the host-ratio forms given the same values.
//   rn_gt_flip_scale_packed_var
//                       the _packed_dev kernel with the original widths read from DEVICE memory too (i32[B][2] = (h, w), written by
//                       rn_image_stage: graph.CapturedTrainStep's image capacity mode) instead of the host ``widths`` array; the
//                       width becomes a float exactly as the host's float(w) does, so the rows are bit-identical again.
// All kernels index their argument tables by blockIdx only (a per-lane index into the argument segment becomes a vector load of
// the table; CHANGELOG, the compiler's treatment of hand-written loops, item 2).
#include "rn_common.hpp"

namespace {

constexpr int GT_MAX = 64;          // images per launch
constexpr int GT_BLOCK = 256;
constexpr int GT_GRID_X = 64;       // row blocks per image at most (a grid-stride loop covers the rest)

struct StageTable {
    const rn::f32x4 *boxes[GT_MAX];
    const int64_t *labels[GT_MAX];
    int32_t count[GT_MAX];
    int32_t off[GT_MAX];
};

__global__ __launch_bounds__(GT_BLOCK) void gt_stage_kernel(const StageTable t, rn::f32x4 *__restrict__ gt_boxes,
                                                           int64_t *__restrict__ gt_labels, int32_t *__restrict__ gt_off,
                                                           int32_t *__restrict__ num_fg, int base, int last, int32_t end)
{
    const int i = blockIdx.y;
    const rn::f32x4 *__restrict__ sb = t.boxes[i];
    const int64_t *__restrict__ sl = t.labels[i];
    const int32_t n = t.count[i], o = t.off[i];
    // exactly n rows of each source: a one-box label tensor is 8 bytes, so labels go one int64 per lane (no 16-byte pairs)
    for (int32_t r = (int32_t)blockIdx.x * GT_BLOCK + (int32_t)threadIdx.x; r < n; r += (int32_t)gridDim.x * GT_BLOCK) {
        gt_boxes[o + r] = sb[r];
        gt_labels[o + r] = sl[r];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        gt_off[base + i] = o;
        num_fg[base + i] = 0;
        if (last && i == (int)gridDim.y - 1) gt_off[base + i + 1] = end;
    }
}

struct ScaleTable { float rh[GT_MAX]; float rw[GT_MAX]; };

__global__ __launch_bounds__(GT_BLOCK) void gt_scale_kernel(const ScaleTable t, const rn::f32x4 *__restrict__ in, rn::f32x4 *__restrict__ out,
                                                           const int32_t *__restrict__ gt_off, int base, int32_t rows)
{
    const int i = blockIdx.y;
    const float rh = t.rh[i], rw = t.rw[i];
    int32_t lo = gt_off[base + i], hi = gt_off[base + i + 1];
    // (gt_off is device data: the row range is clamped to the buffer, whatever it holds)
    lo = lo < 0 ? 0 : (lo > rows ? rows : lo);
    hi = hi < lo ? lo : (hi > rows ? rows : hi);
    for (int32_t r = lo + (int32_t)blockIdx.x * GT_BLOCK + (int32_t)threadIdx.x; r < hi; r += (int32_t)gridDim.x * GT_BLOCK) {
        const rn::f32x4 b = in[r];
        out[r] = rn::f32x4{b.x * rw, b.y * rh, b.z * rw, b.w * rh};
    }
}

__device__ __forceinline__ rn::f32x4 flip_scale(const rn::f32x4 b, const bool flip, const float w, const float rh, const float rw)
{
    const float x1 = flip ? w - b.z : b.x, x2 = flip ? w - b.x : b.z;
    return rn::f32x4{x1 * rw, b.y * rh, x2 * rw, b.w * rh};
}

struct FlipManyTable {
    const rn::f32x4 *boxes[GT_MAX];
    int32_t count[GT_MAX];
    int32_t off[GT_MAX];
    float w[GT_MAX], rh[GT_MAX], rw[GT_MAX];
};

// DEV: rh / rw of image base + i from ``ratios`` (device) instead of the table, and ``flags`` may be null
template <bool DEV>
__global__ __launch_bounds__(GT_BLOCK) void gt_flip_scale_many_kernel(const FlipManyTable t, const uint8_t *__restrict__ flags,
                                                                     const float *__restrict__ ratios, rn::f32x4 *__restrict__ out, int base)
{
    const int i = blockIdx.y;
    const rn::f32x4 *__restrict__ sb = t.boxes[i];
    const int32_t n = t.count[i], o = t.off[i];
    const float w = t.w[i], rh = DEV ? ratios[2 * (base + i)] : t.rh[i], rw = DEV ? ratios[2 * (base + i) + 1] : t.rw[i];
    const bool flip = DEV ? (flags != nullptr && flags[base + i] != 0) : flags[base + i] != 0;
    for (int32_t r = (int32_t)blockIdx.x * GT_BLOCK + (int32_t)threadIdx.x; r < n; r += (int32_t)gridDim.x * GT_BLOCK)
        out[o + r] = flip_scale(sb[r], flip, w, rh, rw);
}

struct FlipScaleTable { float w[GT_MAX]; float rh[GT_MAX]; float rw[GT_MAX]; };

// VAR (implies DEV): the width of image base + i from ``in_hw`` (device, (h, w) pairs) instead of the table
template <bool DEV, bool VAR>
__global__ __launch_bounds__(GT_BLOCK) void gt_flip_scale_kernel(const FlipScaleTable t, const uint8_t *__restrict__ flags,
                                                                const float *__restrict__ ratios, const int32_t *__restrict__ in_hw,
                                                                const rn::f32x4 *__restrict__ in, rn::f32x4 *__restrict__ out,
                                                                const int32_t *__restrict__ gt_off, int base, int32_t rows)
{
    const int i = blockIdx.y;
    const float w = VAR ? (float)in_hw[2 * (base + i) + 1] : t.w[i];
    const float rh = DEV ? ratios[2 * (base + i)] : t.rh[i], rw = DEV ? ratios[2 * (base + i) + 1] : t.rw[i];
    const bool flip = DEV ? (flags != nullptr && flags[base + i] != 0) : flags[base + i] != 0;
    int32_t lo = gt_off[base + i], hi = gt_off[base + i + 1];
    lo = lo < 0 ? 0 : (lo > rows ? rows : lo);
    hi = hi < lo ? lo : (hi > rows ? rows : hi);
    for (int32_t r = lo + (int32_t)blockIdx.x * GT_BLOCK + (int32_t)threadIdx.x; r < hi; r += (int32_t)gridDim.x * GT_BLOCK)
        out[r] = flip_scale(in[r], flip, w, rh, rw);
}

int grid_x(int64_t rows_per_image)
{
    int64_t bx = (rows_per_image + GT_BLOCK - 1) / GT_BLOCK;
    return (int)(bx < 1 ? 1 : (bx > GT_GRID_X ? GT_GRID_X : bx));
}

}  // namespace

RN_API int rn_gt_stage(const void *const *boxes, const void *const *labels, const int64_t *counts, int B, float *gt_boxes,
                       int64_t *gt_labels, int64_t rows, int32_t *gt_off, int32_t *num_fg, void *stream)
{
    if (!boxes || !labels || !counts || B <= 0 || rows < 0 || !gt_off || !num_fg) return RN_EINVAL;
    if (rows > 0 && (!gt_boxes || !gt_labels)) return RN_EINVAL;
    if (!rn::aligned(gt_off, 4) || !rn::aligned(num_fg, 4) || (gt_boxes && !rn::aligned(gt_boxes, 16)) || (gt_labels && !rn::aligned(gt_labels, 8)))
        return RN_EALIGN;
    // every argument is checked before anything is launched: a rejected call leaves the buffers as they were
    int64_t total = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t c = counts[b];
        if (c < 0) return RN_EINVAL;
        if (c > 0) {
            if (!boxes[b] || !labels[b]) return RN_EINVAL;
            if (!rn::aligned(boxes[b], 16) || !rn::aligned(labels[b], 8)) return RN_EALIGN;
        }
        total += c;
        if (total > rows) return RN_EINVAL;
    }
    if (total > INT32_MAX) return RN_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    int64_t off = 0;
    for (int base = 0; base < B; base += GT_MAX) {
        const int cnt = (B - base) < GT_MAX ? (B - base) : GT_MAX;
        StageTable t;
        int64_t most = 0;
        for (int i = 0; i < GT_MAX; ++i) {
            const bool on = i < cnt;
            const int64_t c = on ? counts[base + i] : 0;
            t.boxes[i] = on && c ? (const rn::f32x4 *)boxes[base + i] : nullptr;
            t.labels[i] = on && c ? (const int64_t *)labels[base + i] : nullptr;
            t.count[i] = (int32_t)c;
            t.off[i] = (int32_t)off;
            off += c;
            if (c > most) most = c;
        }
        const int last = base + cnt == B;
        hipLaunchKernelGGL(gt_stage_kernel, dim3((unsigned)grid_x(most), (unsigned)cnt), dim3(GT_BLOCK), 0, st, t, (rn::f32x4 *)gt_boxes,
                           gt_labels, gt_off, num_fg, base, last, (int32_t)total);
        RN_LAUNCH_CHECK();
    }
    return RN_OK;
}

RN_API int rn_gt_scale_packed(const float *gt_boxes, float *out_boxes, const int32_t *gt_off, const float *ratios, int B, int64_t rows,
                              int64_t max_per_image, void *stream)
{
    if (!gt_off || !ratios || B <= 0 || rows < 0 || rows > INT32_MAX || max_per_image < 0) return RN_EINVAL;
    if (rows > 0 && (!gt_boxes || !out_boxes)) return RN_EINVAL;
    if (rows > 0 && gt_boxes == out_boxes) return RN_EINVAL;           // out of place: a replayed graph would compound an in-place scale
    if (!rn::aligned(gt_off, 4) || (gt_boxes && !rn::aligned(gt_boxes, 16)) || (out_boxes && !rn::aligned(out_boxes, 16))) return RN_EALIGN;
    if (rows == 0) return RN_OK;
    hipStream_t st = (hipStream_t)stream;
    for (int base = 0; base < B; base += GT_MAX) {
        const int cnt = (B - base) < GT_MAX ? (B - base) : GT_MAX;
        ScaleTable t;
        for (int i = 0; i < GT_MAX; ++i) {
            t.rh[i] = i < cnt ? ratios[2 * (base + i)] : 1.0f;
            t.rw[i] = i < cnt ? ratios[2 * (base + i) + 1] : 1.0f;
        }
        hipLaunchKernelGGL(gt_scale_kernel, dim3((unsigned)grid_x(max_per_image), (unsigned)cnt), dim3(GT_BLOCK), 0, st, t,
                           (const rn::f32x4 *)gt_boxes, (rn::f32x4 *)out_boxes, gt_off, base, (int32_t)rows);
        RN_LAUNCH_CHECK();
    }
    return RN_OK;
}

namespace {

// ratios: HOST float[2B], or null with ratios_dev (DEVICE float[2B]) in their place; flags may be null only with ratios_dev
int flip_scale_many(const void *const *boxes, const int64_t *counts, int B, const float *widths, const float *ratios, const float *ratios_dev,
                    const uint8_t *flags, float *out_boxes, int64_t rows, void *stream)
{
    if (!boxes || !counts || !widths || (!ratios == !ratios_dev) || (!flags && !ratios_dev) || B <= 0 || rows < 0) return RN_EINVAL;
    if (rows > 0 && !out_boxes) return RN_EINVAL;
    if ((out_boxes && !rn::aligned(out_boxes, 16)) || (ratios_dev && !rn::aligned(ratios_dev, 4))) return RN_EALIGN;
    int64_t total = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t c = counts[b];
        if (c < 0) return RN_EINVAL;
        if (c > 0) {
            if (!boxes[b]) return RN_EINVAL;
            if (!rn::aligned(boxes[b], 16)) return RN_EALIGN;
        }
        total += c;
        if (total > rows) return RN_EINVAL;
    }
    if (total > INT32_MAX) return RN_EINVAL;
    if (total == 0) return RN_OK;
    hipStream_t st = (hipStream_t)stream;
    int64_t off = 0;
    for (int base = 0; base < B; base += GT_MAX) {
        const int cnt = (B - base) < GT_MAX ? (B - base) : GT_MAX;
        FlipManyTable t;
        int64_t most = 0;
        for (int i = 0; i < GT_MAX; ++i) {
            const bool on = i < cnt;
            const int64_t c = on ? counts[base + i] : 0;
            t.boxes[i] = on && c ? (const rn::f32x4 *)boxes[base + i] : nullptr;
            t.count[i] = (int32_t)c;
            t.off[i] = (int32_t)off;
            t.w[i] = on ? widths[base + i] : 0.0f;
            t.rh[i] = on && ratios ? ratios[2 * (base + i)] : 1.0f;
            t.rw[i] = on && ratios ? ratios[2 * (base + i) + 1] : 1.0f;
            off += c;
            if (c > most) most = c;
        }
        const dim3 grid((unsigned)grid_x(most), (unsigned)cnt);
        if (ratios_dev)
            hipLaunchKernelGGL(gt_flip_scale_many_kernel<true>, grid, dim3(GT_BLOCK), 0, st, t, flags, ratios_dev, (rn::f32x4 *)out_boxes, base);
        else
            hipLaunchKernelGGL(gt_flip_scale_many_kernel<false>, grid, dim3(GT_BLOCK), 0, st, t, flags, ratios_dev, (rn::f32x4 *)out_boxes, base);
        RN_LAUNCH_CHECK();
    }
    return RN_OK;
}

// widths: HOST float[B], or null with in_hw_dev (DEVICE i32[B][2]) in their place -- only together with ratios_dev
int flip_scale_packed(const float *gt_boxes, float *out_boxes, const int32_t *gt_off, const float *widths, const int32_t *in_hw_dev,
                      const float *ratios, const float *ratios_dev, const uint8_t *flags, int B, int64_t rows, int64_t max_per_image,
                      void *stream)
{
    if (!gt_off || (!widths == !in_hw_dev) || (in_hw_dev && !ratios_dev) || (!ratios == !ratios_dev) || (!flags && !ratios_dev) || B <= 0 || rows < 0 || rows > INT32_MAX || max_per_image < 0)
        return RN_EINVAL;
    if (rows > 0 && (!gt_boxes || !out_boxes)) return RN_EINVAL;
    if (rows > 0 && gt_boxes == out_boxes) return RN_EINVAL;
    if (!rn::aligned(gt_off, 4) || (gt_boxes && !rn::aligned(gt_boxes, 16)) || (out_boxes && !rn::aligned(out_boxes, 16)) ||
        (ratios_dev && !rn::aligned(ratios_dev, 4)) || (in_hw_dev && !rn::aligned(in_hw_dev, 4)))
        return RN_EALIGN;
    if (rows == 0) return RN_OK;
    hipStream_t st = (hipStream_t)stream;
    for (int base = 0; base < B; base += GT_MAX) {
        const int cnt = (B - base) < GT_MAX ? (B - base) : GT_MAX;
        FlipScaleTable t;
        for (int i = 0; i < GT_MAX; ++i) {
            t.w[i] = i < cnt && widths ? widths[base + i] : 0.0f;
            t.rh[i] = i < cnt && ratios ? ratios[2 * (base + i)] : 1.0f;
            t.rw[i] = i < cnt && ratios ? ratios[2 * (base + i) + 1] : 1.0f;
        }
        const dim3 grid((unsigned)grid_x(max_per_image), (unsigned)cnt);
        if (in_hw_dev)
            hipLaunchKernelGGL((gt_flip_scale_kernel<true, true>), grid, dim3(GT_BLOCK), 0, st, t, flags, ratios_dev, in_hw_dev,
                               (const rn::f32x4 *)gt_boxes, (rn::f32x4 *)out_boxes, gt_off, base, (int32_t)rows);
        else if (ratios_dev)
            hipLaunchKernelGGL((gt_flip_scale_kernel<true, false>), grid, dim3(GT_BLOCK), 0, st, t, flags, ratios_dev, in_hw_dev,
                               (const rn::f32x4 *)gt_boxes, (rn::f32x4 *)out_boxes, gt_off, base, (int32_t)rows);
        else
            hipLaunchKernelGGL((gt_flip_scale_kernel<false, false>), grid, dim3(GT_BLOCK), 0, st, t, flags, ratios_dev, in_hw_dev,
                               (const rn::f32x4 *)gt_boxes, (rn::f32x4 *)out_boxes, gt_off, base, (int32_t)rows);
        RN_LAUNCH_CHECK();
    }
    return RN_OK;
}

}  // namespace

RN_API int rn_gt_flip_scale_many(const void *const *boxes, const int64_t *counts, int B, const float *widths, const float *ratios,
                                 const uint8_t *flags, float *out_boxes, int64_t rows, void *stream)
{
    if (!ratios || !flags) return RN_EINVAL;
    return flip_scale_many(boxes, counts, B, widths, ratios, nullptr, flags, out_boxes, rows, stream);
}

RN_API int rn_gt_flip_scale_packed(const float *gt_boxes, float *out_boxes, const int32_t *gt_off, const float *widths, const float *ratios,
                                   const uint8_t *flags, int B, int64_t rows, int64_t max_per_image, void *stream)
{
    if (!ratios || !flags) return RN_EINVAL;
    return flip_scale_packed(gt_boxes, out_boxes, gt_off, widths, nullptr, ratios, nullptr, flags, B, rows, max_per_image, stream);
}

RN_API int rn_gt_flip_scale_many_dev(const void *const *boxes, const int64_t *counts, int B, const float *widths, const float *ratios_dev,
                                     const uint8_t *flags_or_null, float *out_boxes, int64_t rows, void *stream)
{
    if (!ratios_dev) return RN_EINVAL;
    return flip_scale_many(boxes, counts, B, widths, nullptr, ratios_dev, flags_or_null, out_boxes, rows, stream);
}

RN_API int rn_gt_flip_scale_packed_dev(const float *gt_boxes, float *out_boxes, const int32_t *gt_off, const float *widths,
                                       const float *ratios_dev, const uint8_t *flags_or_null, int B, int64_t rows, int64_t max_per_image,
                                       void *stream)
{
    if (!ratios_dev) return RN_EINVAL;
    return flip_scale_packed(gt_boxes, out_boxes, gt_off, widths, nullptr, nullptr, ratios_dev, flags_or_null, B, rows, max_per_image, stream);
}

RN_API int rn_gt_flip_scale_packed_var(const float *gt_boxes, float *out_boxes, const int32_t *gt_off, const int32_t *in_hw_dev,
                                       const float *ratios_dev, const uint8_t *flags_or_null, int B, int64_t rows, int64_t max_per_image,
                                       void *stream)
{
    if (!in_hw_dev || !ratios_dev) return RN_EINVAL;
    return flip_scale_packed(gt_boxes, out_boxes, gt_off, nullptr, in_hw_dev, nullptr, ratios_dev, flags_or_null, B, rows, max_per_image, stream);
}
