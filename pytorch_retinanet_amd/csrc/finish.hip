// The last step of Retinanet.predict on the device (graph.CapturedPredict, Retinanet.predict_staged).
//
//   rn_detect_finish_var   transform.postprocess for the whole batch -- the detections of rn_detect_levels, which live on the resized
//                          images, mapped back to the original image sizes -- and everything the host has to read gathered into ONE
//                          result block, so a replayed predict ends in one device-to-host copy.
//
// Nothing about an image is a kernel argument: the original sizes come from in_hw_dev (rn_image_stage wrote them), the resized ones
// from out_hw_dev (rn_resize_plan_dev), the row counts from out_count.  One launch serves any B (no per-64-image table), nothing is
// synchronised, so the call can be captured.
//
// The block (rn_detect_result_bytes(B, max_det) bytes; every section starts on a 16-byte boundary, the padding is written as zero):
//   counts i32[B] | status i32[B] | pad | boxes f32[B][max_det][4] | scores f32[B][max_det] | pad | labels i64[B][max_det] | pad
//
// Row r < count[b] (count clamped to [0, max_det]: device data) is transform.resize_boxes(boxes, resized, original):
//   rh = float(orig_h) / float(res_h),  rw = float(orig_w) / float(res_w)        (fp32, correctly rounded: this file is built without
//   box = (x1 * rw, y1 * rh, x2 * rw, y2 * rh)                                    FMA contraction and with IEEE division)
// with score and label copied; a multiply by a ratio of exactly 1 leaves a value bit for bit as it was, which is resize_boxes'
// early return.  Rows r >= count[b] are written as zero, so the block is a pure function of the inputs.  counts and status are
// passed through as they are.  One thread per row; the threads of row 0 of an image write its two header words, thread 0 the padding.
#include "rn_common.hpp"

namespace {

constexpr int FIN_BLOCK = 256;

struct ResultLayout { size_t status, boxes, scores, labels, total; };

inline size_t up16(const size_t v) { return (v + 15) & ~(size_t)15; }

inline ResultLayout result_layout(const int B, const int max_det)
{
    const size_t rows = (size_t)B * (size_t)max_det;
    ResultLayout l;
    l.status = 4 * (size_t)B;
    l.boxes = up16(8 * (size_t)B);
    l.scores = l.boxes + 16 * rows;
    l.labels = up16(l.scores + 4 * rows);
    l.total = up16(l.labels + 8 * rows);
    return l;
}

__global__ __launch_bounds__(FIN_BLOCK) void detect_finish_var_kernel(
    const rn::f32x4 *__restrict__ boxes, const float *__restrict__ scores, const int64_t *__restrict__ labels,
    const int32_t *__restrict__ count, const int32_t *__restrict__ status, const int32_t *__restrict__ in_hw,
    const int32_t *__restrict__ out_hw, const int B, const int max_det, const int64_t rows, int32_t *__restrict__ r_count,
    int32_t *__restrict__ r_status, rn::f32x4 *__restrict__ r_boxes, float *__restrict__ r_scores, int64_t *__restrict__ r_labels,
    const int pad_head, const int pad_scores, const int pad_labels)
{
    const int64_t t = (int64_t)blockIdx.x * FIN_BLOCK + (int64_t)threadIdx.x;
    if (t == 0) {
        // (the sections end where the next 16-byte boundary is: 0 or 2 words after the header, 0..3 after the scores, 0 or 1 label)
        for (int i = 0; i < pad_head; ++i) r_status[B + i] = 0;
        for (int i = 0; i < pad_scores; ++i) r_scores[rows + i] = 0.0f;
        for (int i = 0; i < pad_labels; ++i) r_labels[rows + i] = 0;
    }
    if (t >= rows) return;
    const int b = (int)(t / max_det), r = (int)(t - (int64_t)b * max_det);
    const int32_t raw = count[b];
    if (r == 0) {
        r_count[b] = raw;
        r_status[b] = status[b];
    }
    const int32_t n = raw < 0 ? 0 : (raw > max_det ? max_det : raw);          // (device data: never more rows than the image has)
    if (r < n) {
        const float rh = (float)in_hw[2 * b] / (float)out_hw[2 * b], rw = (float)in_hw[2 * b + 1] / (float)out_hw[2 * b + 1];
        const rn::f32x4 v = boxes[t];
        r_boxes[t] = rn::f32x4{v.x * rw, v.y * rh, v.z * rw, v.w * rh};
        r_scores[t] = scores[t];
        r_labels[t] = labels[t];
    } else {
        r_boxes[t] = rn::f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        r_scores[t] = 0.0f;
        r_labels[t] = 0;
    }
}

}  // namespace

RN_API size_t rn_detect_result_bytes(int B, int max_det)
{
    if (B <= 0 || max_det <= 0) return 0;
    return result_layout(B, max_det).total;
}

RN_API int rn_detect_finish_var(const float *out_boxes, const float *out_scores, const int64_t *out_labels, const int32_t *out_count,
                                const int32_t *out_status, const int32_t *in_hw_dev, const int32_t *out_hw_dev, int B, int max_det,
                                void *result, size_t result_bytes, void *stream)
{
    if (!out_boxes || !out_scores || !out_labels || !out_count || !out_status || !in_hw_dev || !out_hw_dev || !result || B <= 0 || max_det <= 0)
        return RN_EINVAL;
    if (!rn::aligned(out_boxes, 16) || !rn::aligned(out_scores, 4) || !rn::aligned(out_labels, 8) || !rn::aligned(out_count, 4) ||
        !rn::aligned(out_status, 4) || !rn::aligned(in_hw_dev, 4) || !rn::aligned(out_hw_dev, 4) || !rn::aligned(result, 16))
        return RN_EALIGN;
    const ResultLayout l = result_layout(B, max_det);
    if (result_bytes < l.total) return RN_EWORKSPACE;
    const int64_t rows = (int64_t)B * (int64_t)max_det;
    const int64_t blocks = (rows + FIN_BLOCK - 1) / FIN_BLOCK;
    if (blocks > 0x7fffffffll) return RN_EUNSUPPORTED;
    char *base = (char *)result;
    hipLaunchKernelGGL(detect_finish_var_kernel, dim3((unsigned)blocks), dim3(FIN_BLOCK), 0, (hipStream_t)stream,
                       (const rn::f32x4 *)out_boxes, out_scores, out_labels, out_count, out_status, in_hw_dev, out_hw_dev, B, max_det, rows,
                       (int32_t *)base, (int32_t *)(base + l.status), (rn::f32x4 *)(base + l.boxes), (float *)(base + l.scores),
                       (int64_t *)(base + l.labels), (int)((l.boxes - 8 * (size_t)B) / 4), (int)((l.labels - l.scores - 4 * (size_t)rows) / 4),
                       (int)((l.total - l.labels - 8 * (size_t)rows) / 8));
    RN_LAUNCH_CHECK();
    return RN_OK;
}
