// Global-norm gradient clipping for the master optimizers, capturable: the L2 norm of every gradient of a step and the clip
// coefficient of torch.nn.utils.clip_grad_norm_, left in a DEVICE block that rn_sgd_master_step / rn_adam_master_step read.
//
// optim.GradClip owns the block (rn_clip_state below; include/retinanet_hip.h documents the layout) and a scratch buffer of one
// float per chunk.  Per call:
//   pass 1  grad_sqsum_kernel, one launch per 224 tensors: the gradients are cut into chunks of RN_CLIP_CHUNK elements and one
//           workgroup takes one chunk, so a 2.4 M-element conv gradient is 144 workgroups and a BatchNorm vector is one -- the grid
//           is the chunk count, not (largest tensor) x (tensor count).  Every element is read once, in 16-byte loads (8 x 16-bit or
//           4 x fp32 per lane, four loads in flight per lane), widened to double and squared-and-added by one fp64 fma into four
//           accumulators per lane, then summed across the wave (__shfl_xor butterfly, wave64), across the four waves through LDS,
//           and the workgroup's sum is STORED, as a double, to the chunk's own slot of the scratch buffer.  No atomics: every partial
//           and the order they are added in are fixed by the tensor sizes, so the norm is bit-identical from call to call.
//           Why double all the way (the kernel stays bound by its loads: one cvt + one fp64 fma per element): with fp32 lane sums the
//           sum of squares carried ~1e-8 of relative error on small gradient sets, enough to round the fp32 norm the wrong way when
//           the exact value lies near the middle of two fp32 numbers (measured: 0.52 ulp off where torch's own norm was 0.48 off,
//           and a coefficient one ulp from torch's for that step); in double the fp32 norm is the correctly rounded one.
//   pass 2  clip_finalize_kernel, one workgroup: the slots of this call in double (lane l adds slots l, l + 256, ... in order, then
//           a fixed tree), total = float(sqrt(sum)) * (1 / grad_scale), and torch's coefficient in fp32, in torch's operations:
//           coef = min((1 / (total + 1e-6)) * max_norm, 1)      (max_norm / tensor is reciprocal-then-multiply in torch)
//           A non-finite norm gives what torch gives (0 or NaN); under a GradScaler found_inf skips that step anyway.
// The chunk -> (tensor, offset) map is a table of first-chunk indices in the kernel arguments; a workgroup finds its tensor by a
// binary search of it (8 uniform steps): rn_multi.hpp.  No memset and no memcpy node on this path (graph.py).
#include <stddef.h>

#include "rn_multi.hpp"

namespace {

constexpr int CLIP_MAX_TENSORS = 224;            // 224 x 16 B of tables + 16 B: inside the 4 KiB of kernel arguments

struct rn_clip_state {                           // RN_CLIP_STATE doubles (include/retinanet_hip.h)
    float max_norm, total_norm, clip_coef, reserved;
    int64_t calls, clipped, nonfinite, reserved2;
    double reserved3[2];
};
static_assert(sizeof(rn_clip_state) == RN_CLIP_STATE * sizeof(double), "rn_clip_state");
static_assert(offsetof(rn_clip_state, clip_coef) == RN_CLIP_COEF_OFFSET, "clip_coef offset");

struct ClipTable {
    rn::ChunkMap<CLIP_MAX_TENSORS> map;
    double *partial;                             // slot of this launch's chunk 0
};
static_assert(sizeof(ClipTable) <= 4096, "kernel arguments");

template <int DT16>
__device__ __forceinline__ double sq_sum(const rn::u32x4 q, const bool is16, double acc)
{
    if (is16) {
        float f[8];
        rn::dt<DT16>::unpack(q, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) { const double d = (double)f[j]; acc = fma(d, d, acc); }
    } else {
        float f[4];
        rn::dt<RN_F32>::unpack(q, f);
#pragma unroll
        for (int j = 0; j < 4; ++j) { const double d = (double)f[j]; acc = fma(d, d, acc); }
    }
    return acc;
}

template <int DT16>
__global__ __launch_bounds__(256) void grad_sqsum_kernel(const ClipTable t)
{
    __shared__ double wave_part[4];
    const rn::ChunkLoc c = rn::locate(t.map, blockIdx.x);
    const unsigned char *p = (const unsigned char *)t.map.grad[c.ti] + c.off * (c.is16 ? 2 : 4);
    const rn::ChunkSplit sp(p, c.cnt, c.is16);
    const bool is16 = c.is16;
    const int nv = sp.nv;
    const rn::u32x4 *__restrict__ pv = sp.pv;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int v = threadIdx.x; v < nv; v += 1024) {
        rn::u32x4 q[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = (v + 256 * j < nv) ? pv[v + 256 * j] : rn::u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = sq_sum<DT16>(q[j], is16, acc[j]);
    }
    const int e = sp.scalar_elem(threadIdx.x);
    if (e >= 0) {
        const double d = (double)(is16 ? rn::dt<DT16>::ld(p, e) : ((const float *)p)[e]);
        acc[0] = fma(d, d, acc[0]);
    }
    const double s = rn::wave_sum_d((acc[0] + acc[1]) + (acc[2] + acc[3]));
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) t.partial[blockIdx.x] = (wave_part[0] + wave_part[1]) + (wave_part[2] + wave_part[3]);
}

__global__ __launch_bounds__(256) void clip_finalize_kernel(const double *__restrict__ partial, const int64_t n_slots,
                                                            const float *__restrict__ grad_scale, rn_clip_state *__restrict__ blk)
{
    __shared__ double wave_part[4];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n_slots; i += 256) s += partial[i];
    s = rn::wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double sum = (wave_part[0] + wave_part[1]) + (wave_part[2] + wave_part[3]);
    float total = (float)sqrt(sum);
    if (grad_scale) total = total * (1.0f / *grad_scale);       // the step kernels' inv_scale: the norm of the unscaled gradients
    float coef = (1.0f / (total + 1e-6f)) * blk->max_norm;       // torch: max_norm / (total_norm + 1e-6) = reciprocal * max_norm
    coef = coef > 1.0f ? 1.0f : coef;                            // torch.clamp(max = 1): NaN stays NaN
    blk->total_norm = total;
    blk->clip_coef = coef;
    blk->calls += 1;
    if (coef < 1.0f) blk->clipped += 1;
    if (!(fabsf(total) <= 3.402823466e38f)) blk->nonfinite += 1;
}

__global__ __launch_bounds__(64) void clip_set_kernel(rn_clip_state *__restrict__ blk, const float max_norm)
{
    if (threadIdx.x == 0) blk->max_norm = max_norm;
}

}  // namespace

RN_API int rn_grad_clip_set(void *block, float max_norm, void *stream)
{
    if (!block || !(max_norm > 0.0f)) return RN_EINVAL;
    if (!rn::aligned(block, 8)) return RN_EALIGN;
    hipLaunchKernelGGL(clip_set_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (rn_clip_state *)block, max_norm);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

RN_API int rn_grad_norm_clip(const void *const *grads, void *const *params16, const int64_t *numels, int n_tensors, int grads16, int dtype16,
                             const float *grad_scale, double *scratch, int64_t scratch_slots, void *block, void *stream)
{
    if (dtype16 != RN_BF16 && dtype16 != RN_F16) return RN_EUNSUPPORTED;
    if (!grads || !numels || !scratch || !block || n_tensors < 0 || scratch_slots < 0) return RN_EINVAL;
    if (!rn::aligned(block, 8) || !rn::aligned(scratch, 8)) return RN_EALIGN;
    int64_t slots = 0;
    for (int i = 0; i < n_tensors; ++i) {                        // everything is checked before anything is launched
        if (!grads[i] || numels[i] < 0) return RN_EINVAL;
        const bool is16 = grads16 && params16 && params16[i];
        if (!rn::aligned(grads[i], is16 ? 8 : 16)) return RN_EALIGN;
        slots += (numels[i] + rn::CHUNK - 1) / rn::CHUNK;
    }
    if (slots > scratch_slots) return RN_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    ClipTable t;
    int64_t done = 0;                                            // slots of the launches so far
    const int rc = rn::for_chunk_maps(t.map, grads, params16, numels, n_tensors, grads16, [](int, int, int64_t) {}, [&](const int64_t chunks) -> int {
        t.partial = scratch + done;
        if (dtype16 == RN_F16) hipLaunchKernelGGL((grad_sqsum_kernel<RN_F16>), dim3((unsigned)chunks), dim3(256), 0, st, t);
        else hipLaunchKernelGGL((grad_sqsum_kernel<RN_BF16>), dim3((unsigned)chunks), dim3(256), 0, st, t);
        RN_LAUNCH_CHECK();
        done += chunks;
        return RN_OK;
    });
    if (rc != RN_OK) return rc;
    hipLaunchKernelGGL(clip_finalize_kernel, dim3(1), dim3(256), 0, st, (const double *)scratch, done, grad_scale, (rn_clip_state *)block);
    RN_LAUNCH_CHECK();
    return RN_OK;
}
