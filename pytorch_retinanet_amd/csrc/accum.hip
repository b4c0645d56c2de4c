// Gradient accumulation for the master optimizers, capturable: the gradients of N micro-batches summed into fp32 accumulators, with
// the window position, the weight 1 / N and found_inf in a DEVICE block, so that one captured graph serves every micro-batch of a
// window and a new N needs no capture.
//
// optim.GradAccumulator owns the accumulators (one fp32 tensor per parameter, in the parameter's strides) and the block
// (rn_accum_state below; include/retinanet_hip.h documents the layout).  Per micro-batch:
//   rn_grad_accumulate   grad_accumulate_kernel, one launch per 160 tensors: the gradients are cut into chunks of RN_ACCUM_CHUNK
//                        elements and one workgroup takes one chunk (the chunking of csrc/clip.hip: the grid is the chunk count).
//                        Every gradient element is read once, in 16-byte loads (8 x 16-bit or 4 x fp32 per lane), widened to fp32
//                        and added in fp32, two roundings, no contraction (this file is built with -ffp-contract=off):
//                            acc = (pos == 0 ? 0.0f : acc) + (float(g) * w)
//                        At pos == 0 the accumulator is OVERWRITTEN, not read: no memset node, no zeroing pass, and the first
//                        micro-batch of a window moves 4 B per element less.  A lane that read a non-finite gradient element stores
//                        1.0f into the block's found_inf: a plain vector store of one value, idempotent, no atomic.
//   rn_grad_accum_advance  one single-wave launch AFTER the streaming kernel (the kernel boundary orders them): a micro step moves
//                        pos on by one; a final step counts the window, resets pos to 0 and clears found_inf for the next window.
// The streaming kernel only reads pos and w; nothing but the advance and the setter writes them.
#include <stddef.h>

#include "rn_multi.hpp"

namespace {

constexpr int ACC_MAX_TENSORS = 160;             // 160 x 24 B of tables + 16 B: inside the 4 KiB of kernel arguments

struct rn_accum_state {                          // RN_ACCUM_STATE doubles (include/retinanet_hip.h)
    float w;                                     // float(1.0 / n)
    int32_t n, pos;
    float found_inf;
    int64_t windows, nonfinite, micro;
    int64_t reserved[3];
};
static_assert(sizeof(rn_accum_state) == RN_ACCUM_STATE * sizeof(double), "rn_accum_state");
static_assert(offsetof(rn_accum_state, found_inf) == RN_ACCUM_FOUND_INF_OFFSET, "found_inf offset");

struct AccTable {
    float *acc[ACC_MAX_TENSORS];
    rn::ChunkMap<ACC_MAX_TENSORS> map;
    rn_accum_state *blk;
};
static_assert(sizeof(AccTable) <= 4096, "kernel arguments");

__device__ __forceinline__ bool nonfinite(const float f) { return !(fabsf(f) <= 3.402823466e38f); }

// VEC gradient elements (one 16-byte load) into VEC / 4 accumulator vectors
template <int VEC>
__device__ __forceinline__ bool acc_vec(const float (&g)[VEC], rn::f32x4 *__restrict__ a, const bool fresh, const float w)
{
    bool bad = false;
    rn::f32x4 av[VEC / 4];
#pragma unroll
    for (int k = 0; k < VEC / 4; ++k) av[k] = fresh ? rn::f32x4{0.0f, 0.0f, 0.0f, 0.0f} : a[k];
#pragma unroll
    for (int k = 0; k < VEC / 4; ++k) {
        av[k].x = av[k].x + g[4 * k] * w;
        av[k].y = av[k].y + g[4 * k + 1] * w;
        av[k].z = av[k].z + g[4 * k + 2] * w;
        av[k].w = av[k].w + g[4 * k + 3] * w;
        bad = bad || nonfinite(g[4 * k]) || nonfinite(g[4 * k + 1]) || nonfinite(g[4 * k + 2]) || nonfinite(g[4 * k + 3]);
    }
#pragma unroll
    for (int k = 0; k < VEC / 4; ++k) a[k] = av[k];
    return bad;
}

template <int DT16>
__global__ __launch_bounds__(256) void grad_accumulate_kernel(const AccTable t)
{
    const rn::ChunkLoc c = rn::locate(t.map, blockIdx.x);
    const float w = t.blk->w;
    const bool fresh = t.blk->pos == 0;
    const bool is16 = c.is16;
    const unsigned char *p = (const unsigned char *)t.map.grad[c.ti] + c.off * (is16 ? 2 : 4);
    float *__restrict__ a = t.acc[c.ti] + c.off;
    // (a 16-bit gradient's head of 4 elements is 16 bytes of the accumulator, which stays 16-byte aligned behind it)
    const rn::ChunkSplit sp(p, c.cnt, is16);
    const int nv = sp.nv;
    const rn::u32x4 *__restrict__ pv = sp.pv;
    rn::f32x4 *__restrict__ av = (rn::f32x4 *)(a + sp.head);
    bool bad = false;
    if (is16) {
        for (int v = threadIdx.x; v < nv; v += 512) {
            const bool two = v + 256 < nv;
            const rn::u32x4 q0 = pv[v], q1 = two ? pv[v + 256] : rn::u32x4{0u, 0u, 0u, 0u};
            float f[8];
            rn::dt<DT16>::unpack(q0, f);
            bad = acc_vec<8>(f, av + 2 * (int64_t)v, fresh, w) || bad;
            if (two) {
                rn::dt<DT16>::unpack(q1, f);
                bad = acc_vec<8>(f, av + 2 * (int64_t)(v + 256), fresh, w) || bad;
            }
        }
    } else {
        for (int v = threadIdx.x; v < nv; v += 512) {
            const bool two = v + 256 < nv;
            const rn::u32x4 q0 = pv[v], q1 = two ? pv[v + 256] : rn::u32x4{0u, 0u, 0u, 0u};
            float f[4];
            rn::dt<RN_F32>::unpack(q0, f);
            bad = acc_vec<4>(f, av + v, fresh, w) || bad;
            if (two) {
                rn::dt<RN_F32>::unpack(q1, f);
                bad = acc_vec<4>(f, av + v + 256, fresh, w) || bad;
            }
        }
    }
    const int e = sp.scalar_elem(threadIdx.x);
    if (e >= 0) {
        const float g = is16 ? rn::dt<DT16>::ld(p, e) : ((const float *)p)[e];
        const float old = fresh ? 0.0f : a[e];
        a[e] = old + g * w;
        bad = bad || nonfinite(g);
    }
    if (bad) t.blk->found_inf = 1.0f;                                     // (every writer stores the same value)
}

__global__ __launch_bounds__(64) void accum_advance_kernel(rn_accum_state *__restrict__ blk, const int final)
{
    if (threadIdx.x != 0) return;
    blk->micro += 1;
    if (final) {
        blk->windows += 1;
        if (blk->found_inf != 0.0f) blk->nonfinite += 1;
        blk->pos = 0;
        blk->found_inf = 0.0f;
    } else {
        blk->pos += 1;
    }
}

__global__ __launch_bounds__(64) void accum_set_kernel(rn_accum_state *__restrict__ blk, const int n, const float w)
{
    if (threadIdx.x == 0) { blk->n = n; blk->w = w; }
}

}  // namespace

RN_API int rn_grad_accum_set(void *block, int n, void *stream)
{
    if (!block || n < 1) return RN_EINVAL;
    if (!rn::aligned(block, 8)) return RN_EALIGN;
    hipLaunchKernelGGL(accum_set_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (rn_accum_state *)block, n, (float)(1.0 / (double)n));
    RN_LAUNCH_CHECK();
    return RN_OK;
}

RN_API int rn_grad_accum_advance(void *block, int final, void *stream)
{
    if (!block) return RN_EINVAL;
    if (!rn::aligned(block, 8)) return RN_EALIGN;
    hipLaunchKernelGGL(accum_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (rn_accum_state *)block, final != 0 ? 1 : 0);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

RN_API int rn_grad_accumulate(float *const *accs, const void *const *grads, void *const *params16, const int64_t *numels, int n_tensors,
                              int grads16, int dtype16, void *block, void *stream)
{
    if (dtype16 != RN_BF16 && dtype16 != RN_F16) return RN_EUNSUPPORTED;
    if (!accs || !grads || !numels || !block || n_tensors < 0) return RN_EINVAL;
    if (!rn::aligned(block, 8)) return RN_EALIGN;
    for (int i = 0; i < n_tensors; ++i) {                        // everything is checked before anything is launched
        if (!accs[i] || !grads[i] || numels[i] < 0) return RN_EINVAL;
        const bool is16 = grads16 && params16 && params16[i];
        if (!rn::aligned(accs[i], 16) || !rn::aligned(grads[i], is16 ? 8 : 16)) return RN_EALIGN;
    }
    hipStream_t st = (hipStream_t)stream;
    AccTable t;
    t.blk = (rn_accum_state *)block;
    return rn::for_chunk_maps(t.map, grads, params16, numels, n_tensors, grads16, [&](const int slot, const int i, const int64_t off) { t.acc[slot] = accs[i] + off; },
                              [&](const int64_t chunks) -> int {
        for (int i = t.map.cnt; i < ACC_MAX_TENSORS; ++i) t.acc[i] = nullptr;
        if (dtype16 == RN_F16) hipLaunchKernelGGL((grad_accumulate_kernel<RN_F16>), dim3((unsigned)chunks), dim3(256), 0, st, t);
        else hipLaunchKernelGGL((grad_accumulate_kernel<RN_BF16>), dim3((unsigned)chunks), dim3(256), 0, st, t);
        RN_LAUNCH_CHECK();
        return RN_OK;
    });
}
