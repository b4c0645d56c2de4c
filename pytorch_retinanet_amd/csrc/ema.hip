// An exponential moving average of the fp32 master weights for the master optimizers, capturable: the factor of the next update, the
// update count and the decay schedule in a DEVICE block, so one captured step serves every update (the first, which copies, and the
// warm-up ramp included) and a new decay needs no capture.
//
// optim.WeightEMA owns the averages (one fp32 tensor per parameter, in the master's strides) and the block (rn_ema_state below;
// include/retinanet_hip.h documents the layout).  Per optimizer step:
//   rn_ema_update    ema_update_kernel, one launch per 160 tensors: the tensors are cut into chunks of RN_CLIP_CHUNK elements and one
//                    workgroup takes one chunk (the chunked map of rn_multi.hpp: the grid is the chunk count).  Everything is fp32 and
//                    16-byte aligned, so every chunk is whole 16-byte vectors plus at most 3 elements; per element, three roundings,
//                    no contraction (this file is built with -ffp-contract=off):
//                        ema = updates == 0 ? w : ema + (w - ema) * om
//                    At updates == 0 the average is OVERWRITTEN, not read (the pos == 0 trick of accum.hip): nothing initialises it.
//                    With found_inf non-null and *found_inf != 0 (the loss scaler skipped the step) nothing is written.
//   rn_ema_advance   one single-wave launch AFTER the streaming kernel (the kernel boundary orders them): a skipped step is counted,
//                    any other moves `updates` on by one and recomputes om for the next update.
// The streaming kernel only reads om, updates and found_inf; nothing but the advance and the setter writes the block.
//   rn_ema_swap      ema_swap_kernel, one launch per 120 tensors (three pointer tables): ema <-> master, and the 16-bit working copy
//                    refreshed from the new master.  Twice is the identity.
// All stores are plain vector stores; no atomics.
#include <stddef.h>

#include "rn_multi.hpp"

namespace {

constexpr int EMA_MAX_TENSORS = 160;             // 160 x 24 B of tables + 24 B: inside the 4 KiB of kernel arguments
constexpr int SWAP_MAX_TENSORS = 120;            // 120 x 32 B of tables + 8 B

struct rn_ema_state {                            // RN_EMA_STATE doubles (include/retinanet_hip.h)
    double decay, warmup;
    int64_t updates, skipped;
    float om;                                    // float(1.0 - d_t) for t = updates: the factor the next update uses
    float reserved_f;
    int64_t reserved[3];
};
static_assert(sizeof(rn_ema_state) == RN_EMA_STATE * sizeof(double), "rn_ema_state");
static_assert(offsetof(rn_ema_state, updates) == 16 && offsetof(rn_ema_state, skipped) == 24, "counter offsets");
static_assert(offsetof(rn_ema_state, om) == RN_EMA_OM_OFFSET, "om offset");

struct EmaTable {
    float *ema[EMA_MAX_TENSORS];
    rn::ChunkMap<EMA_MAX_TENSORS> map;           // (map.grad: the masters, all fp32)
    const rn_ema_state *blk;
    const float *found_inf;
};
static_assert(sizeof(EmaTable) <= 4096, "kernel arguments");

struct SwapTable {
    float *ema[SWAP_MAX_TENSORS];
    uint16_t *p16[SWAP_MAX_TENSORS];
    rn::ChunkMap<SWAP_MAX_TENSORS> map;          // (map.grad: the masters, written here: the table's pointer type is the map's)
};
static_assert(sizeof(SwapTable) <= 4096, "kernel arguments");

// all in double: d_t = warmup > 0 ? min(decay, (1 + t) / (warmup + t)) : decay;  om = float(1 - d_t)
__device__ __forceinline__ float one_minus_decay(const double decay, const double warmup, const int64_t t)
{
    double d = decay;
    if (warmup > 0.0) {
        const double ramp = (1.0 + (double)t) / (warmup + (double)t);
        d = ramp < decay ? ramp : decay;
    }
    return (float)(1.0 - d);
}

__global__ __launch_bounds__(256) void ema_update_kernel(const EmaTable t)
{
    if (t.found_inf && *t.found_inf != 0.0f) return;             // (GradScaler: the optimizer moved nothing, so the average stays)
    const rn::ChunkLoc c = rn::locate(t.map, blockIdx.x);
    const float om = t.blk->om;
    const bool fresh = t.blk->updates == 0;
    const float *__restrict__ w = (const float *)t.map.grad[c.ti] + c.off;
    float *__restrict__ e = t.ema[c.ti] + c.off;
    // (both 16-byte aligned: the host checks the tensors, and c.off is a multiple of the chunk)
    const int nv = c.cnt >> 2;
    const rn::f32x4 *__restrict__ wv = (const rn::f32x4 *)w;
    rn::f32x4 *__restrict__ ev = (rn::f32x4 *)e;
    for (int v = threadIdx.x; v < nv; v += 512) {
        const bool two = v + 256 < nv;
        const rn::f32x4 w0 = wv[v], w1 = two ? wv[v + 256] : rn::f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (fresh) {
            ev[v] = w0;
            if (two) ev[v + 256] = w1;
        } else {
            const rn::f32x4 e0 = ev[v], e1 = two ? ev[v + 256] : rn::f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            ev[v] = e0 + (w0 - e0) * om;
            if (two) ev[v + 256] = e1 + (w1 - e1) * om;
        }
    }
    const int i = 4 * nv + (int)threadIdx.x;                     // the < 4 elements behind the last whole vector
    if (i < c.cnt) {
        const float wi = w[i];
        if (fresh) {
            e[i] = wi;
        } else {
            const float ei = e[i];
            e[i] = ei + (wi - ei) * om;
        }
    }
}

template <int DT>
__global__ __launch_bounds__(256) void ema_swap_kernel(const SwapTable t)
{
    const rn::ChunkLoc c = rn::locate(t.map, blockIdx.x);
    float *__restrict__ w = (float *)t.map.grad[c.ti] + c.off;
    float *__restrict__ e = t.ema[c.ti] + c.off;
    uint16_t *__restrict__ p16 = t.p16[c.ti] ? t.p16[c.ti] + c.off : nullptr;      // (8-byte aligned: c.off is a multiple of the chunk)
    const int nv = c.cnt >> 2;
    rn::f32x4 *__restrict__ wv = (rn::f32x4 *)w;
    rn::f32x4 *__restrict__ ev = (rn::f32x4 *)e;
    for (int v = threadIdx.x; v < nv; v += 256) {
        const rn::f32x4 a = ev[v], b = wv[v];
        ev[v] = b;
        wv[v] = a;
        if (p16) {
            const float f[4] = {a.x, a.y, a.z, a.w};
            rn::store16x4<DT>(p16, v, f);
        }
    }
    const int i = 4 * nv + (int)threadIdx.x;
    if (i < c.cnt) {
        const float a = e[i], b = w[i];
        e[i] = b;
        w[i] = a;
        if (p16) p16[i] = (uint16_t)(rn::dt<DT>::pk(a, 0.0f) & 0xffffu);          // (the low half of the step kernels' pk)
    }
}

__global__ __launch_bounds__(64) void ema_advance_kernel(rn_ema_state *__restrict__ blk, const float *__restrict__ found_inf)
{
    if (threadIdx.x != 0) return;
    if (found_inf && *found_inf != 0.0f) {
        blk->skipped += 1;
        return;
    }
    const int64_t t = blk->updates + 1;
    blk->updates = t;
    blk->om = one_minus_decay(blk->decay, blk->warmup, t);
}

__global__ __launch_bounds__(64) void ema_set_kernel(rn_ema_state *__restrict__ blk, const double decay, const double warmup, const int64_t updates)
{
    if (threadIdx.x != 0) return;
    blk->decay = decay;
    blk->warmup = warmup;
    if (updates >= 0) blk->updates = updates;
    blk->om = one_minus_decay(decay, warmup, blk->updates);
}

}  // namespace

RN_API int rn_ema_set(void *block, double decay, double warmup, int64_t updates, void *stream)
{
    if (!block || !(decay >= 0.0 && decay < 1.0) || !(warmup >= 0.0) || updates < -1) return RN_EINVAL;
    if (!rn::aligned(block, 8)) return RN_EALIGN;
    hipLaunchKernelGGL(ema_set_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (rn_ema_state *)block, decay, warmup, updates);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

RN_API int rn_ema_advance(void *block, const float *found_inf, void *stream)
{
    if (!block) return RN_EINVAL;
    if (!rn::aligned(block, 8) || !rn::aligned(found_inf, 4)) return RN_EALIGN;
    hipLaunchKernelGGL(ema_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (rn_ema_state *)block, found_inf);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

RN_API int rn_ema_update(float *const *emas, const float *const *masters, const int64_t *numels, int n_tensors, const void *block,
                         const float *found_inf, void *stream)
{
    if (!emas || !masters || !numels || !block || n_tensors < 0) return RN_EINVAL;
    if (!rn::aligned(block, 8) || !rn::aligned(found_inf, 4)) return RN_EALIGN;
    for (int i = 0; i < n_tensors; ++i) {                        // everything is checked before anything is launched
        if (!emas[i] || !masters[i] || numels[i] < 0) return RN_EINVAL;
        if (!rn::aligned(emas[i], 16) || !rn::aligned(masters[i], 16)) return RN_EALIGN;
    }
    hipStream_t st = (hipStream_t)stream;
    EmaTable t;
    t.blk = (const rn_ema_state *)block;
    t.found_inf = found_inf;
    return rn::for_chunk_maps(t.map, (const void *const *)masters, nullptr, numels, n_tensors, 0,
                              [&](const int slot, const int i, const int64_t off) { t.ema[slot] = emas[i] + off; },
                              [&](const int64_t chunks) -> int {
        for (int i = t.map.cnt; i < EMA_MAX_TENSORS; ++i) t.ema[i] = nullptr;
        hipLaunchKernelGGL(ema_update_kernel, dim3((unsigned)chunks), dim3(256), 0, st, t);
        RN_LAUNCH_CHECK();
        return RN_OK;
    });
}

RN_API int rn_ema_swap(float *const *emas, float *const *masters, void *const *params16, const int64_t *numels, int n_tensors, int dtype16,
                       void *stream)
{
    if (dtype16 != RN_BF16 && dtype16 != RN_F16) return RN_EUNSUPPORTED;
    if (!emas || !masters || !numels || n_tensors < 0) return RN_EINVAL;
    for (int i = 0; i < n_tensors; ++i) {                        // everything is checked before anything is launched
        if (!emas[i] || !masters[i] || numels[i] < 0) return RN_EINVAL;
        if (!rn::aligned(emas[i], 16) || !rn::aligned(masters[i], 16) || (params16 && !rn::aligned(params16[i], 8))) return RN_EALIGN;
    }
    hipStream_t st = (hipStream_t)stream;
    SwapTable t;
    return rn::for_chunk_maps(t.map, (const void *const *)masters, nullptr, numels, n_tensors, 0,
                              [&](const int slot, const int i, const int64_t off) {
        t.ema[slot] = emas[i] + off;
        t.p16[slot] = params16 && params16[i] ? (uint16_t *)params16[i] + off : nullptr;
    },
                              [&](const int64_t chunks) -> int {
        for (int i = t.map.cnt; i < SWAP_MAX_TENSORS; ++i) { t.ema[i] = nullptr; t.p16[i] = nullptr; }
        if (dtype16 == RN_F16) hipLaunchKernelGGL((ema_swap_kernel<RN_F16>), dim3((unsigned)chunks), dim3(256), 0, st, t);
        else hipLaunchKernelGGL((ema_swap_kernel<RN_BF16>), dim3((unsigned)chunks), dim3(256), 0, st, t);
        RN_LAUNCH_CHECK();
        return RN_OK;
    });
}
