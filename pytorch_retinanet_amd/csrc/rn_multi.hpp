// The multi-tensor pieces the optimizer-side files share (internal; no kernels here):
//   the chunked map    clip.hip, accum.hip: gradients cut into chunks of rn::CHUNK elements, one workgroup per chunk, the
//                      chunk -> (tensor, offset) map a table of first-chunk indices in the kernel arguments
//   the step pieces    optim.hip, adam.hip: the gradient loads, unscale-then-clip, the 16-bit store and the grid of the
//                      4-elements-per-thread step kernels, and the host-side check of a step call's tensors
#pragma once
#include "rn_common.hpp"

namespace rn {

// ---- the chunked map --------------------------------------------------------------------------------------------------------
static_assert(RN_CLIP_CHUNK == RN_ACCUM_CHUNK, "clip.hip and accum.hip share one chunking");
constexpr int CHUNK = RN_CLIP_CHUNK;
constexpr int64_t CHUNK_PIECE = (int64_t)1 << 30;   // a tensor above 2^30 elements enters the table in pieces (a multiple of the chunk)
constexpr uint32_t CHUNK_IS16 = 0x80000000u;
static_assert(CHUNK_PIECE % CHUNK == 0 && CHUNK % 8 == 0, "chunking");

template <int MAX>
struct ChunkMap {                                   // embedded in the kernel-argument struct of its user
    const void *grad[MAX];
    uint32_t n[MAX];                                // elements (<= 2^30)
    uint32_t first[MAX];                            // index of the tensor's first chunk in this launch | CHUNK_IS16 for a 16-bit gradient
    int cnt;
};

struct ChunkLoc {
    int ti;                                         // table slot
    int64_t off;                                    // first element of the chunk in that tensor
    int cnt;                                        // elements of the chunk (>= 1: the host counts ceil(n / chunk) chunks per tensor)
    bool is16;
};

// the last tensor whose first chunk is <= `chunk` (a binary search, uniform over the workgroup)
template <int MAX>
__device__ __forceinline__ ChunkLoc locate(const ChunkMap<MAX> &m, const uint32_t chunk)
{
    int lo = 0, hi = m.cnt - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((m.first[mid] & ~CHUNK_IS16) <= chunk) lo = mid;
        else hi = mid - 1;
    }
    const uint32_t first = m.first[lo];
    ChunkLoc c;
    c.ti = lo;
    c.is16 = (first & CHUNK_IS16) != 0;
    c.off = (int64_t)(chunk - (first & ~CHUNK_IS16)) * CHUNK;
    const int64_t left = (int64_t)m.n[lo] - c.off;
    c.cnt = left < CHUNK ? (int)left : CHUNK;
    return c;
}

// A chunk starting at `p`: `head` elements in front of the first 16-byte boundary (a 16-bit gradient may start 8-byte aligned: 4 of
// them), then `nv` whole 16-byte vectors of `vec` elements at `pv`, then the < 8 / < 4 leftover elements from `tail0` on.
struct ChunkSplit {
    int head, nv, vec, tail0, n_tail;
    const u32x4 *pv;
    __device__ __forceinline__ ChunkSplit(const unsigned char *p, const int cnt, const bool is16)
    {
        const int esz = is16 ? 2 : 4;
        vec = is16 ? 8 : 4;
        head = (int)(((16 - ((uintptr_t)p & 15)) & 15) / esz);
        head = head < cnt ? head : cnt;
        nv = (cnt - head) / vec;
        pv = (const u32x4 *)(p + (int64_t)head * esz);
        tail0 = head + nv * vec;
        n_tail = cnt - tail0;
    }
    // scalar paths: lanes 0 .. head - 1 take the head, the next lanes the tail (at most 7 + 7 elements); -1: nothing for this lane
    __device__ __forceinline__ int scalar_elem(const int lane) const
    {
        if (lane < head) return lane;
        if (lane - head < n_tail) return tail0 + lane - head;
        return -1;
    }
};

// Host: enter the tensors into `m` (gradient i is 16-bit when grads16 and params16 and params16[i]), a tensor above CHUNK_PIECE in
// pieces, and call `launch(chunks)` -- the grid of the table just filled, its unused slots zeroed -- whenever the table is full or
// would pass 2^31 chunks, and for the rest.  `place(slot, i, off)` sets the user's own per-slot fields for elements off.. of tensor i.
template <int MAX, class Place, class Launch>
inline int for_chunk_maps(ChunkMap<MAX> &m, const void *const *grads, void *const *params16, const int64_t *numels, const int n_tensors,
                          const int grads16, Place place, Launch launch)
{
    int64_t chunks = 0;                                          // chunks in the table
    m.cnt = 0;
    auto flush = [&]() -> int {
        if (m.cnt == 0) return RN_OK;
        for (int i = m.cnt; i < MAX; ++i) { m.grad[i] = nullptr; m.n[i] = 0; m.first[i] = 0; }
        const int rc = launch(chunks);
        chunks = 0;
        m.cnt = 0;
        return rc;
    };
    for (int i = 0; i < n_tensors; ++i) {
        const bool is16 = grads16 && params16 && params16[i];
        for (int64_t off = 0; off < numels[i]; off += CHUNK_PIECE) {
            const int64_t n = numels[i] - off < CHUNK_PIECE ? numels[i] - off : CHUNK_PIECE;
            const int64_t c = (n + CHUNK - 1) / CHUNK;
            if (m.cnt == MAX || chunks + c > 0x7fffffff) {
                const int rc = flush();
                if (rc != RN_OK) return rc;
            }
            m.grad[m.cnt] = (const unsigned char *)grads[i] + off * (is16 ? 2 : 4);
            m.n[m.cnt] = (uint32_t)n;
            m.first[m.cnt] = (uint32_t)chunks | (is16 ? CHUNK_IS16 : 0u);
            place(m.cnt, i, off);
            ++m.cnt;
            chunks += c;
        }
    }
    return flush();
}

// ---- the step pieces ----------------------------------------------------------------------------------------------------------
// gradient elements 4 v .. 4 v + 3 of tensor ti: one 8-byte load of 16-bit values (DT) or one 16-byte load of fp32.  (`grads` is the
// table in the kernel arguments: each branch reads its own entry, as the kernels did before these lines were shared.)
template <int DT, class Table>
__device__ __forceinline__ f32x4 load_grad4(const Table &t, const int ti, const int64_t v, const bool g16)
{
    if (g16) {
        const u32x2 gv = ((const u32x2 *)t.grad[ti])[v];
        return f32x4{mma<DT>::lo(gv.x), mma<DT>::hi(gv.x), mma<DT>::lo(gv.y), mma<DT>::hi(gv.y)};
    }
    return ((const f32x4 *)t.grad[ti])[v];
}

template <int DT, class Table>
__device__ __forceinline__ float load_grad1(const Table &t, const int ti, const int64_t i, const bool g16)
{
    return g16 ? mma<DT>::lo((uint32_t)((const uint16_t *)t.grad[ti])[i]) : ((const float *)t.grad[ti])[i];
}

// unscale, then clip: two separate fp32 products, each only when its pointer is non-null, before weight decay
__device__ __forceinline__ float unscale_clip(const float g, const float *grad_scale, const float inv_scale, const float *clip_coef, const float coef)
{
    float r = grad_scale ? g * inv_scale : g;
    if (clip_coef) r = r * coef;
    return r;
}

template <int DT>
__device__ __forceinline__ void store16x4(uint16_t *p16, const int64_t v, const float (&w)[4])
{
    u32x2 o;
    o.x = dt<DT>::pk(w[0], w[1]); o.y = dt<DT>::pk(w[2], w[3]);
    ((u32x2 *)p16)[v] = o;
}

constexpr int STEP_BLOCKS_X = 1024;

// one pass over the largest of the launch's `cnt` tensors at 4 elements per thread, capped; one grid row per tensor
inline dim3 step_grid(const int64_t *n, const int cnt)
{
    int64_t max_n = 1;
    for (int i = 0; i < cnt; ++i) max_n = n[i] > max_n ? n[i] : max_n;
    int64_t bx = (max_n / 4 + 255) / 256;
    if (bx > STEP_BLOCKS_X) bx = STEP_BLOCKS_X;
    if (bx < 1) bx = 1;
    return dim3((unsigned)bx, (unsigned)cnt);
}

// Host: every tensor of a step call, checked before anything is launched.  `states`: the optimizer's fp32 state arrays (momentum
// buffers | exp_avg, exp_avg_sq), a null entry an error only when need_state; grad16_align: what a 16-bit gradient must be aligned to.
template <int N_STATES>
inline int check_step_tensors(float *const *masters, float *const *const (&states)[N_STATES], const bool need_state, const void *const *grads,
                              void *const *params16, const int64_t *numels, const int n_tensors, const int grads16, const size_t grad16_align)
{
    for (int i = 0; i < n_tensors; ++i) {
        if (!masters[i] || !grads[i] || numels[i] < 0) return RN_EINVAL;
        for (int s = 0; s < N_STATES; ++s)
            if (need_state && !states[s][i]) return RN_EINVAL;
        if (!aligned(masters[i], 16) || !aligned(grads[i], (params16[i] && grads16) ? grad16_align : 16) ||
            (params16[i] && !aligned(params16[i], 8)))
            return RN_EALIGN;
        for (int s = 0; s < N_STATES; ++s)
            if (!aligned(states[s][i], 16)) return RN_EALIGN;      // (a null state pointer is aligned)
    }
    return RN_OK;
}

}  // namespace rn
