// What the two selecting matchers share -- atss.hip (rn_atss_match) and tal.hip (rn_tal_match): ONE copy of
//   the select    `append` / `shrink`: an LDS buffer of unique 64-bit keys, a radix select that leaves its k SMALLEST (the order's
//                 tie rule is part of the key, so "smallest" is the whole rule);
//   the table     the [B][A] conflict table of (IoU bits << 32) | ~GT index, posted with a 64-bit integer atomicMax -- order
//                 independent, so the same bits on every call; zero on entry, zero again after the emit;
//   the emit      `assign_emit_kernel`: the record whose key IS the table's entry won the anchor; it writes matches, the flag word
//                 and num_fg and puts the entry back to zero;
//   the prep      `assign_prep_kernel`: what a call clears, as one kernel (never hipMemsetAsync: a memset node in a captured step).
// A user supplies its own candidate walk (which keys are appended) and its own rule for which records are posted.
#pragma once
#include "rn_common.hpp"

namespace rn_assign {

typedef unsigned long long u64;

constexpr int EMIT_BLOCK = 256;

// image of GT row `row` (gt_off[0] <= row < gt_off[B]): the number of i in 1..B with gt_off[i] <= row.  Every lane of the wave calls it.
__device__ __forceinline__ int image_of_row(const int32_t *__restrict__ gt_off, const int B, const int row)
{
    const int lane = threadIdx.x & (RN_WAVE - 1);
    int cnt = 0;
    for (int i = 1 + lane; i <= B; i += RN_WAVE) cnt += gt_off[i] <= row ? 1 : 0;
    cnt = rn::wave_sum_i(cnt);
    return min(__builtin_amdgcn_readfirstlane(cnt), B - 1);
}

// the fp32 centre of both rules' step 1
__device__ __forceinline__ float centre(const float lo, const float hi) { return (lo + hi) * 0.5f; }

// the table's key of GT index `gi` (inside its image) with the fp32 IoU `iou`
__device__ __forceinline__ u64 table_key(const float iou, const uint32_t gi) { return ((u64)__float_as_uint(iou) << 32) | (uint32_t)~gi; }
__device__ __forceinline__ void table_post(u64 *__restrict__ keys, const int64_t slot, const float iou, const uint32_t gi)
{
    atomicMax(&keys[slot], table_key(iou, gi));
}

// One LDS counter bump per wave: the lanes that take a slot are numbered by their position in the ballot.  Called by whole waves.
__device__ __forceinline__ void append(u64 *__restrict__ s_key, int *__restrict__ s_n, const bool take, const u64 key)
{
    const u64 m = __ballot(take);
    if (!m) return;
    const int lane = threadIdx.x & (RN_WAVE - 1), leader = __builtin_ctzll(m);
    int base = 0;
    if (lane == leader) base = atomicAdd(s_n, __popcll(m));
    base = __shfl(base, leader, RN_WAVE);
    if (take) s_key[base + __popcll(m & ((1ull << lane) - 1ull))] = key;
}

// The buffer's n keys -> its k smallest (k <= n, keys unique), *s_thr = the k-th.  Radix select from the top byte: the histogram of
// the current byte over the keys that match the prefix found so far, wave 0 finds the bin that holds the k-th key.  The bytes of the
// index that are zero in every key are skipped, and the walk ends early when the bin is taken whole.  Ends with a barrier.
// BLOCK threads (>= 256, all of them call it), a buffer of at most BLOCK * PER keys; s_hist int[256], s_ctl int[4] ([0] the buffer's
// count; [1..3] the bin, the keys below it, the keys in it).
template <int BLOCK, int PER>
__device__ void shrink(u64 *__restrict__ s_key, int *__restrict__ s_hist, int *__restrict__ s_ctl, u64 *__restrict__ s_thr,
                       const int n, const int k, const int idx_bytes)
{
    const int tid = threadIdx.x, lane = tid & (RN_WAVE - 1);
    u64 prefix = 0ull, mask = 0ull, thr = 0ull;
    int need = k;
    bool done = false;
    for (int byte = 7; byte >= 0 && !done; --byte) {
        if (byte < 4 && byte >= idx_bytes) continue;
        const int shift = byte * 8;
        if (tid < 256) s_hist[tid] = 0;
        __syncthreads();
        for (int j = tid; j < n; j += BLOCK) {
            const u64 key = s_key[j];
            if ((key & mask) == prefix) atomicAdd(&s_hist[(int)(key >> shift) & 255], 1);
        }
        __syncthreads();
        if (tid < RN_WAVE) {
            int c[4], s = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) { c[q] = s_hist[4 * lane + q]; s += c[q]; }
            int incl = s;
#pragma unroll
            for (int o = 1; o < RN_WAVE; o <<= 1) {
                const int t = __shfl_up(incl, o, RN_WAVE);
                if (lane >= o) incl += t;
            }
            int run = incl - s;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (run < need && need <= run + c[q]) { s_ctl[1] = 4 * lane + q; s_ctl[2] = run; s_ctl[3] = c[q]; }
                run += c[q];
            }
        }
        __syncthreads();
        const int bin = s_ctl[1], cnt = s_ctl[3];
        need -= s_ctl[2];
        prefix |= (u64)bin << shift;
        mask |= 0xffull << shift;
        if (cnt == need) {                              // the whole bin is taken: every key below prefix | (all ones under the byte)
            thr = prefix | ((1ull << shift) - 1ull);
            done = true;
        }
    }
    if (!done) thr = prefix;
    u64 mine[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int j = tid + q * BLOCK;
        mine[q] = j < n ? s_key[j] : 0ull;
    }
    __syncthreads();
    if (tid == 0) { s_ctl[0] = 0; *s_thr = thr; }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PER; ++q) append(s_key, &s_ctl[0], tid + q * BLOCK < n && mine[q] <= thr, mine[q]);
    __syncthreads();
}

// The emit: one thread per record (cand_idx, cand_iou: [rows][n]; an index of -1 = not posted).  The record whose key is the
// table's entry owns the anchor.
static __global__ __launch_bounds__(EMIT_BLOCK) void assign_emit_kernel(
    const int32_t *__restrict__ gt_off, const int B, const int64_t A, const int n, const int32_t *__restrict__ cand_idx,
    const float *__restrict__ cand_iou, u64 *__restrict__ keys, int64_t *__restrict__ matches, int32_t *__restrict__ num_fg,
    u64 *__restrict__ special)
{
    const int r = blockIdx.x;
    const int row = gt_off[0] + r;
    if (row >= gt_off[B]) return;
    const int b = image_of_row(gt_off, B, row);
    const uint32_t gi = (uint32_t)(row - gt_off[b]);
    const int c = blockIdx.y * EMIT_BLOCK + threadIdx.x;
    bool win = false;
    if (c < n) {
        const int a_idx = cand_idx[(int64_t)r * n + c];
        if (a_idx >= 0) {
            const u64 key = table_key(cand_iou[(int64_t)r * n + c], gi);
            u64 *__restrict__ e = &keys[(int64_t)b * A + a_idx];
            win = *e == key;
            if (win) {
                *e = 0ull;
                matches[(int64_t)b * A + a_idx] = (int64_t)gi;
                if (special) atomicOr(&special[(int64_t)b * ((A + 63) >> 6) + (a_idx >> 6)], 1ull << (a_idx & 63));
            }
        }
    }
    if (num_fg) {
        const u64 w = __ballot(win);
        if ((threadIdx.x & (RN_WAVE - 1)) == 0 && w) atomicAdd(&num_fg[b], __popcll(w));
    }
}

// what the call clears, as ONE kernel (never hipMemsetAsync: a memset node in a captured step, see match.hip)
static __global__ __launch_bounds__(256) void assign_prep_kernel(u64 *__restrict__ special, const int64_t n_special,
                                                                 int32_t *__restrict__ num_fg, const int n_fg,
                                                                 int64_t *__restrict__ matches, const int64_t n_matches)
{
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    for (int64_t i = t0; i < n_special; i += step) special[i] = 0ull;
    for (int64_t i = t0; i < n_fg; i += step) num_fg[i] = 0;
    for (int64_t i = t0; i < n_matches; i += step) matches[i] = -1;
}

static inline size_t align16(const size_t v) { return (v + 15) & ~(size_t)15; }

// The prep launch of a call: the flag words = 0, num_fg = 0 (unless RN_MATCH_NUM_FG_ZEROED), matches = -1 (unless RN_MATCH_FLAGGED_ONLY).
static inline int launch_prep(const int B, const int64_t A, int64_t *matches, int32_t *num_fg, u64 *special, const int flags, hipStream_t st)
{
    const int64_t n_special = special ? (int64_t)B * ((A + 63) >> 6) : 0;
    const int n_fg = (num_fg && !(flags & RN_MATCH_NUM_FG_ZEROED)) ? B : 0;
    const int64_t n_matches = (flags & RN_MATCH_FLAGGED_ONLY) ? 0 : (int64_t)B * A;
    const int64_t most = n_matches > n_special ? n_matches : (n_special > n_fg ? n_special : n_fg);
    if (most > 0) {
        int64_t blocks = (most + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(assign_prep_kernel, dim3((unsigned)blocks), dim3(256), 0, st, special, n_special, num_fg, n_fg, matches, n_matches);
        RN_LAUNCH_CHECK();
    }
    return RN_OK;
}

static inline int launch_emit(const int64_t total_gt, const int n, const int32_t *gt_off, const int B, const int64_t A,
                              const int32_t *cand_idx, const float *cand_iou, u64 *keys, int64_t *matches, int32_t *num_fg,
                              u64 *special, hipStream_t st)
{
    hipLaunchKernelGGL(assign_emit_kernel, dim3((unsigned)total_gt, (unsigned)((n + EMIT_BLOCK - 1) / EMIT_BLOCK)), dim3(EMIT_BLOCK), 0, st,
                       gt_off, B, A, n, cand_idx, cand_iou, keys, matches, num_fg, special);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

}  // namespace rn_assign
