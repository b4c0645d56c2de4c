// K6, the soft kinds: Soft-NMS (Bodla et al., ICCV 2017), linear and Gaussian -- the numbered rule next to K6 in
// include/retinanet_hip.h.  Same interface as rn::launch_nms (rn_internal.hpp): unsorted (inv_ordered(score) << 32) | payload keys per
// segment in, the survivors' keys -- carrying the score each one had when it was picked -- in pick order out.  Nothing is sorted: every
// round picks the smallest live key (highest current score, lower payload on ties), emits it and decays the live entries that overlap
// it, and the decay pass finds the next round's local minimum on the way.  The emitted keys never decrease, so kept[] is in key order
// as launch_nms leaves it, and topk_kernel reads the scores from the keys.
//
// One workgroup per segment, two launches over every segment (a block exits at once when the segment is not in its class):
//   n <= 64     soft_wave_kernel: one wave, one entry per lane, the minimum by shuffles, the picked box by a lane read -- no LDS,
//               no barrier.
//   larger      soft_block_kernel, 256 threads:
//                 n <= 2048: up to 8 entries per thread in registers (key, box, area); per round one wave minimum by shuffles,
//                            the four wave minima AND their boxes through a double-buffered LDS slot, ONE barrier;
//                 beyond:    the same loop with the keys in a.keys and the gathered boxes in a.scratch_boxes (HBM); a thread
//                            only ever reads back what it wrote itself, so nothing but the round's barrier orders anything.
// No atomics: the same bits on every call.  fp32 steps are single rounded operations (the file is compiled with -ffp-contract=off and
// IEEE divides); the Gaussian weight goes through double exp as the rule says.
#include "rn_internal.hpp"

#include <math.h>

namespace {

using rn::f32x4;

constexpr int SOFT_THREADS = 256;
constexpr int SOFT_WAVES = SOFT_THREADS / RN_WAVE;
constexpr int SOFT_EPT = 8;                              // entries per thread of the register form
constexpr int SOFT_CAP = SOFT_THREADS * SOFT_EPT;        // 2048
constexpr uint64_t DEAD = ~0ull;                         // (a live key never has this value: it would be a NaN score with payload 2^32 - 1)

struct SoftRule {
    float thr;           // linear: the IoU above which a score decays
    double sigma;        // Gaussian: (double)sigma
    float min_score;
    int max_keep;        // 0: no cap
};

// K6's IoU: one fp32 operation per step, the comparisons as `overlaps` in nms.hip writes them.
__device__ __forceinline__ float iou_of(const f32x4 bi, const float ai, const f32x4 bj, const float aj)
{
    const float xx1 = bi.x > bj.x ? bi.x : bj.x;
    const float yy1 = bi.y > bj.y ? bi.y : bj.y;
    const float xx2 = bi.z < bj.z ? bi.z : bj.z;
    const float yy2 = bi.w < bj.w ? bi.w : bj.w;
    float w = xx2 - xx1; w = w > 0.0f ? w : 0.0f;
    float h = yy2 - yy1; h = h > 0.0f ? h : 0.0f;
    const float inter = w * h;
    return inter / ((ai + aj) - inter);
}

// Step 4 of the rule for one live entry: its key after the pick of a box it overlaps by `iou`.
template <int METHOD>
__device__ __forceinline__ uint64_t decayed(const uint64_t key, const float iou, const SoftRule &r)
{
    if (!(iou > 0.0f)) return key;                       // NaN and empty unions too
    float s = rn::score_of((uint32_t)(key >> 32));
    if (METHOD == RN_NMS_SOFT_LINEAR) {
        if (!(iou > r.thr)) return key;
        const float w = 1.0f - iou;
        s = s * w;
    } else {
        const double d = (double)iou;
        const float w = (float)exp(-(d * d) / r.sigma);
        s = s * w;
    }
    return ((uint64_t)rn::inv_ordered(s) << 32) | (uint32_t)key;
}

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, RN_WAVE), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, RN_WAVE);
        const uint64_t u = ((uint64_t)hi << 32) | lo;
        v = u < v ? u : v;
    }
    return v;
}

// Steps 2 and 3's test: false when the round must not happen.
__device__ __forceinline__ bool goes_on(const uint64_t best, const int kept, const SoftRule &r)
{
    if (best == DEAD) return false;
    if (!(rn::score_of((uint32_t)(best >> 32)) > r.min_score)) return false;
    return !(r.max_keep > 0 && kept >= r.max_keep);
}

__device__ __forceinline__ void emit(const rn::NmsLaunch &a, const int64_t at, const uint64_t key)
{
    a.kept[at] = key;
    if (a.keep_idx) a.keep_idx[at] = (int64_t)(uint32_t)key;
}

template <int METHOD>
__global__ __launch_bounds__(RN_WAVE) void soft_wave_kernel(const rn::NmsLaunch a, const SoftRule r)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    const int n = a.seg_len[s];
    if (n > RN_WAVE) return;
    if (n <= 0) {
        if (lane == 0) a.kept_count[s] = 0;
        return;
    }
    const int64_t start = a.seg_start[s];
    const int64_t box_base = a.box_mode ? (int64_t)(s / a.K) * a.A : start;
    uint64_t key = DEAD;
    f32x4 b = {0.0f, 0.0f, 0.0f, 0.0f};
    if (lane < n) {
        key = a.keys[start + lane];
        b = a.boxes[box_base + (uint32_t)key];
    }
    const float area = (b.z - b.x) * (b.w - b.y);
    int kept = 0;
    while (true) {
        const uint64_t best = wave_min_u64(key);
        if (!goes_on(best, kept, r)) break;                                 // (wave-uniform)
        const int src = __builtin_ctzll(__ballot(key == best));            // keys are unique: one lane
        f32x4 pb;
        pb.x = __shfl(b.x, src, RN_WAVE); pb.y = __shfl(b.y, src, RN_WAVE); pb.z = __shfl(b.z, src, RN_WAVE); pb.w = __shfl(b.w, src, RN_WAVE);
        const float pa = __shfl(area, src, RN_WAVE);
        if (lane == src) {
            emit(a, start + kept, best);
            key = DEAD;
        } else if (key != DEAD) {
            key = decayed<METHOD>(key, iou_of(pb, pa, b, area), r);
        }
        ++kept;
    }
    if (lane == 0) a.kept_count[s] = kept;
}

// The block-wide argmin of a round: every thread brings its smallest live key and that entry's box; returns the smallest of all and
// its box.  The wave minimum is found by shuffles, its owner lane (keys are unique) puts key and box into the round's LDS slot, and
// after the ONE barrier every thread reads the SOFT_WAVES slots.  The slots are double-buffered by the round's parity: a wave that
// writes slot p in round r + 2 has passed the barrier of round r + 1, which every wave reaches only after its reads of round r.
__device__ __forceinline__ uint64_t block_pick(uint64_t (*s_key)[SOFT_WAVES], f32x4 (*s_box)[SOFT_WAVES], const int par, const uint64_t lmin,
                                               const f32x4 lbox, f32x4 &pb)
{
    const int lane = threadIdx.x & (RN_WAVE - 1), wave = threadIdx.x / RN_WAVE;
    const uint64_t wmin = wave_min_u64(lmin);
    if (wmin != DEAD ? lmin == wmin : lane == 0) {
        s_key[par][wave] = wmin;
        s_box[par][wave] = lbox;
    }
    __syncthreads();
    uint64_t best = s_key[par][0];
    int bw = 0;
#pragma unroll
    for (int w = 1; w < SOFT_WAVES; ++w) {
        const uint64_t k = s_key[par][w];
        if (k < best) { best = k; bw = w; }
    }
    pb = s_box[par][bw];
    return best;
}

// 64 < n <= SOFT_CAP: entry i = e * SOFT_THREADS + t in register set e of thread t.
template <int METHOD>
__device__ __forceinline__ void soft_regs_body(const rn::NmsLaunch &a, const SoftRule &r, const int n, uint64_t (*s_key)[SOFT_WAVES],
                                               f32x4 (*s_box)[SOFT_WAVES])
{
    const int s = blockIdx.x, t = threadIdx.x;
    const int64_t start = a.seg_start[s];
    const int64_t box_base = a.box_mode ? (int64_t)(s / a.K) * a.A : start;
    const int ne = (n + SOFT_THREADS - 1) / SOFT_THREADS;                   // register sets in use (uniform)
    uint64_t key[SOFT_EPT];
    f32x4 box[SOFT_EPT];
    float area[SOFT_EPT];
    uint64_t lmin = DEAD;
    f32x4 lbox = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int e = 0; e < SOFT_EPT; ++e) {
        const int i = e * SOFT_THREADS + t;
        key[e] = DEAD;
        box[e] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (i < n) {
            key[e] = a.keys[start + i];
            box[e] = a.boxes[box_base + (uint32_t)key[e]];
        }
        area[e] = (box[e].z - box[e].x) * (box[e].w - box[e].y);
        if (key[e] < lmin) { lmin = key[e]; lbox = box[e]; }
    }
    int kept = 0, par = 0;
    while (true) {
        f32x4 pb;
        const uint64_t best = block_pick(s_key, s_box, par, lmin, lbox, pb);
        if (!goes_on(best, kept, r)) break;                                 // (workgroup-uniform: every thread read the same slots)
        const float pa = (pb.z - pb.x) * (pb.w - pb.y);
        if (lmin == best) emit(a, start + kept, best);
        lmin = DEAD;
#pragma unroll
        for (int e = 0; e < SOFT_EPT; ++e) {
            if (e < ne) {
                uint64_t k = key[e];
                if (k == best) k = DEAD;
                else if (k != DEAD) k = decayed<METHOD>(k, iou_of(pb, pa, box[e], area[e]), r);
                key[e] = k;
                if (k < lmin) { lmin = k; lbox = box[e]; }
            }
        }
        ++kept;
        par ^= 1;
    }
    if (t == 0) a.kept_count[s] = kept;
}

// n > SOFT_CAP: the same loop, the current keys in a.keys and the gathered boxes in a.scratch_boxes.  Thread t owns the entries
// i = t (mod SOFT_THREADS) and is the only one to read or write them.
template <int METHOD>
__device__ __forceinline__ void soft_hbm_body(const rn::NmsLaunch &a, const SoftRule &r, const int n, uint64_t (*s_key)[SOFT_WAVES],
                                              f32x4 (*s_box)[SOFT_WAVES])
{
    const int s = blockIdx.x, t = threadIdx.x;
    const int64_t start = a.seg_start[s];
    const int64_t box_base = a.box_mode ? (int64_t)(s / a.K) * a.A : start;
    uint64_t *keys = a.keys + start;
    f32x4 *g_box = a.scratch_boxes + start;
    uint64_t lmin = DEAD;
    f32x4 lbox = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = t; i < n; i += SOFT_THREADS) {
        const uint64_t k = keys[i];
        const f32x4 b = a.boxes[box_base + (uint32_t)k];
        g_box[i] = b;
        if (k < lmin) { lmin = k; lbox = b; }
    }
    int kept = 0, par = 0;
    while (true) {
        f32x4 pb;
        const uint64_t best = block_pick(s_key, s_box, par, lmin, lbox, pb);
        if (!goes_on(best, kept, r)) break;
        const float pa = (pb.z - pb.x) * (pb.w - pb.y);
        if (lmin == best) emit(a, start + kept, best);
        lmin = DEAD;
        for (int i = t; i < n; i += SOFT_THREADS) {
            const uint64_t k = keys[i];
            if (k == DEAD) continue;
            if (k == best) { keys[i] = DEAD; continue; }
            const f32x4 b = g_box[i];
            const uint64_t nk = decayed<METHOD>(k, iou_of(pb, pa, b, (b.z - b.x) * (b.w - b.y)), r);
            if (nk != k) keys[i] = nk;
            if (nk < lmin) { lmin = nk; lbox = b; }
        }
        ++kept;
        par ^= 1;
    }
    if (t == 0) a.kept_count[s] = kept;
}

template <int METHOD>
__global__ __launch_bounds__(SOFT_THREADS) void soft_block_kernel(const rn::NmsLaunch a, const SoftRule r)
{
    __shared__ uint64_t s_key[2][SOFT_WAVES];
    __shared__ f32x4 s_box[2][SOFT_WAVES];
    const int n = a.seg_len[blockIdx.x];
    if (n <= RN_WAVE) return;
    if (n <= SOFT_CAP) soft_regs_body<METHOD>(a, r, n, s_key, s_box);
    else soft_hbm_body<METHOD>(a, r, n, s_key, s_box);
}

// keep_scores of the op entry: the score field of the survivors' keys, zero in the rest of the segment.
__global__ __launch_bounds__(256) void soft_scores_kernel(const uint64_t *__restrict__ kept, const int64_t *__restrict__ seg_start,
                                                          const int32_t *__restrict__ seg_len, const int32_t *__restrict__ kept_count,
                                                          float *__restrict__ keep_scores)
{
    const int s = blockIdx.x;
    const int n = seg_len[s], m = kept_count[s];
    const int64_t start = seg_start[s];
    for (int i = threadIdx.x; i < n; i += 256) keep_scores[start + i] = i < m ? rn::score_of((uint32_t)(kept[start + i] >> 32)) : 0.0f;
}

}  // namespace

int rn::launch_soft_nms(const rn::NmsLaunch &a, int method, float sigma, float min_score, hipStream_t st)
{
    if (method != RN_NMS_SOFT_LINEAR && method != RN_NMS_SOFT_GAUSSIAN) return RN_EINVAL;
    if (a.S <= 0) return RN_OK;
    SoftRule r;
    r.thr = a.iou_thr; r.sigma = (double)sigma; r.min_score = min_score; r.max_keep = a.max_keep > 0 ? a.max_keep : 0;
    const dim3 grid((unsigned)a.S);
    if (method == RN_NMS_SOFT_LINEAR) {
        hipLaunchKernelGGL((soft_wave_kernel<RN_NMS_SOFT_LINEAR>), grid, dim3(RN_WAVE), 0, st, a, r);
        RN_LAUNCH_CHECK();
        hipLaunchKernelGGL((soft_block_kernel<RN_NMS_SOFT_LINEAR>), grid, dim3(SOFT_THREADS), 0, st, a, r);
    } else {
        hipLaunchKernelGGL((soft_wave_kernel<RN_NMS_SOFT_GAUSSIAN>), grid, dim3(RN_WAVE), 0, st, a, r);
        RN_LAUNCH_CHECK();
        hipLaunchKernelGGL((soft_block_kernel<RN_NMS_SOFT_GAUSSIAN>), grid, dim3(SOFT_THREADS), 0, st, a, r);
    }
    RN_LAUNCH_CHECK();
    return RN_OK;
}

RN_API int rn_soft_nms_segments(const float *boxes, const float *scores, const int32_t *seg_off, int S, int64_t N, float iou_thr,
                                const rn_nms_params *nms, int64_t *keep, float *keep_scores, int32_t *keep_count, void *workspace,
                                size_t workspace_bytes, void *stream)
{
    if (!seg_off || !keep_count || !nms || S <= 0 || N < 0) return RN_EINVAL;
    if (N > 0 && (!boxes || !scores || !keep || !keep_scores)) return RN_EINVAL;
    if (nms->method == RN_NMS_HARD || rn::check_nms_params(nms) != RN_OK) return RN_EINVAL;       // (the hard kind is rn_nms_segments)
    if (N >= ((int64_t)1 << 31)) return RN_EUNSUPPORTED;
    if (!workspace || workspace_bytes < rn_nms_workspace_bytes(N, S)) return RN_EWORKSPACE;
    if ((boxes && !rn::aligned(boxes, 16)) || !rn::aligned(workspace, 16)) return RN_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    rn::NmsLaunch a;
    int rc = rn::nms_op_prepare(boxes, scores, seg_off, S, N, iou_thr, keep, keep_count, workspace, a, st);
    if (rc != RN_OK) return rc;
    a.max_keep = nms->max_keep > 0 ? nms->max_keep : 0;
    rc = rn::launch_soft_nms(a, nms->method, nms->sigma, nms->min_score, st);
    if (rc != RN_OK) return rc;
    hipLaunchKernelGGL(soft_scores_kernel, dim3((unsigned)S), dim3(256), 0, st, a.kept, a.seg_start, a.seg_len, keep_count, keep_scores);
    RN_LAUNCH_CHECK();
    return RN_OK;
}
