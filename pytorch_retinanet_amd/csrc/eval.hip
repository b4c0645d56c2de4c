// COCO bbox AP on the device (coco_eval.DeviceBBoxEval): the two interpreted loops of coco_eval.BBoxEval as kernels.
//
//   rn_eval_match        per (image, category) pair the greedy matching of BBoxEval._evaluate_img, for every area range and threshold
//   rn_eval_accumulate   per (threshold, category, area range, maxDets) row the precision / recall arrays of BBoxEval.evaluate
//
// The numbered rules in include/retinanet_hip.h are the definition and BBoxEval is what they restate.  Every floating-point step of
// BBoxEval is ONE double operation on values that started as fp32, and the kernels do the same operations in the same order, so the
// results are its bits: this file is built without FMA contraction and without any fast-math flag (a fused ga - w * h moves an IoU in
// the last place and can flip a match at a tie or at a threshold).  Double division on gfx950 is correctly rounded.  No atomics; a
// result depends on nothing but the inputs.
//
// rn_eval_match: one WAVE per pair, EV_MATCH_WAVES pairs per workgroup, no barrier.  The lanes run over the pair's ground truth in
// strips of 64 (row g belongs to lane g % 64, whatever the count); the detections are walked in rank order by the whole wave.  For a
// detection every lane computes its rows' IoU once and the thresholds they reach (a T-bit mask; the wave's OR says which thresholds
// have a candidate at all, and most detections have none).  Per (area range, threshold) with a candidate: every lane picks its best
// available row -- the key is (cared-for, IoU bits), a later row wins a tie -- and two wave reductions (the largest key, then the
// largest row index among its holders) give the row the host's loop ends on.  What is matched is a 64-bit mask per row, bit a T + t:
// strip 0 keeps it in a register, rows past 64 keep theirs in gt_state (read and written by the row's own lane only).
//
// rn_eval_accumulate: one wave per row, over the category's score-sorted list in chunks of EV_CHUNK = 64 entries.  A forward pass
// counts tp, fp and the entries with rank < maxDets.  A backward pass walks the chunks from the last to the first with a carry (the
// counts at the chunk's end, the running maximum of the precision to the right): inside a chunk the counts are ballots and
// popcounts, the envelope is a suffix maximum over the lanes; the entry at which tp grows (or the first entry) owns the recall
// points in (rc before it, rc at it] and stores the envelope there -- disjoint ranges, so no two lanes write one point.  The 101
// points sit in LDS and leave in one pass.
#include "rn_common.hpp"

namespace {

constexpr int EV_WAVE = 64;
constexpr int EV_MATCH_WAVES = 4;                     // pairs per workgroup
constexpr int EV_CHUNK = 64;                          // entries per step of the accumulate scans (include/retinanet_hip.h states it)
constexpr int EV_MAX_R = 1024;                        // recall points held in LDS
constexpr double EV_EPS = 0x1p-52;                    // np.spacing(1)

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, o, EV_WAVE), hi = __shfl_xor((uint32_t)(v >> 32), o, EV_WAVE);
        const uint64_t u = ((uint64_t)hi << 32) | lo;
        v = u > v ? u : v;
    }
    return v;
}
__device__ __forceinline__ int wave_max_i(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int u = __shfl_xor(v, o, EV_WAVE);
        v = u > v ? u : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_or_u32(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, EV_WAVE);
    return v;
}
__device__ __forceinline__ int clampi(const int64_t v, const int64_t lo, const int64_t hi) { return (int)(v < lo ? lo : (v > hi ? hi : v)); }

struct Det { double x1, y1, x2, y2, area; };

// rule 2: _iou_xywh for one (detection, ground truth) -- double, one operation at a time
__device__ __forceinline__ double iou_row(const Det &d, const double *g, const bool crowd)
{
    const double gx1 = g[0], gy1 = g[1], gx2 = g[0] + g[2], gy2 = g[1] + g[3];
    double w = (d.x2 < gx2 ? d.x2 : gx2) - (d.x1 > gx1 ? d.x1 : gx1);
    double h = (d.y2 < gy2 ? d.y2 : gy2) - (d.y1 > gy1 ? d.y1 : gy1);
    w = w < 0.0 ? 0.0 : w;
    h = h < 0.0 ? 0.0 : h;
    const double inter = w * h, ga = g[2] * g[3];
    const double uni = crowd ? d.area : (d.area + ga) - inter;
    return uni > 0.0 ? inter / uni : 0.0;
}

__device__ __forceinline__ double thr_eff(const double t) { return t < 1.0 - 1e-10 ? t : 1.0 - 1e-10; }       // min(t, 1 - 1e-10)

__global__ __launch_bounds__(EV_MATCH_WAVES *EV_WAVE) void eval_match_kernel(
    const rn::f32x4 *__restrict__ dt_boxes, const double *__restrict__ gt_xywh, const double *__restrict__ gt_area,
    const uint8_t *__restrict__ gt_crowd, const int32_t *__restrict__ pairs, const int P, const int64_t D, const int64_t G,
    const double *__restrict__ thrs, const int T, const double *__restrict__ rng, const int A, const int cut,
    uint64_t *__restrict__ dt_matched, uint64_t *__restrict__ dt_ignored, uint8_t *__restrict__ gt_ignored, uint64_t *gt_state)
{
    const int p = blockIdx.x * EV_MATCH_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= P) return;                                                        // (the whole wave: there is no barrier below)
    // the table is device data: every range is clamped into the arrays
    const int db = clampi(pairs[4 * p], 0, D), de = clampi(pairs[4 * p + 1], db, D);
    const int gb = clampi(pairs[4 * p + 2], 0, G), ge = clampi(pairs[4 * p + 3], gb, G);
    const int nd_all = de - db, nd = nd_all < cut ? nd_all : cut, ng = ge - gb;
    for (int d = nd + lane; d < nd_all; d += EV_WAVE) {                        // past the cut: takes no part
        dt_matched[db + d] = 0;
        dt_ignored[db + d] = 0;
    }
    // rule 1: the ignore flags of the pair's rows, one bit per area range; the state of the rows past strip 0 starts empty
    uint32_t ig0 = 0;
    bool crowd0 = false;
    for (int g = lane; g < ng; g += EV_WAVE) {
        const double ar = gt_area[gb + g];
        const bool crowd = gt_crowd[gb + g] != 0;
        uint32_t ig = 0;
        for (int a = 0; a < A; ++a) ig |= (crowd || !(rng[2 * a] <= ar && ar <= rng[2 * a + 1])) ? 1u << a : 0u;
        gt_ignored[gb + g] = (uint8_t)ig;
        if (g < EV_WAVE) {
            ig0 = ig;
            crowd0 = crowd;
        } else {
            gt_state[gb + g] = 0;
        }
    }
    uint64_t m0 = 0;                                                           // what row ``lane`` is matched at, bit a T + t
    for (int d = 0; d < nd; ++d) {
        const rn::f32x4 b = dt_boxes[db + d];
        Det det;
        det.x1 = (double)b.x;
        det.y1 = (double)b.y;
        const double dw = (double)(b.z - b.x), dh = (double)(b.w - b.y);       // convert_to_xywh subtracts in fp32
        det.x2 = det.x1 + dw;
        det.y2 = det.y1 + dh;
        det.area = dw * dh;
        // the thresholds this detection reaches on any row (``not iou < thr``, as the host asks it)
        double iou0 = 0.0;
        uint32_t reach0 = 0, reach = 0;
        for (int g = lane; g < ng; g += EV_WAVE) {
            const double v = iou_row(det, gt_xywh + 4 * (int64_t)(gb + g), gt_crowd[gb + g] != 0);
            uint32_t r = 0;
            for (int t = 0; t < T; ++t) r |= !(v < thr_eff(thrs[t])) ? 1u << t : 0u;
            if (g < EV_WAVE) {
                iou0 = v;
                reach0 = r;
            }
            reach |= r;
        }
        reach = wave_or_u32(reach);
        uint64_t M = 0, I = 0;
        for (int a = 0; a < A; ++a) {
            const bool out = det.area < rng[2 * a] || det.area > rng[2 * a + 1];
            for (int t = 0; t < T; ++t) {
                const uint64_t bit = 1ull << (a * T + t);
                bool matched = false;
                if ((reach >> t) & 1u) {                                       // (wave-uniform)
                    const double thr = thr_eff(thrs[t]);
                    uint64_t bk = 0;
                    int bg = -1;
                    for (int g = lane; g < ng; g += EV_WAVE) {
                        double v;
                        bool crowd, ign, taken;
                        if (g < EV_WAVE) {
                            if (!((reach0 >> t) & 1u)) continue;
                            v = iou0;
                            crowd = crowd0;
                            ign = (ig0 >> a) & 1u;
                            taken = (m0 & bit) != 0;
                        } else {
                            crowd = gt_crowd[gb + g] != 0;
                            v = iou_row(det, gt_xywh + 4 * (int64_t)(gb + g), crowd);
                            if (v < thr) continue;
                            ign = (gt_ignored[gb + g] >> a) & 1u;
                            taken = (gt_state[gb + g] & bit) != 0;
                        }
                        if (taken && !crowd) continue;                         // a crowd region stays available
                        const uint64_t key = (uint64_t)__double_as_longlong(v) | (ign ? 0ull : 1ull << 63);
                        if (bg < 0 || key >= bk) {                             // rows ascend: the later row wins a tie
                            bk = key;
                            bg = g;
                        }
                    }
                    // a candidate's key is not 0: its IoU is at least a threshold
                    const uint64_t kmax = wave_max_u64(bg >= 0 ? bk : 0ull);
                    if (kmax != 0) {
                        const int gm = wave_max_i(bg >= 0 && bk == kmax ? bg : -1);
                        matched = true;
                        M |= bit;
                        if (!(kmax >> 63)) I |= bit;                           // matched to an ignored row
                        if (lane == (gm & 63)) {
                            if (gm < EV_WAVE)
                                m0 |= bit;
                            else
                                gt_state[gb + gm] |= bit;
                        }
                    }
                }
                if (!matched && out) I |= bit;
            }
        }
        if (lane == 0) {
            dt_matched[db + d] = M;
            dt_ignored[db + d] = I;
        }
    }
}

__global__ __launch_bounds__(EV_WAVE) void eval_accumulate_kernel(
    const uint64_t *__restrict__ matched, const uint64_t *__restrict__ ignored, const int32_t *__restrict__ rank,
    const int64_t *__restrict__ cat_off, const int64_t N, const int64_t *__restrict__ npig, const double *__restrict__ rec_thrs, const int R,
    const int32_t *__restrict__ max_dets, const int T, const int K, const int A, const int Mx, double *__restrict__ precision,
    double *__restrict__ recall)
{
    __shared__ double q[EV_MAX_R];
    const int lane = threadIdx.x;
    // blockIdx.x = ((k A + a) Mx + m) T + t: the rows of a category are neighbours and share its list in the caches
    int row = blockIdx.x;
    const int t = row % T;
    row /= T;
    const int m = row % Mx;
    row /= Mx;
    const int a = row % A, k = row / A;
    const int64_t am = (int64_t)A * Mx, out = ((int64_t)t * K + k) * am + (int64_t)a * Mx + m;        // recall[t][k][a][m]
    const int64_t pstride = (int64_t)K * am, pbase = (int64_t)t * R * pstride + (int64_t)k * am + (int64_t)a * Mx + m;   // precision[t][r][k][a][m]
    const int64_t np = npig[(int64_t)k * A + a];
    if (np <= 0) {                                                             // rule 6: nothing to find, the row stays at -1
        for (int r = lane; r < R; r += EV_WAVE) precision[pbase + r * pstride] = -1.0;
        if (lane == 0) recall[out] = -1.0;
        return;
    }
    int64_t b0 = cat_off[k], b1 = cat_off[k + 1];
    b0 = b0 < 0 ? 0 : (b0 > N ? N : b0);
    b1 = b1 < b0 ? b0 : (b1 > N ? N : b1);
    const int md = max_dets[m], bitpos = a * T + t;
    // forward: the counts over the whole list
    int tp_n = 0, fp_n = 0, nd_n = 0;
    for (int64_t i = b0 + lane; i < b1; i += EV_WAVE) {
        if (rank[i] < md) {
            const bool mt = (matched[i] >> bitpos) & 1ull, ig = (ignored[i] >> bitpos) & 1ull;
            nd_n += 1;
            tp_n += mt && !ig;
            fp_n += !mt && !ig;
        }
    }
    tp_n = rn::wave_sum_i(tp_n);
    fp_n = rn::wave_sum_i(fp_n);
    nd_n = rn::wave_sum_i(nd_n);
    for (int r = lane; r < R; r += EV_WAVE) q[r] = 0.0;
    __syncthreads();
    // backward: chunks of EV_CHUNK from the last to the first; the carry is the counts at the chunk's end and the maximum to its right
    const double dnp = (double)np;
    const uint64_t upto = lane == 63 ? ~0ull : (2ull << lane) - 1ull;          // lanes 0 .. lane
    int tp_end = tp_n, fp_end = fp_n, nd_end = nd_n;
    double right = -1.0;                                                       // below every precision
    const int64_t chunks = (b1 - b0 + EV_CHUNK - 1) / EV_CHUNK;
    for (int64_t c = chunks - 1; c >= 0; --c) {
        const int64_t i = b0 + c * EV_CHUNK + lane;
        bool in = false, tpf = false, fpf = false;
        if (i < b1 && rank[i] < md) {
            const bool mt = (matched[i] >> bitpos) & 1ull, ig = (ignored[i] >> bitpos) & 1ull;
            in = true;
            tpf = mt && !ig;
            fpf = !mt && !ig;
        }
        const uint64_t inb = __ballot(in), tpb = __ballot(tpf), fpb = __ballot(fpf);
        const int tp_i = tp_end - __popcll(tpb) + __popcll(tpb & upto), fp_i = fp_end - __popcll(fpb) + __popcll(fpb & upto);
        const int nd_i = nd_end - __popcll(inb) + __popcll(inb & upto);
        const double pr = in ? (double)tp_i / (((double)fp_i + (double)tp_i) + EV_EPS) : -1.0;
        double sm = pr;                                                        // the maximum over lanes >= lane
#pragma unroll
        for (int o = 1; o < EV_WAVE; o <<= 1) {
            const double u = __shfl_down(sm, o, EV_WAVE);
            if (lane + o < EV_WAVE && u > sm) sm = u;
        }
        const double env = sm > right ? sm : right;
        if (in && (tpf || nd_i == 1)) {                                        // rc grows here, or this is the list's first entry
            const double rc = (double)tp_i / dnp, before = (double)(tp_i - (tpf ? 1 : 0)) / dnp;
            const bool first = nd_i == 1;
            for (int r = 0; r < R; ++r) {
                const double thr = rec_thrs[r];
                if (thr <= rc && (first || thr > before)) q[r] = env;
            }
        }
        const double head = __shfl(sm, 0, EV_WAVE);
        right = head > right ? head : right;
        tp_end -= __popcll(tpb);
        fp_end -= __popcll(fpb);
        nd_end -= __popcll(inb);
    }
    __syncthreads();
    for (int r = lane; r < R; r += EV_WAVE) precision[pbase + r * pstride] = q[r];
    if (lane == 0) recall[out] = nd_n > 0 ? (double)tp_n / dnp : 0.0;
}

}  // namespace

RN_API int rn_eval_match(const float *dt_boxes, int64_t D, const double *gt_xywh, const double *gt_area, const uint8_t *gt_crowd, int64_t G,
                         const int32_t *pairs, int64_t P, const double *iou_thrs, int T, const double *area_rng, int A, int max_det,
                         uint64_t *dt_matched, uint64_t *dt_ignored, uint8_t *gt_ignored, uint64_t *gt_state, void *stream)
{
    if (D < 0 || G < 0 || P < 0 || D > INT32_MAX || G > INT32_MAX || P > INT32_MAX - EV_MATCH_WAVES) return RN_EINVAL;
    if (!iou_thrs || !area_rng || T < 1 || T > 32 || A < 1 || A > 8 || A * T > 64 || max_det < 1) return RN_EINVAL;
    if (D > 0 && (!dt_boxes || !dt_matched || !dt_ignored)) return RN_EINVAL;
    if (G > 0 && (!gt_xywh || !gt_area || !gt_crowd || !gt_ignored || !gt_state)) return RN_EINVAL;
    if (P > 0 && !pairs) return RN_EINVAL;
    if (!rn::aligned(dt_boxes, 16) || !rn::aligned(gt_xywh, 8) || !rn::aligned(gt_area, 8) || !rn::aligned(pairs, 4) || !rn::aligned(iou_thrs, 8) ||
        !rn::aligned(area_rng, 8) || !rn::aligned(dt_matched, 8) || !rn::aligned(dt_ignored, 8) || !rn::aligned(gt_state, 8))
        return RN_EALIGN;
    if (P == 0) return RN_OK;
    const unsigned blocks = (unsigned)((P + EV_MATCH_WAVES - 1) / EV_MATCH_WAVES);
    hipLaunchKernelGGL(eval_match_kernel, dim3(blocks), dim3(EV_MATCH_WAVES * EV_WAVE), 0, (hipStream_t)stream, (const rn::f32x4 *)dt_boxes, gt_xywh,
                       gt_area, gt_crowd, pairs, (int)P, D, G, iou_thrs, T, area_rng, A, max_det, dt_matched, dt_ignored, gt_ignored, gt_state);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

RN_API int rn_eval_accumulate(const uint64_t *matched, const uint64_t *ignored, const int32_t *rank, int64_t N, const int64_t *cat_off,
                              const int64_t *npig, const double *rec_thrs, int R, const int32_t *max_dets, int M, int T, int K, int A,
                              double *precision, double *recall, void *stream)
{
    if (N < 0 || N > INT32_MAX || K < 0 || T < 1 || T > 32 || A < 1 || A > 8 || A * T > 64 || M < 1 || R < 1 || R > EV_MAX_R) return RN_EINVAL;
    if (N > 0 && (!matched || !ignored || !rank)) return RN_EINVAL;
    if (K == 0) return RN_OK;
    if (!cat_off || !npig || !rec_thrs || !max_dets || !precision || !recall) return RN_EINVAL;
    const int64_t rows = (int64_t)T * K * A * M;
    if (rows > INT32_MAX) return RN_EINVAL;
    if (!rn::aligned(matched, 8) || !rn::aligned(ignored, 8) || !rn::aligned(rank, 4) || !rn::aligned(cat_off, 8) || !rn::aligned(npig, 8) ||
        !rn::aligned(rec_thrs, 8) || !rn::aligned(max_dets, 4) || !rn::aligned(precision, 8) || !rn::aligned(recall, 8))
        return RN_EALIGN;
    hipLaunchKernelGGL(eval_accumulate_kernel, dim3((unsigned)rows), dim3(EV_WAVE), 0, (hipStream_t)stream, matched, ignored, rank, cat_off, N, npig,
                       rec_thrs, R, max_dets, T, K, A, M, precision, recall);
    RN_LAUNCH_CHECK();
    return RN_OK;
}
