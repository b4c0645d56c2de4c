// Train-time shift / scale / rotate drawn and applied on the device (augment.ShiftScaleRotate: albumentations' ShiftScaleRotate with
// bilinear interpolation and the reflect-101 border in intent, not bit for bit).  Like the bbox-safe crop it is a second staging pass
// over staged images and packed GT, so nothing downstream changes:
//
//   rn_affine_draw        coef[b] = {m, inv, applied, kept}; the rows that survive, packed, with their labels and offsets; counter += 1
//   rn_image_warp_stage   image b of arena slot b gathered through inv (bilinear, reflect-101) into slot b of a second arena, same (h, w)
//
// The numbered rule in include/retinanet_hip.h is the definition; augment.ShiftScaleRotate restates it (draw_coefs, warp_boxes,
// warp_image).  This file is built without FMA contraction and with IEEE division.
//
// The draw is three launches and no atomics.  affine_coef_kernel, one wave per image: every lane draws the same five uniforms and
// computes the same matrices in double; the lanes walk the image's rows and count the ones step 3 keeps (a wave reduction); lane 0
// writes coef[b].  affine_rows_kernel, one wave per image again: the wave adds the kept counts of the images before it (a wave
// reduction in index order: O(B) per image, B is a batch size), then walks its rows 64 at a time and packs the kept ones with a
// ballot -- a row's place is the number of kept rows before it, so the order within an image stays.  Both kernels take a row's fate
// from one function (warp_box), so the count and the packing cannot disagree.  Every wave of the first kernel reads the counter, so a
// single-wave launch behind the other two advances it.
//
// The warp is a gather: four taps per channel and pixel, each a 4-byte load, and one dense store.  A fixed grid of WS_BLOCKS blocks
// per image walks 32 x 32 destination tiles -- under a rotation the source footprint of a square tile is a square of about the same
// size, which the caches hold, where a row of 1024 pixels would sweep a diagonal.  A thread owns four pixels; it computes their
// source indices and weights ONCE and applies them to the three channels.  Where w % 4 == 0 and the destination slot is 16-byte
// aligned a thread's pixels are four neighbours of one row and leave as one 16-byte store per channel (a wave writes 128-byte row
// segments); else they are one column position in four rows and a wave writes 128-byte row segments with 4-byte stores.  An image
// that is left alone (applied = 0) takes a flat copy: the branch depends on blockIdx.y alone, so it is uniform across the block.
#include <stddef.h>

#include "rn_common.hpp"
#include "rn_draw.hpp"

namespace {

constexpr int AF_WAVE = 64;
constexpr uint64_t AF_SALT_APPLY = 0xA551A551A551A551ull, AF_SALT_ANGLE = 0xA4613A4613A46135ull, AF_SALT_SCALE = 0x5CA7E5CA7E5CA7E5ull,
                   AF_SALT_DX = 0xD0C5D0C5D0C5D0C5ull, AF_SALT_DY = 0xD1E7D1E7D1E7D1E7ull;
constexpr double AF_MIN_DET = 1e-12;                  // step 2: below it the matrix is not inverted and the image is left alone

__device__ __forceinline__ float min2(const float p, const float q) { return q < p ? q : p; }
__device__ __forceinline__ float max2(const float p, const float q) { return q > p ? q : p; }
__device__ __forceinline__ float clamp0(const float v, const float hi) { return v < 0.0f ? 0.0f : (v > hi ? hi : v); }

// step 3 for one row: the clamped box in ``o``; true when the row is kept
__device__ __forceinline__ bool warp_box(const float *m, const float fw, const float fh, const float mv, const rn::f32x4 v, rn::f32x4 &o)
{
    const float xs[4] = {v.x, v.z, v.z, v.x}, ys[4] = {v.y, v.y, v.w, v.w};
    float X[4], Y[4];
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        X[k] = (m[0] * xs[k] + m[1] * ys[k]) + m[2];
        Y[k] = (m[3] * xs[k] + m[4] * ys[k]) + m[5];
        finite = finite && isfinite(X[k]) && isfinite(Y[k]);
    }
    const float X1 = min2(min2(min2(X[0], X[1]), X[2]), X[3]), X2 = max2(max2(max2(X[0], X[1]), X[2]), X[3]);
    const float Y1 = min2(min2(min2(Y[0], Y[1]), Y[2]), Y[3]), Y2 = max2(max2(max2(Y[0], Y[1]), Y[2]), Y[3]);
    o.x = clamp0(X1, fw);
    o.y = clamp0(Y1, fh);
    o.z = clamp0(X2, fw);
    o.w = clamp0(Y2, fh);
    const float au = (X2 - X1) * (Y2 - Y1), cw = o.z - o.x, ch = o.w - o.y;
    const float ac = cw * ch;
    return finite && cw > 0.0f && ch > 0.0f && ac >= mv * au;
}

__device__ __forceinline__ void row_range(const int32_t *__restrict__ gt_off, const int b, const int32_t rows, int32_t &lo, int32_t &hi)
{
    lo = gt_off[b];
    hi = gt_off[b + 1];
    lo = lo < 0 ? 0 : (lo > rows ? rows : lo);                                  // (device data: the rows stay inside the buffers)
    hi = hi < lo ? lo : (hi > rows ? rows : hi);
}

// (the Python side packs the block by these offsets -- draw_state.py's layout table: a struct edit that it does not follow fails here)
static_assert(sizeof(rn_affine_state) == 56 && offsetof(rn_affine_state, seed) == 0 && offsetof(rn_affine_state, counter) == 8 &&
                  offsetof(rn_affine_state, p) == 16 && offsetof(rn_affine_state, min_visibility) == 20 && offsetof(rn_affine_state, lo) == 24 &&
                  offsetof(rn_affine_state, hi) == 40, "draw_state.AFFINE");

// one wave per image (blockIdx.x); the state block is only read here
__global__ __launch_bounds__(AF_WAVE) void affine_coef_kernel(const rn_affine_state *__restrict__ st, const rn::f32x4 *__restrict__ in,
                                                             const int32_t *__restrict__ gt_off, const int32_t *__restrict__ in_hw,
                                                             rn_affine_coef *__restrict__ coef, const int32_t rows)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const uint64_t seed = st->seed;
    const int64_t counter = st->counter;
    const float mv = st->min_visibility;
    const int h = in_hw[2 * b], w = in_hw[2 * b + 1];
    int32_t lo, hi;
    row_range(gt_off, b, rows, lo, hi);
    // step 1
    const bool applied = hflip_u(seed ^ AF_SALT_APPLY, counter, b) < st->p;
    const float angle = st->lo[0] + hflip_u(seed ^ AF_SALT_ANGLE, counter, b) * (st->hi[0] - st->lo[0]);
    const float scale = st->lo[1] + hflip_u(seed ^ AF_SALT_SCALE, counter, b) * (st->hi[1] - st->lo[1]);
    const float dx = st->lo[2] + hflip_u(seed ^ AF_SALT_DX, counter, b) * (st->hi[2] - st->lo[2]);
    const float dy = st->lo[3] + hflip_u(seed ^ AF_SALT_DY, counter, b) * (st->hi[3] - st->lo[3]);
    // step 2
    const double t = (double)angle * 3.14159265358979323846 / 180.0;
    const double ca = (double)scale * cos(t), sb = (double)scale * sin(t);
    const double cx = ((double)w - 1.0) / 2.0, cy = ((double)h - 1.0) / 2.0;
    const double tx = ((1.0 - ca) * cx - sb * cy) + (double)dx * (double)w, ty = (sb * cx + (1.0 - ca) * cy) + (double)dy * (double)h;
    const double det = ca * ca + sb * sb;
    const double i00 = ca / det, i01 = -sb / det, i10 = sb / det, i11 = ca / det;
    float m[6] = {(float)ca, (float)sb, (float)tx, (float)-sb, (float)ca, (float)ty};
    float inv[6] = {(float)i00, (float)i01, (float)-(i00 * tx + i01 * ty), (float)i10, (float)i11, (float)-(i10 * tx + i11 * ty)};
    bool ok = applied && h >= 1 && w >= 1 && det >= AF_MIN_DET;
#pragma unroll
    for (int k = 0; k < 6; ++k) ok = ok && isfinite(m[k]) && isfinite(inv[k]);
    // step 3: how many rows stay
    int kept = 0;
    if (ok) {
        const float fw = (float)w, fh = (float)h;
        for (int32_t r = lo + lane; r < hi; r += AF_WAVE) {
            rn::f32x4 o;
            kept += warp_box(m, fw, fh, mv, in[r], o) ? 1 : 0;
        }
        kept = rn::wave_sum_i(kept);
        if (hi > lo && kept == 0) ok = false;                                   // (no image loses all of its GT)
    }
    if (!ok) {
        kept = hi - lo;
#pragma unroll
        for (int k = 0; k < 6; ++k) m[k] = inv[k] = (k == 0 || k == 4) ? 1.0f : 0.0f;
    }
    if (lane == 0) {
        rn_affine_coef c;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            c.m[k] = m[k];
            c.inv[k] = inv[k];
        }
        c.applied = ok ? 1 : 0;
        c.kept = kept;
        c.reserved[0] = c.reserved[1] = 0;
        coef[b] = c;
    }
}

// one wave per image (blockIdx.x): the image's offset from the counts before it, then its kept rows packed in order
__global__ __launch_bounds__(AF_WAVE) void affine_rows_kernel(const rn_affine_state *__restrict__ st, const rn::f32x4 *__restrict__ in,
                                                             const int64_t *__restrict__ labels, const int32_t *__restrict__ gt_off,
                                                             const int32_t *__restrict__ in_hw, const rn_affine_coef *__restrict__ coef,
                                                             const int B, rn::f32x4 *__restrict__ out, int64_t *__restrict__ out_labels,
                                                             int32_t *__restrict__ out_gt_off, const int32_t rows)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    // the rows of the images before this one: integers, so the order of the additions does not matter.  No count exceeds rows
    // (affine_coef_kernel clamped the range it counted), so 65535 of them stay far inside 64 bits
    int64_t before = 0;
    for (int i = lane; i < b; i += AF_WAVE) before += coef[i].kept;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {                                          // (a 64-bit butterfly out of 32-bit shuffles, as rn::wave_sum_d)
        const uint64_t u = (uint64_t)before;
        const unsigned lo32 = __shfl_xor((unsigned)u, o, AF_WAVE), hi32 = __shfl_xor((unsigned)(u >> 32), o, AF_WAVE);
        before += (int64_t)(((uint64_t)hi32 << 32) | lo32);
    }
    const int mine = coef[b].kept, applied = coef[b].applied;
    const int64_t base64 = before < (int64_t)rows ? before : (int64_t)rows;
    const int32_t base = (int32_t)(base64 < 0 ? 0 : base64);
    if (lane == 0) {
        out_gt_off[b] = base;
        if (b == B - 1) {
            int64_t end = (int64_t)base + (mine > 0 ? mine : 0);
            out_gt_off[B] = (int32_t)(end < (int64_t)rows ? end : (int64_t)rows);
        }
    }
    int32_t lo, hi;
    row_range(gt_off, b, rows, lo, hi);
    const float mv = st->min_visibility;
    const float fw = (float)in_hw[2 * b + 1], fh = (float)in_hw[2 * b];
    float m[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) m[k] = coef[b].m[k];
    int64_t at = base;                                                          // (64 bits: hostile offsets cannot wrap it)
    for (int32_t r0 = lo; r0 < hi; r0 += AF_WAVE) {
        const int32_t r = r0 + lane;
        const bool valid = r < hi;
        rn::f32x4 v, o;
        v.x = v.y = v.z = v.w = 0.0f;
        if (valid) v = in[r];
        o = v;                                                                  // (an image left alone: copied bit for bit)
        const bool keep = valid && (applied ? warp_box(m, fw, fh, mv, v, o) : true);
        const unsigned long long mask = __ballot(keep);
        const int64_t dst = at + __popcll(mask & ((1ull << lane) - 1ull));
        if (keep && dst < (int64_t)rows) {                                      // (never past the buffers, whatever gt_off claims)
            out[dst] = o;
            out_labels[dst] = labels[r];
        }
        at += __popcll(mask);
    }
}

// ---- the warp ------------------------------------------------------------------------------------------------------------------
constexpr int WS_BLOCKS = 256;      // blocks per image: fixed, so neither the grid nor an argument depends on a size
constexpr int WS_BLOCK = 256;
constexpr int WS_TILE = 32;         // a block's destination tile is WS_TILE x WS_TILE pixels: four per thread
static_assert(WS_TILE * WS_TILE == 4 * WS_BLOCK, "four pixels per thread");

__device__ __forceinline__ float sat30(float s)
{
    s = s >= -0x1p30f ? s : -0x1p30f;                                           // (a NaN becomes -2^30: the conversion below is defined)
    return s <= 0x1p30f ? s : 0x1p30f;
}

// reflect-101 without a loop: i in [-2^30, 2^30 + 1], n >= 1, period = 2 (n - 1); the result is in [0, n) for every i
__device__ __forceinline__ int reflect101(const int i, const int n, const int period)
{
    if ((unsigned)i < (unsigned)n) return i;                                    // (inside: i mod period is i itself)
    if (n == 1) return 0;
    int t = i % period;
    t = t < 0 ? t + period : t;
    return t < n ? t : period - t;
}

// the four source offsets inside a plane and the two weights of one destination pixel: computed once, used by the three channels
struct Tap { uint32_t o00, o01, o10, o11; float fx, fy; };

__device__ __forceinline__ Tap make_tap(const float *inv, const int x, const int y, const int h, const int w)
{
    const float X = (float)x, Y = (float)y;
    const float sx = sat30((inv[0] * X + inv[1] * Y) + inv[2]), sy = sat30((inv[3] * X + inv[4] * Y) + inv[5]);
    const float flx = floorf(sx), fly = floorf(sy);
    const int x0 = (int)flx, y0 = (int)fly;
    const int xa = reflect101(x0, w, 2 * (w - 1)), xb = reflect101(x0 + 1, w, 2 * (w - 1));
    const int ya = reflect101(y0, h, 2 * (h - 1)), yb = reflect101(y0 + 1, h, 2 * (h - 1));
    Tap t;
    t.fx = sx - flx;
    t.fy = sy - fly;
    t.o00 = (uint32_t)ya * (uint32_t)w + (uint32_t)xa;                          // (< h w <= slot / 3 < 2^31)
    t.o01 = (uint32_t)ya * (uint32_t)w + (uint32_t)xb;
    t.o10 = (uint32_t)yb * (uint32_t)w + (uint32_t)xa;
    t.o11 = (uint32_t)yb * (uint32_t)w + (uint32_t)xb;
    return t;
}

__device__ __forceinline__ float tap_sample(const float *__restrict__ p, const Tap &t)
{
    const float gx = 1.0f - t.fx, gy = 1.0f - t.fy;
    return (p[t.o00] * gx + p[t.o01] * t.fx) * gy + (p[t.o10] * gx + p[t.o11] * t.fx) * t.fy;
}

// VEC: a thread's four pixels are neighbours in one row (w % 4 == 0, d 16-byte aligned); else one column position in four rows
template <bool VEC>
__device__ __forceinline__ void warp_tiles(const float *__restrict__ s, float *__restrict__ d, const int h, const int w, const float *inv)
{
    const uint32_t plane = (uint32_t)h * (uint32_t)w;
    const int tiles_x = (w + WS_TILE - 1) / WS_TILE, tiles_y = (h + WS_TILE - 1) / WS_TILE;
    const int tiles = tiles_x * tiles_y;                                        // (<= h w)
    for (int tile = blockIdx.x; tile < tiles; tile += WS_BLOCKS) {
        const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
        if (VEC) {
            const int x = tx * WS_TILE + 4 * ((int)threadIdx.x & 7), y = ty * WS_TILE + ((int)threadIdx.x >> 3);
            if (x >= w || y >= h) continue;                                     // (w % 4 == 0: x < w means x + 3 < w)
            Tap t[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = make_tap(inv, x + j, y, h, w);
            const uint32_t at = (uint32_t)y * (uint32_t)w + (uint32_t)x;
#pragma unroll
            for (uint32_t c = 0; c < 3; ++c) {
                const float *__restrict__ p = s + c * plane;
                rn::f32x4 o;
                o.x = tap_sample(p, t[0]);
                o.y = tap_sample(p, t[1]);
                o.z = tap_sample(p, t[2]);
                o.w = tap_sample(p, t[3]);
                *(rn::f32x4 *)(d + c * plane + at) = o;
            }
        } else {
            const int x = tx * WS_TILE + ((int)threadIdx.x & 31);
            if (x >= w) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int y = ty * WS_TILE + ((int)threadIdx.x >> 5) + 8 * j;
                if (y >= h) break;
                const Tap t = make_tap(inv, x, y, h, w);
                const uint32_t at = (uint32_t)y * (uint32_t)w + (uint32_t)x;
#pragma unroll
                for (uint32_t c = 0; c < 3; ++c) d[c * plane + at] = tap_sample(s + c * plane, t);
            }
        }
    }
}

__global__ __launch_bounds__(WS_BLOCK) void image_warp_stage_kernel(const float *__restrict__ arena, const int64_t slot,
                                                                   const int32_t *__restrict__ in_hw, const rn_affine_coef *__restrict__ coef,
                                                                   float *__restrict__ arena_out, const int64_t slot_out)
{
    const int b = blockIdx.y;
    const int h = in_hw[2 * b], w = in_hw[2 * b + 1];
    if (h < 1 || w < 1 || (int64_t)h * w > slot / 3 || (int64_t)h * w > slot_out / 3) return;       // (device data: an image no slot can hold)
    const float *__restrict__ s = arena + (int64_t)b * slot;
    float *__restrict__ d = arena_out + (int64_t)b * slot_out;
    if (coef[b].applied == 0) {
        // left alone: the 3 h w floats bit for bit (loads and stores only), 16 bytes at a time where both slots allow
        const uint32_t n = 3u * (uint32_t)h * (uint32_t)w;                      // <= slot < 2^31
        const uint32_t tid = blockIdx.x * WS_BLOCK + threadIdx.x, step = WS_BLOCKS * WS_BLOCK;
        const uint32_t n4 = ((((uintptr_t)d) | ((uintptr_t)s)) & 15) == 0 ? n >> 2 : 0;
        for (uint32_t v = tid; v < n4; v += step) ((rn::u32x4 *)d)[v] = ((const rn::u32x4 *)s)[v];
        for (uint32_t e = 4u * n4 + tid; e < n; e += step) ((uint32_t *)d)[e] = ((const uint32_t *)s)[e];
        return;
    }
    float inv[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) inv[k] = coef[b].inv[k];
    if ((w & 3) == 0 && (((uintptr_t)d) & 15) == 0)
        warp_tiles<true>(s, d, h, w, inv);
    else
        warp_tiles<false>(s, d, h, w, inv);
}

}  // namespace

RN_API int rn_affine_draw(rn_affine_state *state, const float *gt_boxes, const int64_t *gt_labels, const int32_t *gt_off, const int32_t *in_hw_dev,
                          int B, rn_affine_coef *coef, float *out_boxes, int64_t *out_labels, int32_t *out_gt_off, int64_t rows, void *stream)
{
    if (!state || !gt_off || !in_hw_dev || !coef || !out_gt_off || gt_off == out_gt_off || B <= 0 || B > 65535 || rows < 0 || rows > INT32_MAX)
        return RN_EINVAL;
    if (rows > 0 && (!gt_boxes || !out_boxes || !gt_labels || !out_labels || gt_boxes == out_boxes || gt_labels == out_labels)) return RN_EINVAL;
    if (!rn::aligned(state, 8) || !rn::aligned(gt_off, 4) || !rn::aligned(in_hw_dev, 4) || !rn::aligned(coef, 4) || !rn::aligned(out_gt_off, 4) ||
        !rn::aligned(gt_boxes, 16) || !rn::aligned(out_boxes, 16) || !rn::aligned(gt_labels, 8) || !rn::aligned(out_labels, 8))
        return RN_EALIGN;
    hipLaunchKernelGGL(affine_coef_kernel, dim3((unsigned)B), dim3(AF_WAVE), 0, (hipStream_t)stream, state, (const rn::f32x4 *)gt_boxes, gt_off,
                       in_hw_dev, coef, (int32_t)rows);
    hipLaunchKernelGGL(affine_rows_kernel, dim3((unsigned)B), dim3(AF_WAVE), 0, (hipStream_t)stream, state, (const rn::f32x4 *)gt_boxes, gt_labels,
                       gt_off, in_hw_dev, coef, B, (rn::f32x4 *)out_boxes, out_labels, out_gt_off, (int32_t)rows);
    hipLaunchKernelGGL(draw_advance_kernel, dim3(1), dim3(DRAW_ADVANCE_BLOCK), 0, (hipStream_t)stream, &state->counter);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

RN_API int rn_image_warp_stage(const float *arena, int64_t slot, const int32_t *in_hw_dev, const rn_affine_coef *coef, int B, float *arena_out,
                               int64_t slot_out, void *stream)
{
    if (!arena || !in_hw_dev || !coef || !arena_out || arena == arena_out || B <= 0 || B > 65535) return RN_EINVAL;
    if (slot < 3 || slot_out < 3 || slot > INT32_MAX || slot_out > INT32_MAX) return RN_EINVAL;      // (the kernel indexes a slot with 32 bits)
    if (!rn::aligned(arena, 4) || !rn::aligned(arena_out, 4) || !rn::aligned(in_hw_dev, 4) || !rn::aligned(coef, 4)) return RN_EALIGN;
    hipLaunchKernelGGL(image_warp_stage_kernel, dim3(WS_BLOCKS, (unsigned)B), dim3(WS_BLOCK), 0, (hipStream_t)stream, arena, slot, in_hw_dev,
                       coef, arena_out, slot_out);
    RN_LAUNCH_CHECK();
    return RN_OK;
}
