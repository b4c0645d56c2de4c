// Train-time augmentation decisions drawn on the device (augment.RandomHorizontalFlip, augment.RandomShortSide).
//
// The reference's only training augmentation is a random horizontal flip with p = 0.5 (hparams.yaml transforms,
// albumentations.HorizontalFlip; RandomHorizontalFlip(prob=0.5) for COCO), decided per image on the host.  Here the decision is
// made by ONE tiny launch inside the train step, so a replayed hipGraph draws new flips at every replay without a host round trip:
//
//   rn_hflip_draw   flags[b] = u(seed, counter, b) < p for b < B, then counter += 1
//
// seed, counter and p live in a device block (rn_hflip_state) that the host writes outside any capture; changing p or the seed
// needs no re-capture.  u is a counter-based hash (splitmix64's finalizer) mapped to [0, 1) with 24 bits:
//
//   z  = seed ^ (counter * 0x9E3779B97F4A7C15) ^ ((b + 1) * 0xD1B54A32D192ED03)      (all mod 2^64)
//   z  = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
//   z  = (z ^ (z >> 27)) * 0x94D049BB133111EB
//   z ^= z >> 31
//   u  = (z >> 40) * 2^-24                                                            (exact in fp32)
//
// and the comparison is in fp32, so p = 0 never flips and p = 1 always does.  augment.RandomHorizontalFlip.draw restates this in
// Python.  The kernel is one wave: every lane reads the block (one uniform load), lane 0 writes counter + 1 with an ordinary
// global store after that read, which its value depends on.
//
// Multi-scale training (torchvision's min_size tuple: one short side per image and step) is drawn the same way, so that ONE captured
// graph serves every scale over a fixed canvas:
//
//   rn_short_side_draw   out_hw[b], ratios[b] for b < B from u(seed ^ salt, counter, b), then counter += 1
//
// with the block rn_short_side_state (seed, counter, n, sizes[16]):
//
//   idx   = min(int(u * n), n - 1)                      (u has 24 bits and n <= 16: u * n is exact in fp32)
//   short = sizes[idx]
//   scale = short / min(h, w);  if (max(h, w) * scale > max_size) scale = max_size / max(h, w)          (double, this order)
//   nh    = floor(h * scale),  nw = floor(w * scale)                                                    (double)
//   rh    = float(nh) / float(h),  rw = float(nw) / float(w)                                            (fp32, correctly rounded)
//
// i.e. transform.GeneralizedRCNNTransform._scale_for, the two floors of its resize and transform._ratios; this file is built without
// FMA contraction and with IEEE division.  The salt keeps a flip and a jitter that share a seed from tying small sizes to flipped
// images.  The input sizes are host values carried in the kernel arguments (64 images per launch; lane i serves image i); a batch
// of more than 64 images takes several launches that read the SAME counter, and only the last one advances it.
//
//   rn_resize_plan_dev   the same plan with h, w read from DEVICE memory (in_hw i32[B][2], written by rn_image_stage: the image
//                        capacity mode of graph.CapturedTrainStep), so a captured step serves images of any size
//
// With a state block the draw is rn_short_side_draw's: same hash, salt and counter advance (augment.RandomShortSide.draw restates
// both).  With a null block the short side is a value passed by the host (a transform without multi-scale training) and nothing
// is drawn.  No table in the kernel arguments: one wave walks the images 64 at a time, so one launch serves any B.  A size < 1
// (device data) gives out_hw = (0, 0) and ratios (0, 0): the transform kernel treats such an image as all padding.
//
// Colour jitter (augment.ColorJitter: torchvision's ColorJitter on fp32 RGB in [0, 1]) is drawn the same way once more:
//
//   rn_color_jitter_draw   coef[b] = {four factors, mean = 0, order} for b < B, then counter += 1
//
// with the block rn_color_jitter_state (seed, counter, p, lo[4], hi[4], enabled_mask) and six salts, one per uniform:
//
//   applied = u_apply < p                                                               (fp32 compare)
//   order   = the min(int(u_order * 24), 23)-th permutation of (brightness, contrast, saturation, hue) in lexicographic order, as
//             four nibbles; a disabled operation's nibble is 0xF, and so is every nibble of an image that is not applied
//   f[k]    = lo[k] + u_k * (hi[k] - lo[k])                                             (fp32, this order; drawn whatever ``applied``)
//
// The operations themselves run inside the transform kernel (transform.hip, rn_color.hpp).  The one thing that is not per-pixel is
// the contrast's mean gray, taken over the image as it is when the contrast's turn comes:
//
//   rn_color_mean   coef[b].mean = float(sum_pixels double(gray(pre(pixel))) / double(h w)) for the images whose order holds a contrast
//
// pre = the operations before the contrast, by the helper the transform kernel calls.  No atomics: 32 blocks per image, thread t of
// block k adds the pixels k * 256 + t + j * 8192 in order of j, the block adds its 256 sums as a fixed tree, and a second single-wave
// launch adds an image's 32 partials in index order -- two calls give the same bits.
//
// Brightness / contrast (augment.RandomBrightnessContrast: albumentations' alpha x + beta ref on fp32 RGB in [0, 1]) rides in the same
// rows, behind the four operations (the numbered rule in include/retinanet_hip.h):
//
//   rn_brightness_contrast_draw   coef[b].bc_mul = alpha, .bc_add = beta, order bits 16 (present) and 17 (mean pending); counter += 1
//   rn_brightness_contrast_mean   for the rows with bit 17: bc_add = beta * float(sum of double(every channel value) / double(3 h w)),
//                                 the values taken after the row's colour operations; bit 17 cleared
//
// with rn_color_mean's structure: the same blocks, the same order of every sum, the same single-wave finish.
//
// The bbox-safe random crop (augment.BBoxSafeRandomCrop: albumentations' BBoxSafeRandomCrop with erosion_rate = 0 in intent, on integer
// pixels) is a second staging pass over staged images and packed GT (the image capacity mode), so nothing downstream changes:
//
//   rn_bbox_crop_draw     rect[b] = (y0, x0, ch, cw), crop_hw[b] = (ch, cw), out_boxes = the boxes shifted by (x0, y0); then counter += 1
//   rn_image_crop_stage   image b's window [3][ch][cw] of arena slot b, dense, to the start of slot b of a second arena
//
// The draw is one wave per image: the lanes walk the image's rows, the union of the boxes is a wave reduction (no atomics), every lane
// then computes the same rectangle (the numbered rule in include/retinanet_hip.h; augment.BBoxSafeRandomCrop.draw_rects restates it) and
// the lanes write the shifted rows.  Every wave reads the counter, so it is advanced by a single-wave launch of its own behind the
// draw (draw_advance_kernel, rn_draw.hpp).  The copy is a bandwidth kernel with a fixed grid (CS_BLOCKS blocks per image): a thread gathers four consecutive floats of the
// dense destination -- the source rows start at x0 and are only 4-byte aligned, so they are read as four 4-byte loads, which the lanes
// of a wave still coalesce -- and writes them as one 16-byte store when the destination slot is 16-byte aligned.
#include "rn_color.hpp"
#include "rn_common.hpp"
#include <stddef.h>

#include "rn_draw.hpp"              // hflip_u: the hash stated above, and draw_advance_kernel, shared with affine.hip

namespace {

constexpr int HF_BLOCK = 64;        // one wave: the counter update needs no barrier across waves

// (every static_assert on a state struct below: the Python side packs the block by these offsets -- draw_state.py's layout table --
// so a struct edit that the table does not follow fails the build)
static_assert(sizeof(rn_hflip_state) == 24 && offsetof(rn_hflip_state, seed) == 0 && offsetof(rn_hflip_state, counter) == 8 &&
                  offsetof(rn_hflip_state, p) == 16, "draw_state.HFLIP");

__global__ __launch_bounds__(HF_BLOCK) void hflip_draw_kernel(rn_hflip_state *st, const int B, uint8_t *__restrict__ flags)
{
    const uint64_t seed = st->seed;
    const int64_t counter = st->counter;
    const float p = st->p;
    for (int b = (int)threadIdx.x; b < B; b += HF_BLOCK) flags[b] = hflip_u(seed, counter, b) < p ? 1 : 0;
    if (threadIdx.x == 0) st->counter = counter + 1;
}

constexpr int SS_MAX_IMAGES = 64;   // per launch (kernel-argument table): one lane per image
constexpr uint64_t SS_SALT = 0x5CA1E5CA1E5CA1E5ull;
static_assert(SS_MAX_IMAGES == HF_BLOCK, "one lane per image of a launch");

// The plan of ONE image, shared by the two kernels below so that they cannot drift apart: _scale_for, the two floors of resize and
// _ratios for an h x w image (both >= 1) and the short side ``shrt``, written to entry b of out_hw / ratios.
__device__ __forceinline__ void resize_plan(const int h, const int w, const int shrt, const int max_size, const int b,
                                            int32_t *__restrict__ out_hw, float *__restrict__ ratios)
{
    const double lo = (double)(h < w ? h : w), hi = (double)(h < w ? w : h);
    double scale = (double)shrt / lo;
    if (hi * scale > (double)max_size) scale = (double)max_size / hi;
    const int nh = (int)floor((double)h * scale), nw = (int)floor((double)w * scale);
    out_hw[2 * b] = nh;
    out_hw[2 * b + 1] = nw;
    ratios[2 * b] = (float)nh / (float)h;
    ratios[2 * b + 1] = (float)nw / (float)w;
}

struct ShortSideTable { int32_t ih[SS_MAX_IMAGES], iw[SS_MAX_IMAGES]; };

// (the layout's ``sizes`` field is n, the reserved word and the 16 entries: bytes 16..88)
static_assert(sizeof(rn_short_side_state) == 24 + 4 * RN_SHORT_SIDE_MAX && RN_SHORT_SIDE_MAX == 16 && offsetof(rn_short_side_state, seed) == 0 &&
                  offsetof(rn_short_side_state, counter) == 8 && offsetof(rn_short_side_state, n) == 16 &&
                  offsetof(rn_short_side_state, reserved) == 20 && offsetof(rn_short_side_state, sizes) == 24, "draw_state.SHORT_SIDE");

__global__ __launch_bounds__(HF_BLOCK) void short_side_draw_kernel(rn_short_side_state *st, const ShortSideTable t, const int cnt, const int base,
                                                                  const int max_size, const int advance, int32_t *__restrict__ out_hw,
                                                                  float *__restrict__ ratios)
{
    const uint64_t seed = st->seed ^ SS_SALT;
    const int64_t counter = st->counter;
    int n = st->n;
    n = n < 1 ? 1 : (n > RN_SHORT_SIDE_MAX ? RN_SHORT_SIDE_MAX : n);          // (device data: the index below stays inside sizes[])
    const int i = (int)threadIdx.x;
    if (i < cnt) {
        const int b = base + i;
        int idx = (int)(hflip_u(seed, counter, b) * (float)n);
        idx = idx < n - 1 ? idx : n - 1;
        resize_plan(t.ih[i], t.iw[i], st->sizes[idx], max_size, b, out_hw, ratios);
    }
    if (advance && threadIdx.x == 0) st->counter = counter + 1;
}

// DRAW: short side from the state block (and the counter advanced), else ``fixed_short``; st is null without DRAW
template <bool DRAW>
__global__ __launch_bounds__(HF_BLOCK) void resize_plan_dev_kernel(rn_short_side_state *st, const int32_t *__restrict__ in_hw, const int fixed_short,
                                                                  const int max_size, const int B, int32_t *__restrict__ out_hw,
                                                                  float *__restrict__ ratios)
{
    uint64_t seed = 0;
    int64_t counter = 0;
    int n = 1;
    if (DRAW) {
        seed = st->seed ^ SS_SALT;
        counter = st->counter;
        n = st->n;
        n = n < 1 ? 1 : (n > RN_SHORT_SIDE_MAX ? RN_SHORT_SIDE_MAX : n);      // (device data: the index below stays inside sizes[])
    }
    for (int b = (int)threadIdx.x; b < B; b += HF_BLOCK) {
        int shrt = fixed_short;
        if (DRAW) {
            int idx = (int)(hflip_u(seed, counter, b) * (float)n);
            idx = idx < n - 1 ? idx : n - 1;
            shrt = st->sizes[idx];
        }
        const int h = in_hw[2 * b], w = in_hw[2 * b + 1];
        if (h >= 1 && w >= 1) {
            resize_plan(h, w, shrt, max_size, b, out_hw, ratios);
        } else {                                                               // (device data: an empty entry, nothing is divided)
            out_hw[2 * b] = out_hw[2 * b + 1] = 0;
            ratios[2 * b] = ratios[2 * b + 1] = 0.0f;
        }
    }
    // (one wave: every lane read the counter above, in program order before this store)
    if (DRAW && threadIdx.x == 0) st->counter = counter + 1;
}

// ---- colour jitter: the draw and the contrast mean (augment.ColorJitter) -------------------------------------------------------------
constexpr uint64_t CJ_SALT_APPLY = 0xC0104A11C0104A11ull, CJ_SALT_ORDER = 0x04DE404DE404DE45ull;
constexpr uint64_t CJ_SALT_F0 = 0xB416B416B416B417ull, CJ_SALT_F1 = 0xC0274A57C0274A57ull, CJ_SALT_F2 = 0x5A7C5A7C5A7C5A7Dull,
                   CJ_SALT_F3 = 0x40E040E040E040E1ull;

// the idx-th permutation of (0, 1, 2, 3) in lexicographic order as four nibbles (nibble k = the k-th element), ids outside ``mask`` -> 0xF
__device__ __forceinline__ int color_order(int idx, const int mask)
{
    int avail = 0x3210, order = 0;      // the ids not yet placed, ascending
    const int div[4] = {6, 2, 1, 1};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int d = idx / div[k];     // which of the remaining ids comes next (0 at k = 3: idx is 0 by then)
        idx -= d * div[k];
        const int id = (avail >> (4 * d)) & 0xF;
        avail = (avail & ((1 << (4 * d)) - 1)) | ((avail >> (4 * d + 4)) << (4 * d));
        order |= (((mask >> id) & 1) ? id : rn::COLOR_SKIP) << (4 * k);
    }
    return order;
}

static_assert(sizeof(rn_color_jitter_state) == 56 && offsetof(rn_color_jitter_state, seed) == 0 && offsetof(rn_color_jitter_state, counter) == 8 &&
                  offsetof(rn_color_jitter_state, p) == 16 && offsetof(rn_color_jitter_state, lo) == 20 && offsetof(rn_color_jitter_state, hi) == 36 &&
                  offsetof(rn_color_jitter_state, enabled_mask) == 52, "draw_state.COLOR_JITTER");

__global__ __launch_bounds__(HF_BLOCK) void color_jitter_draw_kernel(rn_color_jitter_state *st, const int B, rn_color_coef *__restrict__ coef)
{
    const uint64_t seed = st->seed;
    const int64_t counter = st->counter;
    const float p = st->p;
    const int mask = st->enabled_mask & 0xF;
    float lo[4], hi[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { lo[k] = st->lo[k]; hi[k] = st->hi[k]; }
    const uint64_t salt[4] = {CJ_SALT_F0, CJ_SALT_F1, CJ_SALT_F2, CJ_SALT_F3};
    for (int b = (int)threadIdx.x; b < B; b += HF_BLOCK) {
        rn_color_coef c;
        const bool applied = hflip_u(seed ^ CJ_SALT_APPLY, counter, b) < p;
        int idx = (int)(hflip_u(seed ^ CJ_SALT_ORDER, counter, b) * 24.0f);
        idx = idx < 23 ? idx : 23;
        c.order = applied ? color_order(idx, mask) : 0xFFFF;
#pragma unroll
        for (int k = 0; k < 4; ++k) c.f[k] = lo[k] + hflip_u(seed ^ salt[k], counter, b) * (hi[k] - lo[k]);
        c.mean = 0.0f;
        c.bc_mul = c.bc_add = 0.0f;                                      // (no brightness / contrast: the two words stay zero bits)
        coef[b] = c;
    }
    // (one wave: every lane read the counter above, in program order before this store)
    if (threadIdx.x == 0) st->counter = counter + 1;
}

constexpr int CM_MAX_IMAGES = 64;   // per launch (kernel-argument table)
constexpr int CM_BLOCKS = 32;       // blocks per image: fixed, so the order of every sum is
constexpr int CM_BLOCK = 256;

struct ColorMeanArgs {
    const float *img[CM_MAX_IMAGES];   // [3][h][w] f32, contiguous
    int32_t ih[CM_MAX_IMAGES], iw[CM_MAX_IMAGES];
    const float *arena;                // VAR: this launch's first image's slot (device); img / ih / iw above are unused
    const int32_t *in_hw;              // VAR: this launch's first image's (ih, iw) (device)
    int64_t slot;                      // VAR: floats per slot
    rn_color_coef *coef;               // this launch's first image
    double *partial;                   // this launch's first image: [image][CM_BLOCKS]
};

// (ih, iw) of image b of the launch; false: an image no slot can hold (device data) -- the guards of transform_batch_kernel<VAR>
template <bool VAR>
__device__ __forceinline__ bool color_mean_size(const ColorMeanArgs &a, const int b, int &ih, int &iw)
{
    ih = VAR ? a.in_hw[2 * b] : a.ih[b];
    iw = VAR ? a.in_hw[2 * b + 1] : a.iw[b];
    return !(VAR && (ih < 1 || iw < 1 || (int64_t)ih * iw > a.slot / 3));
}

// partial[b][blockIdx.x] = the sum in double, in a fixed order, of gray(pre(pixel)) over the pixels blockIdx.x * 256 + t + j * 8192
template <bool VAR>
__global__ __launch_bounds__(CM_BLOCK) void color_mean_partial_kernel(const ColorMeanArgs a)
{
    __shared__ double sums[CM_BLOCK];
    const int b = blockIdx.y;
    const rn_color_coef c = a.coef[b];
    if (!rn::color_has_contrast(c.order)) return;
    int ih, iw;
    const bool fits = color_mean_size<VAR>(a, b, ih, iw);
    double acc = 0.0;
    if (fits) {
        const float *__restrict__ src = VAR ? a.arena + (int64_t)b * a.slot : a.img[b];
        const int64_t plane = (int64_t)ih * iw;
        for (int64_t i = (int64_t)blockIdx.x * CM_BLOCK + threadIdx.x; i < plane; i += (int64_t)CM_BLOCKS * CM_BLOCK) {
            float r = src[i], g = src[plane + i], bl = src[2 * plane + i];
            rn::color_apply<true>(r, g, bl, c);
            acc += (double)rn::color_gray(r, g, bl);
        }
    }
    sums[threadIdx.x] = acc;
    __syncthreads();
    for (int s = CM_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sums[threadIdx.x] += sums[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.partial[(int64_t)b * CM_BLOCKS + blockIdx.x] = sums[0];
}

// lane i: image i of the launch -- its partials added in index order, mean = float(sum / double(h w)); 0 for an image no slot holds
template <bool VAR>
__global__ __launch_bounds__(HF_BLOCK) void color_mean_finish_kernel(const ColorMeanArgs a, const int cnt)
{
    const int b = (int)threadIdx.x;
    if (b >= cnt) return;
    if (!rn::color_has_contrast(a.coef[b].order)) return;
    int ih, iw;
    if (!color_mean_size<VAR>(a, b, ih, iw)) { a.coef[b].mean = 0.0f; return; }
    double sum = 0.0;
    for (int k = 0; k < CM_BLOCKS; ++k) sum += a.partial[(int64_t)b * CM_BLOCKS + k];
    a.coef[b].mean = (float)(sum / (double)((int64_t)ih * iw));
}

// ---- brightness / contrast: the draw and the image mean (augment.RandomBrightnessContrast) -------------------------------------------
constexpr uint64_t RB_SALT_APPLY = 0xB7C0A991B7C0A991ull, RB_SALT_CONTRAST = 0xC0A7C0A7C0A7C0A7ull, RB_SALT_BRIGHTNESS = 0xB419B419B419B419ull;

static_assert(sizeof(rn_brightness_contrast_state) == 40 && offsetof(rn_brightness_contrast_state, seed) == 0 &&
                  offsetof(rn_brightness_contrast_state, counter) == 8 && offsetof(rn_brightness_contrast_state, p) == 16 &&
                  offsetof(rn_brightness_contrast_state, blo) == 20 && offsetof(rn_brightness_contrast_state, bhi) == 24 &&
                  offsetof(rn_brightness_contrast_state, clo) == 28 && offsetof(rn_brightness_contrast_state, chi) == 32 &&
                  offsetof(rn_brightness_contrast_state, by_max) == 36, "draw_state.BRIGHTNESS_CONTRAST");
static_assert(sizeof(rn_color_coef) == 32 && offsetof(rn_color_coef, order) == 20 && offsetof(rn_color_coef, bc_mul) == 24 &&
                  offsetof(rn_color_coef, bc_add) == 28, "rn_color_coef: ops.COLOR_COEF_FLOATS and the columns the Python side reads");

// fresh: no colour jitter wrote the rows -- each is made the identity first; else its six colour words stay as they are
__global__ __launch_bounds__(HF_BLOCK) void brightness_contrast_draw_kernel(rn_brightness_contrast_state *st, const int B,
                                                                           rn_color_coef *__restrict__ coef, const int fresh)
{
    const uint64_t seed = st->seed;
    const int64_t counter = st->counter;
    const float p = st->p, blo = st->blo, bhi = st->bhi, clo = st->clo, chi = st->chi;
    const int pending = st->by_max != 0 ? 0 : rn::COLOR_BC_PENDING;
    for (int b = (int)threadIdx.x; b < B; b += HF_BLOCK) {
        rn_color_coef c;
        if (fresh) {
            c.f[0] = c.f[1] = c.f[2] = 1.0f;
            c.f[3] = 0.0f;
            c.mean = 0.0f;
            c.order = 0xFFFF;
        } else {
            c = coef[b];
        }
        const bool applied = hflip_u(seed ^ RB_SALT_APPLY, counter, b) < p;
        const float alpha = 1.0f + (clo + hflip_u(seed ^ RB_SALT_CONTRAST, counter, b) * (chi - clo));
        const float beta = blo + hflip_u(seed ^ RB_SALT_BRIGHTNESS, counter, b) * (bhi - blo);
        c.order = (c.order & ~(rn::COLOR_BC_PRESENT | rn::COLOR_BC_PENDING)) | (applied ? (rn::COLOR_BC_PRESENT | pending) : 0);
        c.bc_mul = applied ? alpha : 1.0f;
        c.bc_add = applied ? beta : 0.0f;
        coef[b] = c;
    }
    // (one wave: every lane read the counter above, in program order before this store)
    if (threadIdx.x == 0) st->counter = counter + 1;
}

// partial[b][blockIdx.x] = the sum in double, in a fixed order, of the three channel values after the colour operations over the pixels
// blockIdx.x * 256 + t + j * 8192, for the rows whose image mean is pending
template <bool VAR>
__global__ __launch_bounds__(CM_BLOCK) void bc_mean_partial_kernel(const ColorMeanArgs a)
{
    __shared__ double sums[CM_BLOCK];
    const int b = blockIdx.y;
    rn_color_coef c = a.coef[b];
    if (!(c.order & rn::COLOR_BC_PENDING)) return;
    c.order &= 0xFFFF;                                                          // (the operations that come before this one)
    int ih, iw;
    const bool fits = color_mean_size<VAR>(a, b, ih, iw);
    double acc = 0.0;
    if (fits) {
        const float *__restrict__ src = VAR ? a.arena + (int64_t)b * a.slot : a.img[b];
        const int64_t plane = (int64_t)ih * iw;
        for (int64_t i = (int64_t)blockIdx.x * CM_BLOCK + threadIdx.x; i < plane; i += (int64_t)CM_BLOCKS * CM_BLOCK) {
            float r = src[i], g = src[plane + i], bl = src[2 * plane + i];
            rn::color_apply<false>(r, g, bl, c);
            acc += ((double)r + (double)g) + (double)bl;
        }
    }
    sums[threadIdx.x] = acc;
    __syncthreads();
    for (int s = CM_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sums[threadIdx.x] += sums[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.partial[(int64_t)b * CM_BLOCKS + blockIdx.x] = sums[0];
}

// lane i: image i of the launch -- ref = float(its partials added in index order / double(3 h w)), 0 for an image no slot holds;
// bc_add = beta * ref and the pending bit cleared, so a second call finds nothing to do
template <bool VAR>
__global__ __launch_bounds__(HF_BLOCK) void bc_mean_finish_kernel(const ColorMeanArgs a, float *__restrict__ ref_out, const int cnt)
{
    const int b = (int)threadIdx.x;
    if (b >= cnt) return;
    const int order = a.coef[b].order;
    if (!(order & rn::COLOR_BC_PENDING)) return;
    int ih, iw;
    float ref = 0.0f;
    if (color_mean_size<VAR>(a, b, ih, iw)) {
        double sum = 0.0;
        for (int k = 0; k < CM_BLOCKS; ++k) sum += a.partial[(int64_t)b * CM_BLOCKS + k];
        ref = (float)(sum / (double)(3 * (int64_t)ih * iw));
    }
    ref_out[b] = ref;
    a.coef[b].bc_add = a.coef[b].bc_add * ref;
    a.coef[b].order = order & ~rn::COLOR_BC_PENDING;
}

// ---- bbox-safe random crop: the draw and the copy (augment.BBoxSafeRandomCrop) ---------------------------------------------------------
constexpr uint64_t BC_SALT_APPLY = 0xC409C409C409C40Bull, BC_SALT_LEFT = 0x1EF71EF71EF71EF7ull, BC_SALT_TOP = 0x70B070B070B070B1ull,
                   BC_SALT_RIGHT = 0x4167416741674169ull, BC_SALT_BOTTOM = 0xB077B077B077B079ull;

// int(f) for a finite f, saturating (a box far outside the image must not leave the conversion undefined)
__device__ __forceinline__ int sat_int(const float f)
{
    return f <= -2147483648.0f ? INT32_MIN : (f >= 2147483648.0f ? INT32_MAX : (int)f);
}

__device__ __forceinline__ int clamp_int(const int v, const int lo, const int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the start and the end of the crop on one axis of length n: the margins before the union [u1, u2) and behind it, each drawn uniformly
__device__ __forceinline__ void crop_axis(const float u_lo, const float u_hi, const int u1, const int u2, const int n, int &start, int &end)
{
    const int a = (int)(u_lo * (float)(u1 + 1)), c = (int)(u_hi * (float)(n - u2 + 1));
    start = a < u1 ? a : u1;
    end = u2 + (c < n - u2 ? c : n - u2);
}

static_assert(sizeof(rn_bbox_crop_state) == 24 && offsetof(rn_bbox_crop_state, seed) == 0 && offsetof(rn_bbox_crop_state, counter) == 8 &&
                  offsetof(rn_bbox_crop_state, p) == 16, "draw_state.BBOX_CROP");

// one wave per image (blockIdx.x); the state block is only read here
__global__ __launch_bounds__(HF_BLOCK) void bbox_crop_draw_kernel(const rn_bbox_crop_state *__restrict__ st, const rn::f32x4 *__restrict__ in,
                                                                 const int32_t *__restrict__ gt_off, const int32_t *__restrict__ in_hw,
                                                                 int32_t *__restrict__ rect, int32_t *__restrict__ crop_hw,
                                                                 rn::f32x4 *__restrict__ out, const int32_t rows)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const uint64_t seed = st->seed;
    const int64_t counter = st->counter;
    const float p = st->p;
    const int h = in_hw[2 * b], w = in_hw[2 * b + 1];
    int32_t lo = gt_off[b], hi = gt_off[b + 1];
    lo = lo < 0 ? 0 : (lo > rows ? rows : lo);                                  // (device data: the rows stay inside the buffers)
    hi = hi < lo ? lo : (hi > rows ? rows : hi);
    // the union of the boxes: min x1, min y1, max x2, max y2; a NaN anywhere among them makes its extreme NaN
    float mx1 = INFINITY, my1 = INFINITY, mx2 = -INFINITY, my2 = -INFINITY;
    int nan = 0;
    for (int32_t r = lo + lane; r < hi; r += HF_BLOCK) {
        const rn::f32x4 v = in[r];
        nan |= (v.x != v.x) | (v.y != v.y) | (v.z != v.z) | (v.w != v.w);
        mx1 = fminf(mx1, v.x);
        my1 = fminf(my1, v.y);
        mx2 = fmaxf(mx2, v.z);
        my2 = fmaxf(my2, v.w);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mx1 = fminf(mx1, __shfl_xor(mx1, o, RN_WAVE));
        my1 = fminf(my1, __shfl_xor(my1, o, RN_WAVE));
        mx2 = fmaxf(mx2, __shfl_xor(mx2, o, RN_WAVE));
        my2 = fmaxf(my2, __shfl_xor(my2, o, RN_WAVE));
        nan |= __shfl_xor(nan, o, RN_WAVE);
    }
    const bool empty = h < 1 || w < 1;
    const bool finite = !nan && isfinite(mx1) && isfinite(my1) && isfinite(mx2) && isfinite(my2);
    const bool crop = hi > lo && hflip_u(seed ^ BC_SALT_APPLY, counter, b) < p && !empty && finite;
    int y0 = 0, x0 = 0, ch = empty ? 0 : h, cw = empty ? 0 : w;
    if (crop) {
        const int ux1 = clamp_int(sat_int(floorf(mx1)), 0, w - 1), uy1 = clamp_int(sat_int(floorf(my1)), 0, h - 1);
        const int ux2 = clamp_int(sat_int(ceilf(mx2)), ux1 + 1, w), uy2 = clamp_int(sat_int(ceilf(my2)), uy1 + 1, h);
        int xe, ye;
        crop_axis(hflip_u(seed ^ BC_SALT_LEFT, counter, b), hflip_u(seed ^ BC_SALT_RIGHT, counter, b), ux1, ux2, w, x0, xe);
        crop_axis(hflip_u(seed ^ BC_SALT_TOP, counter, b), hflip_u(seed ^ BC_SALT_BOTTOM, counter, b), uy1, uy2, h, y0, ye);
        cw = xe - x0;
        ch = ye - y0;
        // the orientation is kept: the short axis of the crop is widened around its middle, inside the image
        if (h <= w && ch > cw) {
            const int s = x0 - (ch - cw) / 2, m = w - ch;
            x0 = s < m ? s : m;
            x0 = x0 > 0 ? x0 : 0;
            cw = ch;
        } else if (h > w && cw > ch) {
            const int s = y0 - (cw - ch) / 2, m = h - cw;
            y0 = s < m ? s : m;
            y0 = y0 > 0 ? y0 : 0;
            ch = cw;
        }
    }
    if (lane == 0) {
        rect[4 * b] = y0;
        rect[4 * b + 1] = x0;
        rect[4 * b + 2] = ch;
        rect[4 * b + 3] = cw;
        crop_hw[2 * b] = ch;
        crop_hw[2 * b + 1] = cw;
    }
    const float fx = (float)x0, fy = (float)y0;
    for (int32_t r = lo + lane; r < hi; r += HF_BLOCK) {
        rn::f32x4 v = in[r];
        if (crop) {                                                             // (else copied bit for bit)
            v.x -= fx;
            v.y -= fy;
            v.z -= fx;
            v.w -= fy;
        }
        out[r] = v;
    }
}

constexpr int CS_BLOCKS = 256;      // blocks per image: fixed, so neither the grid nor an argument depends on a size
constexpr int CS_BLOCK = 256;

// source index of destination element e of a [3][ch][cw] window at (y0, x0) of a [3][h][w] image (all < 2^31: the host checked the slots)
struct CropGeom { uint32_t y0, x0, ch, cw, w, plane_s, plane_d; };

__device__ __forceinline__ void crop_split(const CropGeom &g, const uint32_t e, uint32_t &c, uint32_t &y, uint32_t &x)
{
    c = e / g.plane_d;
    const uint32_t r = e - c * g.plane_d;
    y = r / g.cw;
    x = r - y * g.cw;
}

__global__ __launch_bounds__(CS_BLOCK) void image_crop_stage_kernel(const float *__restrict__ arena, const int64_t slot,
                                                                   const int32_t *__restrict__ in_hw, const int32_t *__restrict__ rect,
                                                                   float *__restrict__ arena_out, const int64_t slot_out)
{
    const int b = blockIdx.y;
    const int h = in_hw[2 * b], w = in_hw[2 * b + 1];
    if (h < 1 || w < 1 || (int64_t)h * w > slot / 3) return;                    // (device data: an image no slot can hold)
    // the rectangle re-clamped to the image: whatever rect holds, no thread leaves the source slot
    const int y0 = clamp_int(rect[4 * b], 0, h - 1), x0 = clamp_int(rect[4 * b + 1], 0, w - 1);
    int ch = rect[4 * b + 2], cw = rect[4 * b + 3];
    ch = ch < h - y0 ? ch : h - y0;
    cw = cw < w - x0 ? cw : w - x0;
    if (ch < 1 || cw < 1 || (int64_t)ch * cw > slot_out / 3) return;            // (nor the destination slot)
    const float *__restrict__ s = arena + (int64_t)b * slot;
    float *__restrict__ d = arena_out + (int64_t)b * slot_out;
    CropGeom g;
    g.y0 = (uint32_t)y0; g.x0 = (uint32_t)x0; g.ch = (uint32_t)ch; g.cw = (uint32_t)cw; g.w = (uint32_t)w;
    g.plane_s = (uint32_t)h * (uint32_t)w;
    g.plane_d = (uint32_t)ch * (uint32_t)cw;
    const uint32_t n = 3u * g.plane_d;                                          // <= slot_out < 2^31
    const uint32_t tid = blockIdx.x * CS_BLOCK + threadIdx.x, step = CS_BLOCKS * CS_BLOCK;
    // four consecutive destination floats per thread as ONE 16-byte store where the slot's address allows; the source is read float by
    // float (its rows start at x0: 4-byte aligned only), the lanes of a wave reading neighbouring addresses
    const uint32_t n4 = (((uintptr_t)d) & 15) == 0 ? n >> 2 : 0;
    for (uint32_t v = tid; v < n4; v += step) {
        uint32_t c, y, x;
        crop_split(g, 4u * v, c, y, x);
        float f[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f[j] = s[c * g.plane_s + (g.y0 + y) * g.w + g.x0 + x];
            if (++x == g.cw) {
                x = 0;
                if (++y == g.ch) { y = 0; ++c; }
            }
        }
        rn::f32x4 o;
        o.x = f[0]; o.y = f[1]; o.z = f[2]; o.w = f[3];
        ((rn::f32x4 *)d)[v] = o;
    }
    for (uint32_t e = 4u * n4 + tid; e < n; e += step) {
        uint32_t c, y, x;
        crop_split(g, e, c, y, x);
        d[e] = s[c * g.plane_s + (g.y0 + y) * g.w + g.x0 + x];
    }
}

}  // namespace

RN_API int rn_bbox_crop_draw(rn_bbox_crop_state *state, const float *gt_boxes, const int32_t *gt_off, const int32_t *in_hw_dev, int B,
                             int32_t *rect, int32_t *crop_hw, float *out_boxes, int64_t rows, void *stream)
{
    if (!state || !gt_off || !in_hw_dev || !rect || !crop_hw || B <= 0 || rows < 0 || rows > INT32_MAX) return RN_EINVAL;
    if (rows > 0 && (!gt_boxes || !out_boxes || gt_boxes == out_boxes)) return RN_EINVAL;
    if (!rn::aligned(state, 8) || !rn::aligned(gt_off, 4) || !rn::aligned(in_hw_dev, 4) || !rn::aligned(rect, 4) || !rn::aligned(crop_hw, 4) ||
        !rn::aligned(gt_boxes, 16) || !rn::aligned(out_boxes, 16))
        return RN_EALIGN;
    hipLaunchKernelGGL(bbox_crop_draw_kernel, dim3((unsigned)B), dim3(HF_BLOCK), 0, (hipStream_t)stream, state, (const rn::f32x4 *)gt_boxes,
                       gt_off, in_hw_dev, rect, crop_hw, (rn::f32x4 *)out_boxes, (int32_t)rows);
    hipLaunchKernelGGL(draw_advance_kernel, dim3(1), dim3(DRAW_ADVANCE_BLOCK), 0, (hipStream_t)stream, &state->counter);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

RN_API int rn_image_crop_stage(const float *arena, int64_t slot, const int32_t *in_hw_dev, const int32_t *rect, int B, float *arena_out,
                               int64_t slot_out, void *stream)
{
    if (!arena || !in_hw_dev || !rect || !arena_out || arena == arena_out || B <= 0 || B > 65535) return RN_EINVAL;
    if (slot < 3 || slot_out < 3 || slot > INT32_MAX || slot_out > INT32_MAX) return RN_EINVAL;      // (the kernel indexes a slot with 32 bits)
    if (!rn::aligned(arena, 4) || !rn::aligned(arena_out, 4) || !rn::aligned(in_hw_dev, 4) || !rn::aligned(rect, 4)) return RN_EALIGN;
    hipLaunchKernelGGL(image_crop_stage_kernel, dim3(CS_BLOCKS, (unsigned)B), dim3(CS_BLOCK), 0, (hipStream_t)stream, arena, slot, in_hw_dev,
                       rect, arena_out, slot_out);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

RN_API int rn_color_jitter_draw(rn_color_jitter_state *state, int B, rn_color_coef *coef, void *stream)
{
    if (!state || !coef || B <= 0) return RN_EINVAL;
    if (!rn::aligned(state, 8) || !rn::aligned(coef, 4)) return RN_EALIGN;
    hipLaunchKernelGGL(color_jitter_draw_kernel, dim3(1), dim3(HF_BLOCK), 0, (hipStream_t)stream, state, B, coef);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

RN_API size_t rn_color_mean_workspace_bytes(int B)
{
    return B > 0 ? (size_t)B * CM_BLOCKS * sizeof(double) : 0;
}

// (the partial sums, and behind them f32[B] for ref, rounded up to 8 bytes)
RN_API size_t rn_brightness_contrast_mean_workspace_bytes(int B)
{
    return B > 0 ? (size_t)B * CM_BLOCKS * sizeof(double) + (((size_t)B * sizeof(float) + 7) & ~(size_t)7) : 0;
}

// rn_color_mean (bc false) and rn_brightness_contrast_mean (bc true): the same arguments, checks and launch table
static int mean_launch(const bool bc, const void *const *images, const int32_t *in_hw, const float *arena, int64_t slot, const int32_t *in_hw_dev,
                       int B, rn_color_coef *coef, void *workspace, size_t workspace_bytes, void *stream)
{
    const bool var = arena != nullptr;
    if (!coef || !workspace || B <= 0) return RN_EINVAL;
    if (var ? (images || in_hw || !in_hw_dev || slot < 3) : (!images || !in_hw || in_hw_dev)) return RN_EINVAL;
    if (workspace_bytes < (bc ? rn_brightness_contrast_mean_workspace_bytes(B) : rn_color_mean_workspace_bytes(B))) return RN_EINVAL;
    if (!rn::aligned(coef, 4) || !rn::aligned(workspace, 8)) return RN_EALIGN;
    if (var && (!rn::aligned(arena, 16) || !rn::aligned(in_hw_dev, 4))) return RN_EALIGN;
    for (int b = 0; b < B && !var; ++b) {
        if (!images[b] || in_hw[2 * b] <= 0 || in_hw[2 * b + 1] <= 0) return RN_EINVAL;
        if (!rn::aligned(images[b], 4)) return RN_EALIGN;
    }
    hipStream_t st = (hipStream_t)stream;
    float *ref = (float *)((double *)workspace + (int64_t)B * CM_BLOCKS);        // bc: behind the partial sums
    for (int b0 = 0; b0 < B; b0 += CM_MAX_IMAGES) {
        const int cnt = (B - b0) < CM_MAX_IMAGES ? (B - b0) : CM_MAX_IMAGES;
        ColorMeanArgs a;
        for (int i = 0; i < CM_MAX_IMAGES; ++i) {
            const bool on = !var && i < cnt;
            a.img[i] = on ? (const float *)images[b0 + i] : nullptr;
            a.ih[i] = on ? in_hw[2 * (b0 + i)] : 0;
            a.iw[i] = on ? in_hw[2 * (b0 + i) + 1] : 0;
        }
        a.arena = var ? arena + (int64_t)b0 * slot : nullptr;
        a.in_hw = var ? in_hw_dev + 2 * b0 : nullptr;
        a.slot = slot;
        a.coef = coef + b0;                                      // (this launch's first image: the kernels index from 0)
        a.partial = (double *)workspace + (int64_t)b0 * CM_BLOCKS;
        const dim3 grid(CM_BLOCKS, (unsigned)cnt);
        if (bc && var) {
            hipLaunchKernelGGL(bc_mean_partial_kernel<true>, grid, dim3(CM_BLOCK), 0, st, a);
            hipLaunchKernelGGL(bc_mean_finish_kernel<true>, dim3(1), dim3(HF_BLOCK), 0, st, a, ref + b0, cnt);
        } else if (bc) {
            hipLaunchKernelGGL(bc_mean_partial_kernel<false>, grid, dim3(CM_BLOCK), 0, st, a);
            hipLaunchKernelGGL(bc_mean_finish_kernel<false>, dim3(1), dim3(HF_BLOCK), 0, st, a, ref + b0, cnt);
        } else if (var) {
            hipLaunchKernelGGL(color_mean_partial_kernel<true>, grid, dim3(CM_BLOCK), 0, st, a);
            hipLaunchKernelGGL(color_mean_finish_kernel<true>, dim3(1), dim3(HF_BLOCK), 0, st, a, cnt);
        } else {
            hipLaunchKernelGGL(color_mean_partial_kernel<false>, grid, dim3(CM_BLOCK), 0, st, a);
            hipLaunchKernelGGL(color_mean_finish_kernel<false>, dim3(1), dim3(HF_BLOCK), 0, st, a, cnt);
        }
        RN_LAUNCH_CHECK();
    }
    return RN_OK;
}

RN_API int rn_color_mean(const void *const *images, const int32_t *in_hw, const float *arena, int64_t slot, const int32_t *in_hw_dev, int B,
                         rn_color_coef *coef, void *workspace, size_t workspace_bytes, void *stream)
{
    return mean_launch(false, images, in_hw, arena, slot, in_hw_dev, B, coef, workspace, workspace_bytes, stream);
}

RN_API int rn_brightness_contrast_draw(rn_brightness_contrast_state *state, int B, rn_color_coef *coef, int fresh, void *stream)
{
    if (!state || !coef || B <= 0) return RN_EINVAL;
    if (!rn::aligned(state, 8) || !rn::aligned(coef, 4)) return RN_EALIGN;
    hipLaunchKernelGGL(brightness_contrast_draw_kernel, dim3(1), dim3(HF_BLOCK), 0, (hipStream_t)stream, state, B, coef, fresh ? 1 : 0);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

RN_API int rn_brightness_contrast_mean(const void *const *images, const int32_t *in_hw, const float *arena, int64_t slot,
                                       const int32_t *in_hw_dev, int B, rn_color_coef *coef, void *workspace, size_t workspace_bytes,
                                       void *stream)
{
    return mean_launch(true, images, in_hw, arena, slot, in_hw_dev, B, coef, workspace, workspace_bytes, stream);
}

RN_API int rn_hflip_draw(rn_hflip_state *state, int B, uint8_t *flags, void *stream)
{
    if (!state || !flags || B <= 0) return RN_EINVAL;
    if (!rn::aligned(state, 8)) return RN_EALIGN;
    hipLaunchKernelGGL(hflip_draw_kernel, dim3(1), dim3(HF_BLOCK), 0, (hipStream_t)stream, state, B, flags);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

RN_API int rn_short_side_draw(rn_short_side_state *state, const int32_t *in_hw, int max_size, int B, int32_t *out_hw, float *ratios,
                              void *stream)
{
    if (!state || !in_hw || !out_hw || !ratios || B <= 0 || max_size <= 0) return RN_EINVAL;
    if (!rn::aligned(state, 8) || !rn::aligned(out_hw, 4) || !rn::aligned(ratios, 4)) return RN_EALIGN;
    for (int b = 0; b < B; ++b)
        if (in_hw[2 * b] <= 0 || in_hw[2 * b + 1] <= 0) return RN_EINVAL;
    for (int base = 0; base < B; base += SS_MAX_IMAGES) {
        const int cnt = (B - base) < SS_MAX_IMAGES ? (B - base) : SS_MAX_IMAGES;
        ShortSideTable t;
        for (int i = 0; i < SS_MAX_IMAGES; ++i) {
            t.ih[i] = i < cnt ? in_hw[2 * (base + i)] : 1;
            t.iw[i] = i < cnt ? in_hw[2 * (base + i) + 1] : 1;
        }
        // (launches of one stream run in order: the earlier ones read the counter that the last one advances)
        hipLaunchKernelGGL(short_side_draw_kernel, dim3(1), dim3(HF_BLOCK), 0, (hipStream_t)stream, state, t, cnt, base, max_size,
                           base + cnt == B ? 1 : 0, out_hw, ratios);
        RN_LAUNCH_CHECK();
    }
    return RN_OK;
}

RN_API int rn_resize_plan_dev(rn_short_side_state *state_or_null, const int32_t *in_hw_dev, int fixed_short, int max_size, int B,
                              int32_t *out_hw, float *ratios, void *stream)
{
    if (!in_hw_dev || !out_hw || !ratios || B <= 0 || max_size <= 0) return RN_EINVAL;
    if (!state_or_null && fixed_short <= 0) return RN_EINVAL;
    if ((state_or_null && !rn::aligned(state_or_null, 8)) || !rn::aligned(in_hw_dev, 4) || !rn::aligned(out_hw, 4) || !rn::aligned(ratios, 4))
        return RN_EALIGN;
    if (state_or_null)
        hipLaunchKernelGGL(resize_plan_dev_kernel<true>, dim3(1), dim3(HF_BLOCK), 0, (hipStream_t)stream, state_or_null, in_hw_dev, 0, max_size,
                           B, out_hw, ratios);
    else
        hipLaunchKernelGGL(resize_plan_dev_kernel<false>, dim3(1), dim3(HF_BLOCK), 0, (hipStream_t)stream, state_or_null, in_hw_dev, fixed_short,
                           max_size, B, out_hw, ratios);
    RN_LAUNCH_CHECK();
    return RN_OK;
}
