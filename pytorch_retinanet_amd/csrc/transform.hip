// T1 transform_batch -- replaces the torchvision GeneralizedRCNNTransform the reference runs at
// retinanet/models.py:116, :262, :279 (normalise -> bilinear resize -> zero-padded batch), i.e. per
// image ~2 elementwise kernels + interpolate + a strided copy, plus the batch memset, the
// channels_last re-layout and autocast's fp32->bf16 cast of the conv1 input -- as ONE launch:
//
//   out[b][c][y][x] = y < oh_b && x < ow_b ? bilinear((in_b - mean_c) / std_c)(y, x) : 0
//
// Sampling is torch's upsample_bilinear2d with align_corners=False and the scale recomputed from
// the integer sizes (recompute_scale_factor=True): src = (dst + 0.5) * (in / out) - 0.5, clamped
// at 0, taps (i0, min(i0 + 1, in - 1)), weights (1 - l, l); each tap is normalised before the blend,
// like the reference (normalise first, then resize).  When in == out the weights are exactly
// (1, 0), so the identity case is a single tap.  HBM-bound: reads sum_b 3*h_b*w_b*4 bytes (each
// input pixel is touched by at most 4 neighbouring outputs, served by L1/L2), writes
// B*3*Hp*Wp*s bytes, s = output element size.
//
// Each thread produces 4 consecutive x of one row for all 3 channels, so every output layout gets
// 8- or 16-byte stores: NCHW (f32: 3 x 16 B, 16-bit: 3 x 8 B) or channels-last NHWC (f32: 3 x 16 B,
// 16-bit: 3 x 8 B contiguous).
//
// rn_transform_batch_flip is the same launch with a per-image flag (device, uint8[B], rn_hflip_draw writes it inside a captured
// step): a flagged image's taps are computed as above and then read from the mirrored source columns iw-1-xa / iw-1-xb, i.e.
// exactly what rn_transform_batch computes on img.flip(-1) (the reference flips the raw image before the model's transform).
//
// rn_transform_batch_dev is the same launch again with the output sizes read from DEVICE memory (i32[B][2], rn_short_side_draw writes
// them inside a captured step: augment.RandomShortSide) instead of the kernel-argument table; the canvas Hp x Wp stays a host value
// and a size read from the device is clamped to it, so nothing it holds can make a thread write outside the batch.  Everything after
// the two loads is the code above: bit-identical to rn_transform_batch / _flip called with the same sizes on the host.
//
// rn_transform_batch_var is the _dev launch with the INPUT side on the device as well (graph.CapturedTrainStep's image capacity mode):
// image b lies dense at the start of slot b of a fixed arena (rn_image_stage, below, copies it there before every step) and its
// (ih, iw) are read from device memory next to the (oh, ow) of the resize plan (rn_resize_plan_dev), so neither an image's address nor
// any of its sizes is a kernel argument and one captured graph serves images of every size that fits a slot.  What the device holds
// cannot move a thread outside its operands: oh / ow are clamped to the canvas, and an image with ih < 1, iw < 1 or 3 * ih * iw > slot
// is all padding (every tap lies inside [0, 3 * ih * iw) otherwise).  After the loads it is the code above once more.
//
// rn_image_stage copies B dense f32 [3][h_b][w_b] images into their arena slots and writes in_hw on the device: ONE launch per 64
// images with the pointers and sizes passed BY VALUE in the kernel arguments (like rn_gt_stage), 16-byte vector copies when the
// source is 16-byte aligned (a slot always is) and 4-byte copies otherwise and for the tail.
//
// rn_image_stage_u8 is that launch for uint8 sources, planes [3][h][w] or interleaved [h][w][3] (what image decoders give), converted
// on the way: slot b holds float(v) / 255.0f -- ONE correctly rounded division, never the product with 1 / 255, which differs in the
// last bit for 126 of the 256 bytes -- as dense [3][h][w], i.e. the bits rn_image_stage leaves for the image converted on the CPU.
// Per step a thread turns 16 pixels (48 or 16 source bytes as 16-byte loads) into 16 floats per channel.
//
// rn_transform_batch_color is any of the launches above with the train-time colour jitter (augment.ColorJitter) applied to the raw
// pixels: template flag COLOR, and per image a rn_color_coef on the device (rn_color_jitter_draw writes the factors and the order
// inside a captured step, rn_color_mean the contrast mean).  With COLOR every tap loads its three channels, runs the operations of
// coef[b].order on the triple (rn_color.hpp; b = blockIdx.z, so the branches are wave-uniform) and is then normalised and blended as
// above.  The jitter is per pixel apart from the mean, so it commutes with the flip; an order of all 0xF gives the plain launch's bits.
// The COLOR = false instantiations are the code they were.  Brightness / contrast (augment.RandomBrightnessContrast) rides in the same
// rows -- bc_mul, bc_add and bit 16 of the order -- and is the last step of color_apply<false>: no flag, no argument and no branch here.
#include "rn_color.hpp"
#include "rn_common.hpp"

namespace {

constexpr int TB_MAX_IMAGES = 64;      // per launch (kernarg table)
constexpr int TB_PX = 4;

struct TransformArgs {
    const float *img[TB_MAX_IMAGES];   // [3][h][w] f32, contiguous
    int32_t ih[TB_MAX_IMAGES], iw[TB_MAX_IMAGES], oh[TB_MAX_IMAGES], ow[TB_MAX_IMAGES];
    float mean[3], std[3];
    int32_t B, Hp, Wp;
    void *out;                         // first image of this launch
    const uint8_t *flags;              // FLIP: this launch's first image's flag (device)
    const int32_t *out_hw;             // DEV: this launch's first image's (oh, ow) (device); oh / ow above are unused
    const float *arena;                // VAR: this launch's first image's slot (device); img / ih / iw above are unused
    const int32_t *in_hw;              // VAR: this launch's first image's (ih, iw) (device)
    int64_t slot;                      // VAR: floats per slot
    const rn_color_coef *coef;         // COLOR: this launch's first image's coefficients (device)
};

__device__ __forceinline__ void tap_axis(const int dst, const int in, const int out, int &i0, int &i1, float &l0, float &l1)
{
    if (in == out) { i0 = i1 = dst; l0 = 1.0f; l1 = 0.0f; return; }
    const float scale = (float)in / (float)out;
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    src = src < 0.0f ? 0.0f : src;
    i0 = (int)src;
    i0 = i0 < in - 1 ? i0 : in - 1;
    i1 = i0 + ((i0 < in - 1) ? 1 : 0);
    l1 = src - (float)i0;
    l0 = 1.0f - l1;
}

template <int DT> struct store4;
template <> struct store4<RN_F32> {
    static __device__ __forceinline__ void st(void *p, int64_t elem, const float (&v)[4]) {
        rn::f32x4 o; o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
        *(rn::f32x4 *)((float *)p + elem) = o;
    }
};
template <> struct store4<RN_BF16> {
    static __device__ __forceinline__ void st(void *p, int64_t elem, const float (&v)[4]) {
        rn::u32x2 o; o.x = rn::dt<RN_BF16>::pk(v[0], v[1]); o.y = rn::dt<RN_BF16>::pk(v[2], v[3]);
        *(rn::u32x2 *)((uint16_t *)p + elem) = o;
    }
};
template <> struct store4<RN_F16> {
    static __device__ __forceinline__ void st(void *p, int64_t elem, const float (&v)[4]) {
        rn::u32x2 o; o.x = rn::dt<RN_F16>::pk(v[0], v[1]); o.y = rn::dt<RN_F16>::pk(v[2], v[3]);
        *(rn::u32x2 *)((uint16_t *)p + elem) = o;
    }
};

// COLOR: the three channels of the source pixel at ``at`` after the colour operations of c, normalised
__device__ __forceinline__ void color_tap(const float *__restrict__ src, const int64_t plane, const int64_t at, const rn_color_coef &c,
                                          const float (&mean)[3], const float (&std)[3], float (&o)[3])
{
    float r = src[at], g = src[plane + at], b = src[2 * plane + at];
    rn::color_apply<false>(r, g, b, c);
    o[0] = (r - mean[0]) / std[0]; o[1] = (g - mean[1]) / std[1]; o[2] = (b - mean[2]) / std[2];
}

// VAR implies DEV
template <int DT, bool NHWC, bool FLIP, bool DEV, bool VAR, bool COLOR>
__global__ __launch_bounds__(256) void transform_batch_kernel(const TransformArgs a)
{
    const int b = blockIdx.z;
    const int y = blockIdx.y;
    const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * TB_PX;
    if (x0 >= a.Wp) return;
    const int ih = VAR ? a.in_hw[2 * b] : a.ih[b], iw = VAR ? a.in_hw[2 * b + 1] : a.iw[b];
    int oh, ow;
    if (DEV) {                                                  // device data: clamped to the canvas (<= 0: the image is all padding)
        oh = a.out_hw[2 * b]; ow = a.out_hw[2 * b + 1];
        oh = oh < a.Hp ? oh : a.Hp; ow = ow < a.Wp ? ow : a.Wp;
    } else {
        oh = a.oh[b]; ow = a.ow[b];
    }
    if (VAR && (ih < 1 || iw < 1 || (int64_t)ih * iw > a.slot / 3)) oh = ow = 0;      // device data that no slot can hold (3 * ih * iw > slot): all padding
    const bool flip = FLIP && a.flags[b] != 0;           // source column c of the flipped image is column iw-1-c of img
    float v[3][TB_PX];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int p = 0; p < TB_PX; ++p) v[c][p] = 0.0f;

    if (y < oh && x0 < ow) {
        const float *__restrict__ src = VAR ? a.arena + (int64_t)b * a.slot : a.img[b];
        const int64_t plane = (int64_t)ih * iw;
        int y0, y1; float ly0, ly1;
        tap_axis(y, ih, oh, y0, y1, ly0, ly1);
        if (COLOR) {
            const rn_color_coef cc = a.coef[b];
            const bool ident = ih == oh && iw == ow;             // one tap, as below
#pragma unroll
            for (int p = 0; p < TB_PX; ++p) {
                const int x = x0 + p;
                if (x < ow) {
                    int xa, xb; float lx0, lx1;
                    tap_axis(x, iw, ow, xa, xb, lx0, lx1);
                    if (flip) { xa = iw - 1 - xa; xb = iw - 1 - xb; }
                    float p00[3];
                    color_tap(src, plane, (int64_t)y0 * iw + xa, cc, a.mean, a.std, p00);
                    if (ident) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) v[c][p] = p00[c];
                    } else {
                        float p01[3], p10[3], p11[3];
                        color_tap(src, plane, (int64_t)y0 * iw + xb, cc, a.mean, a.std, p01);
                        color_tap(src, plane, (int64_t)y1 * iw + xa, cc, a.mean, a.std, p10);
                        color_tap(src, plane, (int64_t)y1 * iw + xb, cc, a.mean, a.std, p11);
#pragma unroll
                        for (int c = 0; c < 3; ++c) v[c][p] = ly0 * (lx0 * p00[c] + lx1 * p01[c]) + ly1 * (lx0 * p10[c] + lx1 * p11[c]);
                    }
                }
            }
        } else if (ih == oh && iw == ow) {                      // identity: one tap
#pragma unroll
            for (int p = 0; p < TB_PX; ++p) {
                const int x = x0 + p;
                if (x < ow) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[c][p] = (src[c * plane + (int64_t)y * iw + (flip ? iw - 1 - x : x)] - a.mean[c]) / a.std[c];
                }
            }
        } else {
#pragma unroll
            for (int p = 0; p < TB_PX; ++p) {
                const int x = x0 + p;
                if (x < ow) {
                    int xa, xb; float lx0, lx1;
                    tap_axis(x, iw, ow, xa, xb, lx0, lx1);
                    if (flip) { xa = iw - 1 - xa; xb = iw - 1 - xb; }
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float *pl = src + c * plane;
                        const float m = a.mean[c], s = a.std[c];
                        const float p00 = (pl[(int64_t)y0 * iw + xa] - m) / s, p01 = (pl[(int64_t)y0 * iw + xb] - m) / s;
                        const float p10 = (pl[(int64_t)y1 * iw + xa] - m) / s, p11 = (pl[(int64_t)y1 * iw + xb] - m) / s;
                        v[c][p] = ly0 * (lx0 * p00 + lx1 * p01) + ly1 * (lx0 * p10 + lx1 * p11);
                    }
                }
            }
        }
    }
    const int64_t HW = (int64_t)a.Hp * a.Wp;
    if (NHWC) {                                                 // [b][y][x][c]: 12 contiguous elements
        const int64_t e = ((int64_t)b * HW + (int64_t)y * a.Wp + x0) * 3;
        const float q0[4] = {v[0][0], v[1][0], v[2][0], v[0][1]};
        const float q1[4] = {v[1][1], v[2][1], v[0][2], v[1][2]};
        const float q2[4] = {v[2][2], v[0][3], v[1][3], v[2][3]};
        store4<DT>::st(a.out, e, q0); store4<DT>::st(a.out, e + 4, q1); store4<DT>::st(a.out, e + 8, q2);
    } else {                                                    // [b][c][y][x]
#pragma unroll
        for (int c = 0; c < 3; ++c) store4<DT>::st(a.out, ((int64_t)b * 3 + c) * HW + (int64_t)y * a.Wp + x0, v[c]);
    }
}

// out_hw: HOST sizes, or null with out_hw_dev (DEVICE i32[B][2]) in their place; images / in_hw: HOST arrays, or both null with
// arena / slot / in_hw_dev (the staged images on the DEVICE) in their place -- only together with out_hw_dev
int transform_batch(const void *const *images, const int32_t *in_hw, const float *arena, int64_t slot, const int32_t *in_hw_dev,
                    const int32_t *out_hw, const int32_t *out_hw_dev, int B, const float mean[3], const float std[3], int Hp, int Wp,
                    void *out, int out_dtype, int channels_last, const uint8_t *flags, const rn_color_coef *coef, void *stream)
{
    const bool var = arena != nullptr;
    if (coef && !rn::aligned(coef, 4)) return RN_EALIGN;
    if ((!out_hw == !out_hw_dev) || !mean || !std || !out || B <= 0 || Hp <= 0 || Wp <= 0) return RN_EINVAL;
    if (var ? (images || in_hw || !in_hw_dev || !out_hw_dev || slot < 3) : (!images || !in_hw || in_hw_dev))
        return RN_EINVAL;
    if (out_hw_dev && !rn::aligned(out_hw_dev, 4)) return RN_EALIGN;
    if (var && (!rn::aligned(arena, 16) || !rn::aligned(in_hw_dev, 4))) return RN_EALIGN;
    if (out_dtype != RN_F32 && out_dtype != RN_BF16 && out_dtype != RN_F16) return RN_EINVAL;
    if (Wp % TB_PX) return RN_EUNSUPPORTED;
    if (Hp > 65535) return RN_EUNSUPPORTED;                     // gridDim.y
    if (!rn::aligned(out, 16)) return RN_EALIGN;
    for (int b = 0; b < B && !var; ++b) {
        if (!images[b] || in_hw[2 * b] <= 0 || in_hw[2 * b + 1] <= 0) return RN_EINVAL;
        if (out_hw && (out_hw[2 * b] <= 0 || out_hw[2 * b + 1] <= 0 || out_hw[2 * b] > Hp || out_hw[2 * b + 1] > Wp)) return RN_EINVAL;
        if (!rn::aligned(images[b], 4)) return RN_EALIGN;
        if (std[0] == 0.0f || std[1] == 0.0f || std[2] == 0.0f) return RN_EINVAL;
    }
    // (every form refuses a zero std: the list forms in the loop above, where the check has always been, the staged form here)
    if (var && (std[0] == 0.0f || std[1] == 0.0f || std[2] == 0.0f)) return RN_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const size_t esz = out_dtype == RN_F32 ? 4 : 2;
    for (int b0 = 0; b0 < B; b0 += TB_MAX_IMAGES) {
        TransformArgs a;
        a.B = (B - b0) < TB_MAX_IMAGES ? (B - b0) : TB_MAX_IMAGES;
        for (int i = 0; i < a.B; ++i) {
            a.img[i] = var ? nullptr : (const float *)images[b0 + i];
            a.ih[i] = var ? 0 : in_hw[2 * (b0 + i)]; a.iw[i] = var ? 0 : in_hw[2 * (b0 + i) + 1];
            a.oh[i] = out_hw ? out_hw[2 * (b0 + i)] : 0; a.ow[i] = out_hw ? out_hw[2 * (b0 + i) + 1] : 0;
        }
        a.arena = var ? arena + (int64_t)b0 * slot : nullptr;
        a.in_hw = var ? in_hw_dev + 2 * b0 : nullptr;
        a.slot = slot;
        for (int c = 0; c < 3; ++c) { a.mean[c] = mean[c]; a.std[c] = std[c]; }
        a.Hp = Hp; a.Wp = Wp;
        a.out = (unsigned char *)out + (size_t)b0 * 3 * Hp * Wp * esz;
        a.flags = flags ? flags + b0 : nullptr;
        a.out_hw = out_hw_dev ? out_hw_dev + 2 * b0 : nullptr;
        a.coef = coef ? coef + b0 : nullptr;
        const dim3 blk(256), grid((unsigned)((Wp / TB_PX + 255) / 256), (unsigned)Hp, (unsigned)a.B);
#define RN_TB_LAUNCH_C(DT, NHWC, FLIP, DEV, VAR)                                                                          \
        if (coef) hipLaunchKernelGGL((transform_batch_kernel<DT, NHWC, FLIP, DEV, VAR, true>), grid, blk, 0, st, a);      \
        else hipLaunchKernelGGL((transform_batch_kernel<DT, NHWC, FLIP, DEV, VAR, false>), grid, blk, 0, st, a)
#define RN_TB_LAUNCH_L(DT, FLIP, DEV, VAR)                                                                                \
        if (channels_last) { RN_TB_LAUNCH_C(DT, true, FLIP, DEV, VAR); } else { RN_TB_LAUNCH_C(DT, false, FLIP, DEV, VAR); }
#define RN_TB_LAUNCH(DT)                                                                                                  \
        if (var) {                                                                                                        \
            if (flags) { RN_TB_LAUNCH_L(DT, true, true, true); } else { RN_TB_LAUNCH_L(DT, false, true, true); }          \
        } else if (out_hw_dev) {                                                                                          \
            if (flags) { RN_TB_LAUNCH_L(DT, true, true, false); } else { RN_TB_LAUNCH_L(DT, false, true, false); }        \
        } else {                                                                                                          \
            if (flags) { RN_TB_LAUNCH_L(DT, true, false, false); } else { RN_TB_LAUNCH_L(DT, false, false, false); }      \
        }
        switch (out_dtype) {
            case RN_F32: RN_TB_LAUNCH(RN_F32); break;
            case RN_BF16: RN_TB_LAUNCH(RN_BF16); break;
            default: RN_TB_LAUNCH(RN_F16); break;
        }
#undef RN_TB_LAUNCH
#undef RN_TB_LAUNCH_L
#undef RN_TB_LAUNCH_C
        RN_LAUNCH_CHECK();
    }
    return RN_OK;
}

// ---- the images of a batch into the slots of a fixed arena (the image capacity mode) -----------------------------------------------
constexpr int IS_MAX = 64;          // images per launch (kernel-argument table)
constexpr int IS_BLOCK = 256;
constexpr int IS_GRID_X = 256;      // blocks per image at most (a grid-stride loop covers the rest)

struct ImageStageTable {
    const float *src[IS_MAX];
    int64_t n[IS_MAX];                 // 3 * h * w floats (<= slot: checked on the host)
    int32_t h[IS_MAX], w[IS_MAX];
};

// (the table is indexed by blockIdx only: a per-lane index into the argument segment becomes a vector load of the table)
__global__ __launch_bounds__(IS_BLOCK) void image_stage_kernel(const ImageStageTable t, float *__restrict__ arena, const int64_t slot,
                                                              int32_t *__restrict__ in_hw, const int base)
{
    const int i = blockIdx.y;
    const float *__restrict__ s = t.src[i];
    float *__restrict__ d = arena + (int64_t)(base + i) * slot;
    const int64_t n = t.n[i];
    const int64_t tid = (int64_t)blockIdx.x * IS_BLOCK + threadIdx.x, step = (int64_t)gridDim.x * IS_BLOCK;
    // 16-byte copies where both sides allow (exactly n floats of the source are read and of the slot written), 4-byte ones for the rest
    const int64_t n4 = ((((uintptr_t)s) | ((uintptr_t)d)) & 15) == 0 ? n >> 2 : 0;
    for (int64_t v = tid; v < n4; v += step) ((rn::f32x4 *)d)[v] = ((const rn::f32x4 *)s)[v];
    for (int64_t e = n4 * 4 + tid; e < n; e += step) d[e] = s[e];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        in_hw[2 * (base + i)] = t.h[i];
        in_hw[2 * (base + i) + 1] = t.w[i];
    }
}

// ---- the same for the uint8 images a decoder gives: planes or interleaved, converted on the way into the fp32 arena -----------------
constexpr int IS_U8_PX = 16;        // pixels per thread and step: C 16-byte loads of a C-channel source

struct ImageStageU8Table {
    const uint8_t *src[IS_MAX];
    int32_t h[IS_MAX], w[IS_MAX], layout[IS_MAX];      // layout 0: [3][h][w], 1: [h][w][3]
};

// the correctly rounded quotient (this file is built without contraction and with the IEEE divide): NOT v * (1 / 255)
__device__ __forceinline__ float u8_unit(const uint32_t v) { return (float)v / 255.0f; }

// n pixels of C interleaved bytes each at s (any alignment) -> channel c of pixel p to d[c * plane + p].  Reads exactly C * n bytes and
// writes exactly n floats per channel.  The first ``head`` pixels bring the source to a 16-byte boundary (C is odd, so C * head =
// -s mod 16 has one solution below 16: head = -s * C^-1 mod 16); from there a thread takes IS_U8_PX pixels per step as C 16-byte
// loads, and the pixels after the last whole step are the tail.  Head and tail go byte by byte.  A channel whose first stepped float
// d + c * plane + head is 16-byte aligned is stored 16 bytes per lane, any other 4 bytes per lane (the test is per image and channel:
// wave-uniform).
template <int C>
__device__ __forceinline__ void stage_u8_run(const uint8_t *__restrict__ s, float *__restrict__ d, const int64_t plane, const int64_t n,
                                             const int64_t tid, const int64_t step)
{
    static_assert(C == 1 || C == 3, "C^-1 mod 16 below");
    constexpr int CINV = C == 3 ? 11 : 1;
    int64_t head = (int64_t)((((16 - ((uintptr_t)s & 15)) & 15) * CINV) & 15);
    head = head < n ? head : n;
    const int64_t steps = (n - head) / IS_U8_PX;
    const int64_t tail = head + steps * IS_U8_PX, rest = head + (n - tail);
    for (int64_t e = tid; e < rest; e += step) {
        const int64_t p = e < head ? e : tail + (e - head);
#pragma unroll
        for (int c = 0; c < C; ++c) d[c * plane + p] = u8_unit(s[C * p + c]);
    }
    const rn::u32x4 *__restrict__ sv = (const rn::u32x4 *)(s + C * head);
    for (int64_t j = tid; j < steps; j += step) {
        rn::u32x4 q[C];
#pragma unroll
        for (int i = 0; i < C; ++i) q[i] = sv[C * j + i];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float v[IS_U8_PX];
#pragma unroll
            for (int p = 0; p < IS_U8_PX; ++p) {
                const int k = C * p + c;                           // byte k of the C * 16 loaded
                v[p] = u8_unit((q[k >> 4][(k >> 2) & 3] >> ((k & 3) * 8)) & 0xffu);
            }
            float *__restrict__ o = d + c * plane + head + j * IS_U8_PX;
            if ((((uintptr_t)o) & 15) == 0) {
#pragma unroll
                for (int g = 0; g < IS_U8_PX / 4; ++g) {
                    rn::f32x4 f; f.x = v[4 * g]; f.y = v[4 * g + 1]; f.z = v[4 * g + 2]; f.w = v[4 * g + 3];
                    ((rn::f32x4 *)o)[g] = f;
                }
            } else {
#pragma unroll
                for (int p = 0; p < IS_U8_PX; ++p) o[p] = v[p];
            }
        }
    }
}

// (launch shape and table as image_stage_kernel; the layout is per image, so the branch is block-uniform)
__global__ __launch_bounds__(IS_BLOCK) void image_stage_u8_kernel(const ImageStageU8Table t, float *__restrict__ arena, const int64_t slot,
                                                                 int32_t *__restrict__ in_hw, const int base)
{
    const int i = blockIdx.y;
    const uint8_t *__restrict__ s = t.src[i];
    float *__restrict__ d = arena + (int64_t)(base + i) * slot;
    const int64_t plane = (int64_t)t.h[i] * t.w[i];                // (3 * plane <= slot: checked on the host)
    const int64_t tid = (int64_t)blockIdx.x * IS_BLOCK + threadIdx.x, step = (int64_t)gridDim.x * IS_BLOCK;
    if (t.layout[i] == 1) {
        stage_u8_run<3>(s, d, plane, plane, tid, step);
    } else {
        for (int c = 0; c < 3; ++c) stage_u8_run<1>(s + c * plane, d + c * plane, plane, plane, tid, step);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        in_hw[2 * (base + i)] = t.h[i];
        in_hw[2 * (base + i) + 1] = t.w[i];
    }
}

}  // namespace

RN_API int rn_image_stage_u8(const void *const *images, const int32_t *in_hw, const int32_t *layout, int B, float *arena, int64_t slot,
                             int32_t *in_hw_dev, void *stream)
{
    if (!images || !in_hw || !layout || !arena || !in_hw_dev || B <= 0 || slot <= 0) return RN_EINVAL;
    if (!rn::aligned(arena, 16) || !rn::aligned(in_hw_dev, 4)) return RN_EALIGN;
    // every argument is checked before anything is launched: a rejected call leaves the arena as it was (a source needs no alignment)
    for (int b = 0; b < B; ++b) {
        const int64_t h = in_hw[2 * b], w = in_hw[2 * b + 1];
        if (!images[b] || h <= 0 || w <= 0 || h * w > slot / 3) return RN_EINVAL;      // (3 * h * w > slot, without the overflow)
        if (layout[b] != 0 && layout[b] != 1) return RN_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    for (int base = 0; base < B; base += IS_MAX) {
        const int cnt = (B - base) < IS_MAX ? (B - base) : IS_MAX;
        ImageStageU8Table t;
        int64_t most = 0;
        for (int i = 0; i < IS_MAX; ++i) {
            const bool on = i < cnt;
            t.src[i] = on ? (const uint8_t *)images[base + i] : nullptr;
            t.h[i] = on ? in_hw[2 * (base + i)] : 0;
            t.w[i] = on ? in_hw[2 * (base + i) + 1] : 0;
            t.layout[i] = on ? layout[base + i] : 0;
            const int64_t px = (int64_t)t.h[i] * t.w[i];
            if (px > most) most = px;
        }
        int64_t bx = (most / IS_U8_PX + IS_BLOCK - 1) / IS_BLOCK;
        bx = bx < 1 ? 1 : (bx > IS_GRID_X ? IS_GRID_X : bx);
        hipLaunchKernelGGL(image_stage_u8_kernel, dim3((unsigned)bx, (unsigned)cnt), dim3(IS_BLOCK), 0, st, t, arena, slot, in_hw_dev, base);
        RN_LAUNCH_CHECK();
    }
    return RN_OK;
}

RN_API int rn_image_stage(const void *const *images, const int32_t *in_hw, int B, float *arena, int64_t slot, int32_t *in_hw_dev, void *stream)
{
    if (!images || !in_hw || !arena || !in_hw_dev || B <= 0 || slot <= 0) return RN_EINVAL;
    if (!rn::aligned(arena, 16) || !rn::aligned(in_hw_dev, 4)) return RN_EALIGN;
    // every argument is checked before anything is launched: a rejected call leaves the arena as it was
    for (int b = 0; b < B; ++b) {
        const int64_t h = in_hw[2 * b], w = in_hw[2 * b + 1];
        if (!images[b] || h <= 0 || w <= 0 || h * w > slot / 3) return RN_EINVAL;      // (3 * h * w > slot, without the overflow)
        if (!rn::aligned(images[b], 4)) return RN_EALIGN;
    }
    hipStream_t st = (hipStream_t)stream;
    for (int base = 0; base < B; base += IS_MAX) {
        const int cnt = (B - base) < IS_MAX ? (B - base) : IS_MAX;
        ImageStageTable t;
        int64_t most = 0;
        for (int i = 0; i < IS_MAX; ++i) {
            const bool on = i < cnt;
            t.src[i] = on ? (const float *)images[base + i] : nullptr;
            t.h[i] = on ? in_hw[2 * (base + i)] : 0;
            t.w[i] = on ? in_hw[2 * (base + i) + 1] : 0;
            t.n[i] = (int64_t)3 * t.h[i] * t.w[i];
            if (t.n[i] > most) most = t.n[i];
        }
        int64_t bx = (most / 4 + IS_BLOCK - 1) / IS_BLOCK;
        bx = bx < 1 ? 1 : (bx > IS_GRID_X ? IS_GRID_X : bx);
        hipLaunchKernelGGL(image_stage_kernel, dim3((unsigned)bx, (unsigned)cnt), dim3(IS_BLOCK), 0, st, t, arena, slot, in_hw_dev, base);
        RN_LAUNCH_CHECK();
    }
    return RN_OK;
}

RN_API int rn_transform_batch(const void *const *images, const int32_t *in_hw, const int32_t *out_hw, int B,
                              const float mean[3], const float std[3], int Hp, int Wp, void *out, int out_dtype,
                              int channels_last, void *stream)
{
    if (!out_hw) return RN_EINVAL;
    return transform_batch(images, in_hw, nullptr, 0, nullptr, out_hw, nullptr, B, mean, std, Hp, Wp, out, out_dtype, channels_last, nullptr, nullptr, stream);
}

RN_API int rn_transform_batch_flip(const void *const *images, const int32_t *in_hw, const int32_t *out_hw, int B,
                                   const float mean[3], const float std[3], int Hp, int Wp, void *out, int out_dtype,
                                   int channels_last, const uint8_t *flags, void *stream)
{
    if (!flags || !out_hw) return RN_EINVAL;
    return transform_batch(images, in_hw, nullptr, 0, nullptr, out_hw, nullptr, B, mean, std, Hp, Wp, out, out_dtype, channels_last, flags, nullptr, stream);
}

RN_API int rn_transform_batch_dev(const void *const *images, const int32_t *in_hw, int B, const float mean[3], const float std[3],
                                  int Hp, int Wp, void *out, int out_dtype, int channels_last, const int32_t *out_hw_dev,
                                  const uint8_t *flags_or_null, void *stream)
{
    if (!out_hw_dev) return RN_EINVAL;
    return transform_batch(images, in_hw, nullptr, 0, nullptr, nullptr, out_hw_dev, B, mean, std, Hp, Wp, out, out_dtype, channels_last, flags_or_null, nullptr, stream);
}

RN_API int rn_transform_batch_var(const float *arena, int64_t slot, const int32_t *in_hw_dev, const int32_t *out_hw_dev, int B,
                                  const float mean[3], const float std[3], int Hp, int Wp, void *out, int out_dtype, int channels_last,
                                  const uint8_t *flags_or_null, void *stream)
{
    if (!arena || !in_hw_dev || !out_hw_dev) return RN_EINVAL;
    return transform_batch(nullptr, nullptr, arena, slot, in_hw_dev, nullptr, out_hw_dev, B, mean, std, Hp, Wp, out, out_dtype, channels_last,
                           flags_or_null, nullptr, stream);
}

RN_API int rn_transform_batch_color(const void *const *images, const int32_t *in_hw, const float *arena, int64_t slot, const int32_t *in_hw_dev,
                                    const int32_t *out_hw, const int32_t *out_hw_dev, int B, const float mean[3], const float std[3], int Hp,
                                    int Wp, void *out, int out_dtype, int channels_last, const uint8_t *flags_or_null,
                                    const rn_color_coef *coef, void *stream)
{
    if (!coef) return RN_EINVAL;
    return transform_batch(images, in_hw, arena, slot, in_hw_dev, out_hw, out_hw_dev, B, mean, std, Hp, Wp, out, out_dtype, channels_last,
                           flags_or_null, coef, stream);
}
