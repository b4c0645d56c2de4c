// The colour-jitter arithmetic of ONE pixel (augment.ColorJitter; include/retinanet_hip.h: rn_color_coef), shared by the transform
// kernel (transform.hip, which applies it to every tap) and the contrast-mean kernel (augment.hip, which applies the operations that
// precede the contrast), so that the two cannot drift apart.  The pin is torchvision 0.8's tensor algorithm
// (transforms.functional_tensor) on fp32 RGB in [0, 1]: every operation below is one correctly rounded fp32 add, multiply, divide,
// compare, floor or select, in the written order -- the files that include this are built without FMA contraction and with IEEE division.
#pragma once
#include "rn_common.hpp"

namespace rn {

constexpr int COLOR_BRIGHTNESS = 0, COLOR_CONTRAST = 1, COLOR_SATURATION = 2, COLOR_HUE = 3, COLOR_SKIP = 0xF;
// bits of rn_color_coef.order above the four nibbles: brightness / contrast present (bc_mul, bc_add are applied), and bc_add still
// holds beta because the image mean it is to be multiplied with is pending (rn_brightness_contrast_mean clears it)
constexpr int COLOR_BC_PRESENT = 1 << 16, COLOR_BC_PENDING = 1 << 17;

__device__ __forceinline__ float color_clamp(const float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }

__device__ __forceinline__ float color_gray(const float r, const float g, const float b) { return 0.2989f * r + 0.587f * g + 0.114f * b; }

// x = clamp(f * x + (1 - f) * other)
__device__ __forceinline__ float color_blend(const float x, const float other, const float f) { return color_clamp(f * x + (1.0f - f) * other); }

__device__ __forceinline__ void color_hue(float &r, float &g, float &b, const float f)
{
    // RGB -> HSV
    const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
    const bool eq = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eq ? 1.0f : maxc);
    const float d = eq ? 1.0f : cr;
    const float rc = (maxc - r) / d, gc = (maxc - g) / d, bc = (maxc - b) / d;
    const float h0 = maxc == r ? bc - gc : (maxc == g ? 2.0f + rc - bc : 4.0f + gc - rc);
    float h = fmodf(h0 / 6.0f + 1.0f, 1.0f);
    const float v = maxc;
    // the shift
    h = h + f;
    h = h - floorf(h);
    // HSV -> RGB
    const float h6 = h * 6.0f;
    const float fl = floorf(h6);
    const float ff = h6 - fl;
    int i = (int)fl % 6;
    i = i < 0 ? i + 6 : i;
    const float p = color_clamp(v * (1.0f - s));
    const float q = color_clamp(v * (1.0f - s * ff));
    const float t = color_clamp(v * (1.0f - s * (1.0f - ff)));
    r = i == 0 ? v : (i == 1 ? q : (i == 2 ? p : (i == 3 ? p : (i == 4 ? t : v))));
    g = i == 0 ? t : (i == 1 ? v : (i == 2 ? v : (i == 3 ? q : (i == 4 ? p : p))));
    b = i == 0 ? p : (i == 1 ? p : (i == 2 ? t : (i == 3 ? v : (i == 4 ? v : q))));
}

__device__ __forceinline__ bool color_has_contrast(const int order)
{
    return (order & 0xF) == COLOR_CONTRAST || ((order >> 4) & 0xF) == COLOR_CONTRAST || ((order >> 8) & 0xF) == COLOR_CONTRAST ||
           ((order >> 12) & 0xF) == COLOR_CONTRAST;
}

// The operations of c.order on one pixel, in their order; UNTIL_CONTRAST: only those before the contrast (the pixel the contrast mean
// is taken over).  c is the same for every lane of a block, so the branches are wave-uniform.
template <bool UNTIL_CONTRAST>
__device__ __forceinline__ void color_apply(float &r, float &g, float &b, const rn_color_coef &c)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int op = (c.order >> (4 * k)) & 0xF;
        if (op == COLOR_BRIGHTNESS) {
            const float f = c.f[COLOR_BRIGHTNESS];
            r = color_clamp(r * f); g = color_clamp(g * f); b = color_clamp(b * f);
        } else if (op == COLOR_CONTRAST) {
            if (UNTIL_CONTRAST) return;
            const float f = c.f[COLOR_CONTRAST], m = c.mean;
            r = color_blend(r, m, f); g = color_blend(g, m, f); b = color_blend(b, m, f);
        } else if (op == COLOR_SATURATION) {
            const float f = c.f[COLOR_SATURATION], y = color_gray(r, g, b);
            r = color_blend(r, y, f); g = color_blend(g, y, f); b = color_blend(b, y, f);
        } else if (op == COLOR_HUE) {
            color_hue(r, g, b, c.f[COLOR_HUE]);
        }
    }
    // brightness / contrast (augment.RandomBrightnessContrast; the header's step 5) behind the four operations: one multiply, one add,
    // the clamp.  A row of rn_color_jitter_draw has the bit clear and takes the code above alone.
    if (!UNTIL_CONTRAST && (c.order & COLOR_BC_PRESENT)) {
        const float m = c.bc_mul, a = c.bc_add;
        r = color_clamp(m * r + a); g = color_clamp(m * g + a); b = color_clamp(m * b + a);
    }
}

}  // namespace rn
