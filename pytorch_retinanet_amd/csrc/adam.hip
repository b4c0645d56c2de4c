// Multi-tensor Adam / AdamW step on fp32 master weights with a 16-bit working copy, capturable.
//
// optim.MasterAdam / MasterAdamW: the same fp32-master + 16-bit-conv-weight scheme as rn_sgd_master_step (optim.hip), with
// torch.optim.Adam / AdamW's update.  Every hyperparameter and the step counter live in a per-group DEVICE block (double[16],
// RN_ADAM_HPARAMS): a captured step reads whatever the host last wrote there, so a per-step LR schedule replays one graph.
//
// Per group and step: adam_prologue_kernel (one wave) advances the step counter unless found_inf[0] != 0 and writes
//   step_size = lr / (1 - beta1^step)  and  bc2_sqrt = sqrt(1 - beta2^step)     (double, as torch computes them in Python),
// then adam_master_kernel updates up to 40 tensors per launch, elementwise, in torch's single-tensor (foreach=False) fp32 order,
// with the fused multiply-adds ATen's ROCm kernels perform (fma(a, b, c) = a * b + c rounded once):
//   g = float(grad) * (1 / grad_scale)              (the GradScaler's scale; the whole step is skipped when found_inf[0] != 0)
//   Adam  (L2):        g = fma(wd, w, g)
//   AdamW (decoupled): w = w * float(1 - lr * wd)
//   m = lerp(m, g, float(1 - beta1))                (ATen's two-branch lerp: fma(b1', g - m, m) or fma(-(g - m), 1 - b1', g))
//   v = v * float(beta2);  v = fma(float(1 - beta2), g * g, v)
//   denom = sqrt(v) * (1 / float(bc2_sqrt)) + eps   (ATen divides a tensor by a scalar as a multiply by the scalar's reciprocal)
//   w = fma(float(-step_size), m / denom, w);  w16 = round(w)
// The same kernel updates plain fp32 parameters (BN, biases): no 16-bit copy, fp32 gradient.
#include "rn_multi.hpp"

namespace {

constexpr int ADAM_MAX_TENSORS = 40;          // 40 x 48 B: the size of SgdTable's 48 x 40 B

// the device block, double[RN_ADAM_HPARAMS] (include/retinanet_hip.h)
enum { HP_LR = 0, HP_BETA1, HP_BETA2, HP_EPS, HP_WD, HP_STEP, HP_STEP_SIZE, HP_BC2_SQRT };

struct AdamTable {
    float *master[ADAM_MAX_TENSORS];
    float *m[ADAM_MAX_TENSORS];
    float *v[ADAM_MAX_TENSORS];
    const void *grad[ADAM_MAX_TENSORS];
    void *p16[ADAM_MAX_TENSORS];
    int64_t n[ADAM_MAX_TENSORS];
    const double *hp;
    const float *grad_scale, *found_inf;      // nullable device scalars (torch.amp.GradScaler): 1 / 0
    const float *clip_coef;                   // nullable device scalar: the global-norm clip coefficient (csrc/clip.hip)
    int grad16;                               // gradients of tensors WITH a 16-bit copy are 16-bit as well (else f32)
};

__global__ __launch_bounds__(64) void adam_prologue_kernel(double *__restrict__ hp, const float *__restrict__ found_inf)
{
    if (threadIdx.x != 0) return;
    if (found_inf && *found_inf != 0.0f) return;                 // a skipped step advances nothing (torch's fused Adam)
    const double step = hp[HP_STEP] + 1.0;
    const double bc1 = 1.0 - pow(hp[HP_BETA1], step), bc2 = 1.0 - pow(hp[HP_BETA2], step);
    hp[HP_STEP] = step;
    hp[HP_STEP_SIZE] = hp[HP_LR] / bc1;
    hp[HP_BC2_SQRT] = sqrt(bc2);
}

struct AdamScalars {
    float wd, decay, omb1, omb1c, b2, omb2, inv_bc2, eps, neg_step, inv_scale;
};

__device__ __forceinline__ AdamScalars adam_scalars(const AdamTable &t)
{
    const double *hp = t.hp;
    AdamScalars s;
    s.wd = (float)hp[HP_WD];
    s.decay = (float)(1.0 - hp[HP_LR] * hp[HP_WD]);
    s.omb1 = (float)(1.0 - hp[HP_BETA1]);
    s.omb1c = 1.0f - s.omb1;
    s.b2 = (float)hp[HP_BETA2];
    s.omb2 = (float)(1.0 - hp[HP_BETA2]);
    s.inv_bc2 = 1.0f / (float)hp[HP_BC2_SQRT];
    s.eps = (float)hp[HP_EPS];
    s.neg_step = (float)(-hp[HP_STEP_SIZE]);
    s.inv_scale = t.grad_scale ? 1.0f / *t.grad_scale : 1.0f;
    return s;
}

template <bool DECOUPLED>
__device__ __forceinline__ void adam_one(const AdamScalars &s, const bool decay, float g, float &w, float &m, float &v)
{
    // (each line is one ATen pointwise kernel; those kernels contract their a + b * c into one fma, so these do too)
    if (decay) {
        if (DECOUPLED) w = w * s.decay;
        else g = fmaf(s.wd, w, g);
    }
    m = fabsf(s.omb1) < 0.5f ? fmaf(s.omb1, g - m, m) : fmaf(-(g - m), s.omb1c, g);
    v = v * s.b2;
    v = fmaf(s.omb2, g * g, v);
    const float denom = sqrtf(v) * s.inv_bc2 + s.eps;
    w = fmaf(s.neg_step, m / denom, w);
}

template <bool F16, bool DECOUPLED>
__global__ __launch_bounds__(256) void adam_master_kernel(const AdamTable t)
{
    constexpr int DT = F16 ? RN_F16 : RN_BF16;
    if (t.found_inf && *t.found_inf != 0.0f) return;             // (GradScaler: a non-finite gradient somewhere -> nothing moves)
    const AdamScalars s = adam_scalars(t);
    const float coef = t.clip_coef ? *t.clip_coef : 1.0f;
    const bool decay = s.wd != 0.0f;
    const int ti = blockIdx.y;
    float *__restrict__ w = t.master[ti];
    float *__restrict__ m = t.m[ti];
    float *__restrict__ v = t.v[ti];
    uint16_t *__restrict__ p16 = (uint16_t *)t.p16[ti];
    const bool g16 = p16 && t.grad16;
    const int64_t n = t.n[ti], n4 = n >> 2;
    // 4 elements per thread and iteration: 16-byte accesses on the fp32 arrays, 8-byte on the 16-bit ones (every array starts
    // 16- / 8-byte aligned: checked on the host); the < 4 leftover elements go through the scalar tail below
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n4; q += (int64_t)gridDim.x * 256) {
        rn::f32x4 wv = ((const rn::f32x4 *)w)[q];
        rn::f32x4 mv = ((const rn::f32x4 *)m)[q];
        rn::f32x4 vv = ((const rn::f32x4 *)v)[q];
        const rn::f32x4 gv = rn::load_grad4<DT>(t, ti, q, g16);
        const float g[4] = {gv.x, gv.y, gv.z, gv.w};
        float ww[4] = {wv.x, wv.y, wv.z, wv.w}, mm[4] = {mv.x, mv.y, mv.z, mv.w}, vq[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)                              // unscale, then clip: two fp32 products, before weight decay
            adam_one<DECOUPLED>(s, decay, rn::unscale_clip(g[j], t.grad_scale, s.inv_scale, t.clip_coef, coef), ww[j], mm[j], vq[j]);
        ((rn::f32x4 *)w)[q] = rn::f32x4{ww[0], ww[1], ww[2], ww[3]};
        ((rn::f32x4 *)m)[q] = rn::f32x4{mm[0], mm[1], mm[2], mm[3]};
        ((rn::f32x4 *)v)[q] = rn::f32x4{vq[0], vq[1], vq[2], vq[3]};
        if (p16) rn::store16x4<DT>(p16, q, ww);
    }
    if (blockIdx.x == 0) {                                       // < 4 leftover elements
        const int64_t i = n4 * 4 + threadIdx.x;
        if (threadIdx.x < 4 && i < n) {
            float wi = w[i], mi = m[i], vi = v[i];
            const float g = rn::unscale_clip(rn::load_grad1<DT>(t, ti, i, g16), t.grad_scale, s.inv_scale, t.clip_coef, coef);
            adam_one<DECOUPLED>(s, decay, g, wi, mi, vi);
            w[i] = wi; m[i] = mi; v[i] = vi;
            if (p16) p16[i] = rn::mma<DT>::dn(wi);
        }
    }
}

__global__ __launch_bounds__(64) void adam_hparams_set_kernel(double *__restrict__ hp, const double lr, const double beta1, const double beta2,
                                                              const double eps, const double wd, const double step)
{
    if (threadIdx.x != 0) return;
    hp[HP_LR] = lr; hp[HP_BETA1] = beta1; hp[HP_BETA2] = beta2; hp[HP_EPS] = eps; hp[HP_WD] = wd;
    if (step >= 0.0) hp[HP_STEP] = step;
}

}  // namespace

RN_API int rn_adam_hparams_set(double *hparams, double lr, double beta1, double beta2, double eps, double weight_decay, double step, void *stream)
{
    if (!hparams) return RN_EINVAL;
    if (!rn::aligned(hparams, 8)) return RN_EALIGN;
    hipLaunchKernelGGL(adam_hparams_set_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, hparams, lr, beta1, beta2, eps, weight_decay, step);
    RN_LAUNCH_CHECK();
    return RN_OK;
}

RN_API int rn_adam_master_step(float *const *masters, float *const *exp_avgs, float *const *exp_avg_sqs, const void *const *grads,
                               void *const *params16, const int64_t *numels, int n_tensors, int grads16, int dtype16, int decoupled,
                               double *hparams, const float *grad_scale, const float *found_inf, const float *clip_coef, void *stream)
{
    if (dtype16 != RN_BF16 && dtype16 != RN_F16) return RN_EUNSUPPORTED;
    if (!masters || !exp_avgs || !exp_avg_sqs || !grads || !params16 || !numels || !hparams || n_tensors < 0) return RN_EINVAL;
    if (!rn::aligned(hparams, 8)) return RN_EALIGN;
    const int rc = rn::check_step_tensors<2>(masters, {exp_avgs, exp_avg_sqs}, true, grads, params16, numels, n_tensors, grads16, 8);
    if (rc != RN_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(adam_prologue_kernel, dim3(1), dim3(64), 0, st, hparams, found_inf);
    RN_LAUNCH_CHECK();
    for (int base = 0; base < n_tensors; base += ADAM_MAX_TENSORS) {
        AdamTable t;
        const int cnt = (n_tensors - base) < ADAM_MAX_TENSORS ? (n_tensors - base) : ADAM_MAX_TENSORS;
        for (int i = 0; i < cnt; ++i) {
            t.master[i] = masters[base + i]; t.m[i] = exp_avgs[base + i]; t.v[i] = exp_avg_sqs[base + i];
            t.grad[i] = grads[base + i]; t.p16[i] = params16[base + i]; t.n[i] = numels[base + i];
        }
        t.hp = hparams; t.grad_scale = grad_scale; t.found_inf = found_inf; t.clip_coef = clip_coef; t.grad16 = grads16;
        const dim3 grid = rn::step_grid(t.n, cnt);
        if (dtype16 == RN_F16) {
            if (decoupled) hipLaunchKernelGGL((adam_master_kernel<true, true>), grid, dim3(256), 0, st, t);
            else hipLaunchKernelGGL((adam_master_kernel<true, false>), grid, dim3(256), 0, st, t);
        } else {
            if (decoupled) hipLaunchKernelGGL((adam_master_kernel<false, true>), grid, dim3(256), 0, st, t);
            else hipLaunchKernelGGL((adam_master_kernel<false, false>), grid, dim3(256), 0, st, t);
        }
        RN_LAUNCH_CHECK();
    }
    return RN_OK;
}
