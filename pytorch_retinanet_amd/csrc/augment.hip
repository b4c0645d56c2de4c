// Train-time augmentation decisions drawn on the device (augment.RandomHorizontalFlip).
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
#include "rn_common.hpp"

namespace {

constexpr int HF_BLOCK = 64;        // one wave: the counter update needs no barrier across waves

__device__ __forceinline__ float hflip_u(const uint64_t seed, const int64_t counter, const int b)
{
    uint64_t z = seed ^ ((uint64_t)counter * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)(b + 1) * 0xD1B54A32D192ED03ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (float)(uint32_t)(z >> 40) * 0x1p-24f;
}

__global__ __launch_bounds__(HF_BLOCK) void hflip_draw_kernel(rn_hflip_state *st, const int B, uint8_t *__restrict__ flags)
{
    const uint64_t seed = st->seed;
    const int64_t counter = st->counter;
    const float p = st->p;
    for (int b = (int)threadIdx.x; b < B; b += HF_BLOCK) flags[b] = hflip_u(seed, counter, b) < p ? 1 : 0;
    if (threadIdx.x == 0) st->counter = counter + 1;
}

}  // namespace

RN_API int rn_hflip_draw(rn_hflip_state *state, int B, uint8_t *flags, void *stream)
{
    if (!state || !flags || B <= 0) return RN_EINVAL;
    if (!rn::aligned(state, 8)) return RN_EALIGN;
    hipLaunchKernelGGL(hflip_draw_kernel, dim3(1), dim3(HF_BLOCK), 0, (hipStream_t)stream, state, B, flags);
    RN_LAUNCH_CHECK();
    return RN_OK;
}
