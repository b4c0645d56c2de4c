// The counter-based uniform behind every train-time draw (augment.hip, affine.hip): splitmix64's finalizer on (seed, counter, b),
// mapped to [0, 1) with 24 bits -- exact in fp32.  include/retinanet_hip.h (rn_hflip_draw) states it; augment.hflip_u restates it.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

static __device__ __forceinline__ float hflip_u(const uint64_t seed, const int64_t counter, const int b)
{
    uint64_t z = seed ^ ((uint64_t)counter * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)(b + 1) * 0xD1B54A32D192ED03ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (float)(uint32_t)(z >> 40) * 0x1p-24f;
}

// counter += 1 as a launch of its own, <<<1, DRAW_ADVANCE_BLOCK>>>, for a draw whose every wave reads the counter: launched LAST, so
// stream order puts it behind every wave of the draw.  (One wave: every lane reads the counter, in program order before lane 0's
// store.)  ``counter``: the address of a state block's counter field.
constexpr int DRAW_ADVANCE_BLOCK = 64;

static __global__ __launch_bounds__(DRAW_ADVANCE_BLOCK) void draw_advance_kernel(int64_t *counter)
{
    const int64_t c = *counter;
    if (threadIdx.x == 0) *counter = c + 1;
}
