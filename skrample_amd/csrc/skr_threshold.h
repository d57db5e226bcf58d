// What the statistic of dynamic thresholding (skr_threshold.hip) and the thresholded step (skr_step_thresholded.hip) share: the data
// prediction x0 and the clipped, normalised prediction p, one rounded fp32 operation at a time (include/skrample_hip.h,
// skr_threshold_scale).  One body each, so that the statistic selects among exactly the values the step clips.
#pragma once
#include "skr_step_guided.h"

namespace skr {

// x0 = rn32( rn32(a * x) + rn32(b * o) ): three separate fp32 operations, each result pinned in a register of its own so that nothing
// is contracted into an fma or paired into a packed instruction (see guided_value, skr_step_guided.h)
__device__ __forceinline__ float x0_value(float a, float x, float b, float o) {
  float ax = mul_(a, x);
  asm("" : "+v"(ax));
  float bo = mul_(b, o);
  asm("" : "+v"(bo));
  float r = add_(ax, bo);
  asm("" : "+v"(r));
  return r;
}

// p = rn_T( min(max(x0, -s), s) / s ): comparisons, not fmin / fmax, so that a NaN x0 stays one and a NaN s makes every p of its sample
// one; an IEEE fp32 division
template <typename T>
__device__ __forceinline__ float thresholded_value(float x0, float s) {
  float c = x0 < -s ? -s : x0;
  c = c > s ? s : c;
  float p = div_(c, s);
  asm("" : "+v"(p));
  return rnd<T>(p);
}

// |x0| as the 31 bits it orders by, and whether x0 is a NaN (counted on the side, never selected among)
__device__ __forceinline__ uint32_t magnitude_bits(float x0) { return __builtin_bit_cast(uint32_t, x0) & 0x7fffffffu; }
__device__ __forceinline__ bool magnitude_is_nan(uint32_t m) { return m > 0x7f800000u; }

}  // namespace skr
