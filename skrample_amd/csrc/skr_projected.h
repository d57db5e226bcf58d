// What the statistic of adaptive projected guidance (skr_projected_coef.hip) and its step (skr_step_projected.hip) share: the difference d
// and the projected prediction p of include/skrample_hip.h (skr_projected_guidance_coef), one rounded fp32 operation at a time.  Each fp32
// result is pinned in a register of its own, as in guided_value (skr_step_guided.h): neither fused with a neighbour nor paired into a
// packed instruction, and for fp16 never folded into a multiply-and-convert.
#pragma once
#include "skr_step_guided.h"

namespace skr {

// d = rn_T(c - u)
template <typename T>
__device__ __forceinline__ float projected_diff(float u, float c) {
  float d = sub_(c, u);
  asm("" : "+v"(d));
  return rnd<T>(d);
}

// d = rn_T( (c - u) + (beta * m) ): the running average of the difference, three separate operations
template <typename T>
__device__ __forceinline__ float projected_diff(float u, float c, float beta, float m) {
  float d = sub_(c, u);
  asm("" : "+v"(d));
  float bm = mul_(beta, m);
  asm("" : "+v"(bm));
  float s = add_(d, bm);
  asm("" : "+v"(s));
  return rnd<T>(s);
}

// p = rn_T( (B * c) + (A * d) ): the two per-sample coefficients of the statistic over cond and the difference
template <typename T>
__device__ __forceinline__ float projected_value(float c, float d, float A, float B) {
  float bc = mul_(B, c);
  asm("" : "+v"(bc));
  float ad = mul_(A, d);
  asm("" : "+v"(ad));
  float p = add_(bc, ad);
  asm("" : "+v"(p));
  return rnd<T>(p);
}

}  // namespace skr
