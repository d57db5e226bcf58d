// What the guided step in all its forms (skr_step_guided.hip) and the statistic of rescaled guidance (skr_guidance_stats.hip,
// skr_guidance_stats_rows.hip) share: the guided value and its rescaled twin, one rounded operation at a time, and torch's fp16 tail rule.
#pragma once
#include "skr_step_common.h"

namespace skr {

// an individually rounded add: the twin of sub_ / mul_ (skr_step_common.h), contraction off so that no neighbour fuses with it
__device__ __forceinline__ float add_(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ double add_(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}

// torch's  uncond + g * (cond - uncond)  on tensors of dtype T: three ops in fp32, each result rounded to fp32 and then to T.
// Each fp32 result is pinned in a register of its own: three plain instructions per element, neither fused nor paired into packed ones
// (a packed fp32 instruction issues at 1.75x a plain one on gfx950, and the shuffles that line its operands up cost more than it saves).
template <typename T>
__device__ __forceinline__ float guided_value(float u, float c, float g) {
  float d = sub_(c, u);
  asm("" : "+v"(d));
  d = rnd<T>(d);
  float m = mul_(g, d);
  asm("" : "+v"(m));
  m = rnd<T>(m);
  float p = add_(u, m);
  asm("" : "+v"(p));
  return rnd<T>(p);
}

// diffusers' rescale_noise_cfg of the guided value p with the sample's factor r: the four torch ops behind the guided value, one rounded operation at a time, each fp32 result pinned in a register of its own (neither
// fused nor paired into packed instructions: see guided_value)
template <typename T>
__device__ __forceinline__ float rescaled_value(float p, float r, float phi, float psi) {
  float resc = mul_(p, r);
  asm("" : "+v"(resc));
  resc = rnd<T>(resc);
  float a = mul_(phi, resc);
  asm("" : "+v"(a));
  a = rnd<T>(a);
  float b = mul_(psi, p);
  asm("" : "+v"(b));
  b = rnd<T>(b);
  float q = add_(a, b);
  asm("" : "+v"(q));
  return rnd<T>(q);
}

// fp16 elements of the partial last block of torch's vectorised elementwise kernel (TORCH_TAIL below).  Its compiler fuses the scalar
// multiply with the conversion there (v_fma_mixlo_f16), so  g * d  is rounded ONCE, from the exact product, where the whole blocks round
// the fp32 product again.  (d is an fp16 value and g an fp32 one: the product has up to 35 significant bits.  c - u and u + m are sums
// of two fp16 values, for which the second rounding never changes the result.)  The single rounding is made of plain operations: the
// fp32 product is moved to its odd neighbour when it is inexact and even, after which the rounding to fp16 cannot meet a false tie.
__device__ __forceinline__ float mul_once_f16(float g, float d) {
  float m = mul_(g, d);
  asm("" : "+v"(m));
  const float err = fma_(g, d, -m);  // exact: what the fp32 rounding dropped
  uint32_t b = __builtin_bit_cast(uint32_t, m);
  const bool finite_nonzero = (b & 0x7f800000u) != 0x7f800000u && (b << 1) != 0;
  if (finite_nonzero && err != 0.f && (b & 1u) == 0) b += ((err > 0.f) == (m > 0.f)) ? 1u : 0xffffffffu;
  return rnd<f16_t>(__builtin_bit_cast(float, b));
}
__device__ __forceinline__ float guided_value_f16_tail(float u, float c, float g) {
  float d = sub_(c, u);
  asm("" : "+v"(d));
  d = rnd<f16_t>(d);
  const float m = mul_once_f16(g, d);
  float p = add_(u, m);
  asm("" : "+v"(p));
  return rnd<f16_t>(p);
}
// The rescaled value there: the two scalar products are rounded once (p * r is exact in fp32, a + b is a sum of two fp16 values: neither
// is changed by its second rounding).  Measured against torch on the device: the fused multiply-and-convert of that block is a
// multiply-ADD with +0 (v_fma_mixlo_f16 k, x, 0), so a product that is exactly zero comes out as +0 whatever its sign -- (-0) + (+0) = +0
// -- while a product that only underflows in the rounding keeps its sign.  It shows where phi or psi is 0: psi * p = 0 * (negative p) is
// +0 there and -0 in the whole blocks, and a + b = (-0) + that differs in the sign bit.
__device__ __forceinline__ float mul_once_f16_add0(float k, float x) {
  const float m = mul_once_f16(k, x);
  return (k == 0.f || x == 0.f) && m == 0.f ? 0.f : m;  // (0 * inf is NaN and stays one)
}
__device__ __forceinline__ float rescaled_value_f16_tail(float p, float r, float phi, float psi) {
  float resc = mul_(p, r);
  asm("" : "+v"(resc));
  resc = rnd<f16_t>(resc);
  const float a = mul_once_f16_add0(phi, resc), b = mul_once_f16_add0(psi, p);
  float q = add_(a, b);
  asm("" : "+v"(q));
  return rnd<f16_t>(q);
}
// the block of that torch kernel for 16-bit tensors on gfx950 (256 threads of 8 elements): elements from the last multiple of it on are
// its tail.  The one-trip kernel's chunk has the same size, so a tensor of whole chunks has no tail.
constexpr int64_t TORCH_TAIL = 2048;
static_assert(TORCH_TAIL == (int64_t)BLOCK * VEC, "whole chunks must be whole blocks of torch's kernel: the one-trip kernel has no tail path");

__device__ __forceinline__ double guide_d(double u, double c, double g) { return add_(u, mul_(g, sub_(c, u))); }
__device__ __forceinline__ double rescaled_d(double p, double r, double phi, double psi) { return add_(mul_(phi, mul_(p, r)), mul_(psi, p)); }

}  // namespace skr
