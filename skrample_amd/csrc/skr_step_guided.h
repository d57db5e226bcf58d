// What the guided step (skr_step_guided.hip), its row forms (skr_step_guided_rows.hip), the rescaled step (skr_step_guided_rescaled.hip) and
// its statistic (skr_guidance_stats.hip) share: the guided value, one rounded operation at a time, torch's fp16 tail rule, and the entry
// checks of a guided launch.
#pragma once
#include "skr_step_common.h"

namespace skr {

constexpr int guided_kmax(int k) { return k <= 4 ? 4 : (k <= 8 ? 8 : (k <= 12 ? 12 : 16)); }

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

// diffusers' rescale_noise_cfg of the guided value p with the sample's factor r (skr_step_guided_rescaled.hip and its rolling form): the
// four torch ops behind the guided value, one rounded operation at a time, each fp32 result pinned in a register of its own (neither
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
// the block of that torch kernel for 16-bit tensors on gfx950 (256 threads of 8 elements): elements from the last multiple of it on are
// its tail.  The one-trip kernel's chunk has the same size, so a tensor of whole chunks has no tail.
constexpr int64_t TORCH_TAIL = 2048;
static_assert(TORCH_TAIL == (int64_t)BLOCK * VEC, "whole chunks must be whole blocks of torch's kernel: the one-trip kernel has no tail path");

__device__ __forceinline__ double guide_d(double u, double c, double g) { return add_(u, mul_(g, sub_(c, u))); }

// the rolling forms (skr_step_guided_rolling.hip, skr_step_guided_rescaled_rolling.hip): an operand other than the slot is present unless
// its coef0 is exactly zero (either sign): decided on the row's double, in SGPRs
__device__ __forceinline__ bool guided_row_has(const skr_step_row* row, int j) { return (__builtin_bit_cast(uint64_t, row->coef0[j]) << 1) != 0; }

// What the entry checks of a guided launch leave behind for its launcher.
struct GuidedLaunch {
  bool step_out;   // the launch has a step output (out0_dtype is a dtype): false is the guidance-only form
  bool noise;      // the launch may draw: the plan's zeta0 decides for the kernarg form, noise_mode alone for the row forms (the row's zeta0 is data)
  bool one_trip;   // the one-trip vector kernel covers it (the row forms have no other)
  int64_t chunks;  // 2048-element chunks of the launch, and
  int bps_shift;   // chunks per sample as the kernels take them (sample_of; 0 for a launch that does not draw); both set when one_trip
  int32_t dtype_b, dtype_g;  // the dtype of group b (group a's when that group is empty) and of the group `slot` lies in
};

// every check of a guided launch behind its NULL plan / guide tests, in skr_step_launch_guided's order and with its codes (skr_step_guided.hip);
// `rows`: for a row form, whose plan scalars are ignored.  SKR_OK with numel == 0 means "nothing to do".
// `rescale` (skr_step_launch_guided_rescaled alone): what it adds is checked where the like of it stands -- `reserved` beside the
// guide's, the sample size behind that of a launch that draws, factor_dev beside the operands.
int guided_prepare(const skr_step_plan& p, const skr_step_guidance& gd, const void* const* inputs, void* out, const uint64_t* seeds_dev, int64_t numel,
                   bool rows, GuidedLaunch* launch, const skr_step_rescale* rescale = nullptr);

}  // namespace skr
