// What the guided step (skr_step_guided.hip) and its row forms (skr_step_guided_rows.hip) share: the guided value, one rounded operation at
// a time, and the entry checks of a guided launch.
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
int guided_prepare(const skr_step_plan& p, const skr_step_guidance& gd, const void* const* inputs, void* out, const uint64_t* seeds_dev, int64_t numel,
                   bool rows, GuidedLaunch* launch);

}  // namespace skr
