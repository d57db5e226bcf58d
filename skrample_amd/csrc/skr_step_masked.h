// What the masked step (skr_step_masked.hip) and its backward (masked_bwd_k1 of skr_step_backward.hip) share: the load of a lane's mask values.
// (The index arithmetic in front of it is stated in each of the two kernel templates.  As a shared function, however little of it the function
//  holds, it is simplified on its own before it is inlined, apart from the Philox block numbers that share its terms in the forward
//  kernel, and some forward instantiations then come out with other instructions or registers.)
#pragma once
#include "skr_step_common.h"

namespace skr {

// The lane's 8 mask values, at elements m0.. and m1.. of the sample's mask (two groups of 4; consecutive without the tile layout).
// Plain loads, not the operands' non-temporal ones: a (1,H,W) mask is read again by every channel of the sample.
template <typename T>
__device__ __forceinline__ Raw<T> load_mask8(const void* base, int64_t m0, int64_t m1) {
  Raw<T> r;
  if constexpr (sizeof(T) == 2) {
    r.q = *reinterpret_cast<const u32x4_t*>(reinterpret_cast<const uint16_t*>(base) + m0);  // (m1 == m0 + 4: one 16-byte access)
  } else {
    r.q[0] = *reinterpret_cast<const f32x4_t*>(reinterpret_cast<const float*>(base) + m0);
    r.q[1] = *reinterpret_cast<const f32x4_t*>(reinterpret_cast<const float*>(base) + m1);
  }
  return r;
}

// What the entry checks of a masked launch leave behind for its launcher.
struct MaskedLaunch {
  bool noise;      // the launch may draw: the plan's zeta0 decides for the kernarg form, noise_mode alone for the row forms (the row's zeta0 is data)
  bool one_trip;   // the one-trip vector kernel covers it (the row forms have no other)
  int64_t chunks;  // 2048-element chunks of the launch, and
  int bps_shift;   // chunks per sample as the kernels take them (sample_of); both set when one_trip
};

// every check of a masked launch behind its NULL tests (skr_step_masked.hip); also asked by skr_step_launch_masked_channels_last
int masked_prepare(const skr_step_plan& p, const skr_step_mask& mk, const void* const* inputs, void* out, const uint64_t* seeds_dev, int64_t numel,
                   bool rows, MaskedLaunch* launch);

}  // namespace skr
