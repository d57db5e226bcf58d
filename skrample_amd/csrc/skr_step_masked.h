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

}  // namespace skr
