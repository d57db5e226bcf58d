// What the two translation units of the masked step share (skr_step_masked.hip: the kernarg forms and the general kernel;
// skr_step_masked_rows.hip: the device-resident row forms): the one-trip kernarg, the chunk and mask index helpers, the entry checks.
#pragma once
#include "skr_step_common.h"

namespace skr {

constexpr int masked_kmax(int k) { return k <= 4 ? 4 : (k <= 8 ? 8 : (k <= 12 ? 12 : 16)); }

// Kernarg of the one-trip kernel: what the first instructions need (operand pointers, chunk map) leads, as in OneTripArgs.
template <int KMAX>
struct MaskedArgs {
  const void* in[KMAX];
  const void* mask;
  void* out;
  int32_t xmap_lr;      // log2(run length) of the XCD chunk map
  int32_t bps_shift;    // chunks per sample: log2 when >= 0, minus the count otherwise (see chunk_sample)
  uint32_t mask_numel;  // elements of one sample's mask (a multiple of 8, below 2^31)
  uint32_t mask_stride; // elements between the masks of two samples: mask_numel or 0
  const uint64_t* seeds;
  uint64_t stream0;
  float zeta0;
  float c0[KMAX];
  float c1[KMAX];
};

// chunk -> (sample, chunk within the sample): a shift for a power-of-two number of chunks per sample, else one uniform division
__device__ __forceinline__ void chunk_sample(uint32_t c, int32_t bps_shift, uint32_t& smp, uint32_t& within) {
  if (bps_shift >= 0) { smp = c >> bps_shift; within = c - (smp << bps_shift); }
  else { const uint32_t bps = (uint32_t)(-bps_shift); smp = c / bps; within = c - smp * bps; }
}

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
  bool noise;      // the launch may draw: the plan's zeta0 decides for the kernarg forms, noise_mode alone for the row forms (the row's zeta0 is data)
  bool one_trip;   // the one-trip vector kernel covers it (the row forms have no other)
  int64_t chunks;  // 2048-element chunks of the launch, and
  int bps_shift;   // chunks per sample as the kernels take them (chunk_sample); both set when one_trip
};
// Every check of skr_step_launch_masked behind its plan / mask NULL test, in its order and with its codes; `rows`: for a row entry, whose
// plan scalars are ignored.  SKR_OK with numel == 0 means "nothing to do".  Defined in skr_step_masked.hip.
int masked_prepare(const skr_step_plan& p, const skr_step_mask& mk, const void* const* inputs, void* out, const uint64_t* seeds_dev, int64_t numel,
                   bool rows, MaskedLaunch* launch);

}  // namespace skr
