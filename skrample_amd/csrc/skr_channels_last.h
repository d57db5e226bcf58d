// What the two channels-last step files (skr_step_channels_last.hip, skr_step_masked_channels_last.hip) share: the draw of a lane's 8
// storage elements in their one-trip kernels, and on the host the one-trip geometry and the channel-count dispatch
// (DESIGN.md sections 4.1 and 4.6).
#pragma once
#include "skr_step_common.h"

namespace skr {

// ---- the draw of a lane's 8 storage elements, spread over lane groups -----------------------------------------------------------------
// A sample is stored plane x channels, channel innermost: storage position p is the logical element l(p) = (p % C) * plane + p / C, which
// takes lane l & 3 of Philox block l >> 2.  A Philox block is 4 consecutive pixels of one channel (plane % 4 == 0), and a lane's vector is
//   C = 4   two pixels x 4 channels       C = 8   one pixel x 8 channels       C = 16  half a pixel (8 of its 16 channels)
// so G = C / 2 adjacent lanes own 4 pixels x C channels = C blocks: two per lane, the contiguous kernel's count.  Each lane draws two
// WHOLE blocks (channels ch0 and ch0 + 1 of the group's pixel quad) and the group exchanges normals in registers:
//   C = 8   lane j of 4 draws channels 2j, 2j+1 and needs pixel j of all 8: per block a 4x4 transpose over lane bits 0 and 1
//   C = 16  the 4 lanes that hold the same channel half (lane bit 0) transpose among themselves, over lane bits 1 and 2
//   C = 4   lane j of 2 draws channels 2j, 2j+1 and needs pixels 2j, 2j+1 of all 4: it swaps two normals of each block with its neighbour
// Lane bits 0 and 1 are crossed with DPP quad permutes (full-rate VALU moves), bit 2 with ds_swizzle (the LDS crossbar, no LDS memory).
// The register index a normal lands in depends on the lane, so every exchange is framed by v_cndmask selects: 16 per transpose.
template <int M>
__device__ __forceinline__ float lane_xor(float x) {  // the value of lane ^ M (M = 1, 2, 4; every lane of the wave is active)
  const int i = __builtin_bit_cast(int, x);
  int r;
  if constexpr (M == 1) r = __builtin_amdgcn_update_dpp(i, i, 0xB1, 0xF, 0xF, false);       // quad_perm:[1,0,3,2]
  else if constexpr (M == 2) r = __builtin_amdgcn_update_dpp(i, i, 0x4E, 0xF, 0xF, false);  // quad_perm:[2,3,0,1]
  else r = __builtin_amdgcn_ds_swizzle(i, 0x101F);  // bit-mask mode: and 0x1f, or 0, xor 4
  return __builtin_bit_cast(float, r);
}

// one butterfly stage: lanes that differ in the bit `up` tests exchange a[i + S] (bit clear) for a[i] (bit set)
template <int M, int S>
__device__ __forceinline__ void butterfly(float a[4], bool up, int i) {
  const float keep = up ? a[i + S] : a[i];
  const float got = lane_xor<M>(up ? a[i] : a[i + S]);
  a[i] = up ? got : keep;
  a[i + S] = up ? keep : got;
}
// 4x4 transpose over the four lanes spanned by lane bits M1 (lo) and M2 (hi): a[k] becomes element 2*hi + lo of lane k's a
template <int M1, int M2>
__device__ __forceinline__ void transpose4(float a[4], bool lo, bool hi) {
  butterfly<M1, 1>(a, lo, 0);
  butterfly<M1, 1>(a, lo, 2);
  butterfly<M2, 2>(a, hi, 0);
  butterfly<M2, 2>(a, hi, 1);
}

// The normals of the 8 storage elements of lane-vector `vs` of a sample (t = threadIdx.x: the lane's place in its group is in its low
// bits, BLOCK being a multiple of every group size; quads = plane / 4, the Philox blocks per channel): z[i] is the normal of logical
// element l(8 vs + i).  Every lane of the wave must be active.
template <int C>
__device__ __forceinline__ void cl_draw8(uint64_t seed, uint64_t stream0, uint32_t quads, uint32_t vs, uint32_t t, float z[VEC]) {
  static_assert(C == 4 || C == 8 || C == 16, "lane groups of 2, 4 or 8");
  constexpr int LG = C == 4 ? 1 : (C == 8 ? 2 : 3);  // log2(lanes per group)
  const uint32_t quad = vs >> LG;                    // the group's pixel quad: pixels 4 quad .. 4 quad + 3
  // The lane draws channels ch0 and ch0 + 1 of that quad: ch0 = 2 (t & 1) for C = 4, 2 (t & 3) for C = 8, 8 (t & 1) + 2 ((t >> 1) & 3) for
  // C = 16.  Block ch0 * quads + quad, put together from scalar multiples of `quads` chosen by the lane's bits: a vector multiply here
  // would be one more full-width multiply than the contiguous kernel spends.
  // (sample_numel / 4 fits 32 bits: the host sends larger samples to the general kernel)
  const uint32_t q2 = quads * 2, q4 = quads * 4, q8 = quads * 8;
  uint32_t blk = quad;
  if constexpr (C == 16) blk += ((t & 1) ? q8 : 0u) + ((t & 2) ? q2 : 0u) + ((t & 4) ? q4 : 0u);
  else blk += ((t & 1) ? q2 : 0u) + ((C == 8 && (t & 2)) ? q4 : 0u);
  float za[4], zb[4];
  normal4(seed, stream0, (uint64_t)blk, za);
  normal4(seed, stream0, (uint64_t)(blk + quads), zb);
  if constexpr (C == 4) {
    // storage order of the vector: pixel 2j + pl (pl = 0, 1), channels 0..3; own channels 2j + b, the neighbour's 2(1 - j) + b
    const bool up = (t & 1) != 0;
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
      const float keep_a = up ? za[2 + pl] : za[pl], keep_b = up ? zb[2 + pl] : zb[pl];
      const float got_a = lane_xor<1>(up ? za[pl] : za[2 + pl]), got_b = lane_xor<1>(up ? zb[pl] : zb[2 + pl]);
      z[4 * pl + 0] = up ? got_a : keep_a;
      z[4 * pl + 1] = up ? got_b : keep_b;
      z[4 * pl + 2] = up ? keep_a : got_a;
      z[4 * pl + 3] = up ? keep_b : got_b;
    }
  } else {
    // after the transposes za[k] / zb[k] hold this lane's pixel of the channels lane k of the group drew: storage offsets 2k, 2k + 1
    if constexpr (C == 8) { transpose4<1, 2>(za, (t & 1) != 0, (t & 2) != 0); transpose4<1, 2>(zb, (t & 1) != 0, (t & 2) != 0); }
    else { transpose4<2, 4>(za, (t & 2) != 0, (t & 4) != 0); transpose4<2, 4>(zb, (t & 2) != 0, (t & 4) != 0); }
#pragma unroll
    for (int k = 0; k < 4; ++k) { z[2 * k] = za[k]; z[2 * k + 1] = zb[k]; }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
// What both one-trip kernels take (the header's lists): 1..8 operands and an output of one 16-bit dtype, fp32 arithmetic, C = 4, 8 or 16
// over a plane of whole Philox blocks, launch and sample of whole chunks, chunk numbers that fit 31 bits, a sample of at most
// `sample_max` elements (each entry's own bound).
static inline bool cl_one_trip_geometry(const skr_step_plan& p, const skr_step_layout& l, int64_t numel, int64_t sample_max, int* bps_shift) {
  constexpr int64_t CHUNK = (int64_t)BLOCK * VEC;
  const int32_t t = p.dtype_a;
  if (!g_tune.one_trip || p.acc_f64 || p.n_terms < 1 || p.n_terms > 8) return false;
  if ((t != SKR_BF16 && t != SKR_F16) || (p.n_group_a != p.n_terms && p.dtype_b != t) || p.out0_dtype != t) return false;
  if ((l.channels != 4 && l.channels != 8 && l.channels != 16) || l.plane % 4 != 0) return false;
  if (numel % CHUNK != 0 || numel / CHUNK > 0x7fffffffll || p.sample_numel % CHUNK != 0 || p.sample_numel > sample_max) return false;
  *bps_shift = bps_shift_of(p.sample_numel / CHUNK);
  return true;
}

// f(std::integral_constant<int, C>{}) for the C of 4, 8, 16 that equals channels (cl_one_trip_geometry admits no other)
template <typename F>
static inline void with_channels(int64_t channels, F&& f) {
  if (channels == 4) f(std::integral_constant<int, 4>{});
  else if (channels == 8) f(std::integral_constant<int, 8>{});
  else f(std::integral_constant<int, 16>{});
}

}  // namespace skr
