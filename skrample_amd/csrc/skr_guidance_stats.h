// What the statistic of rescaled guidance (skr_guidance_stats.hip) and its row and rolling forms (skr_guidance_stats_rows.hip) share: the summation
// order documented in include/skrample_hip.h (skr_guidance_rescale_factor) -- a lane's eight elements in index order, the shuffle tree
// o = 32 .. 1, the four waves as ((w0 + w1) + w2) + w3 -- and the last operations behind the sums.  One body, so that a sample has the
// same bits through either entry.
#pragma once
#include "skr_step_guided.h"

namespace skr {

constexpr int64_t SPAN = (int64_t)BLOCK * VEC;  // elements per stage-1 workgroup; 4 doubles of partials each
static_assert(SPAN == 2048, "the span is part of the documented summation order (SKR_GUIDANCE_PARTIALS)");

// the guided value of element e of the launch in the op-math type M of T
template <typename T, typename M>
__device__ __forceinline__ M stat_guided(M u, M c, M g, int64_t e, int64_t tail_from) {
  if constexpr (std::is_same<T, double>::value) return guide_d(u, c, g);
  else if constexpr (std::is_same<T, f16_t>::value) return e >= tail_from ? guided_value_f16_tail(u, c, g) : guided_value<f16_t>(u, c, g);
  else return guided_value<T>(u, c, g);
}

template <typename T, typename M>
__device__ __forceinline__ M stat_load(const void* base, int64_t e) {
  if constexpr (std::is_same<T, double>::value) return reinterpret_cast<const double*>(base)[e];
  else return load_scalar<T>(base, e);
}

// the first element of a 16-byte aligned run of T, read as one dword from a uniform address (the pivots of the row and rolling forms)
template <typename T>
__device__ __forceinline__ float first_of(const char* at) {
  const uint32_t w = *reinterpret_cast<const uint32_t*>(at);
  if constexpr (std::is_same<T, bf16_t>::value) return __uint_as_float(w << 16);
  else if constexpr (std::is_same<T, f16_t>::value) return (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xFFFFu));
  else return __uint_as_float(w);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);  // (a double shuffle is two 32-bit moves)
  return v;
}

// Stage 1 behind the loads: this lane's elements `at .. at + 7` of the span that starts at element `start` of the launch, the first `len`
// of the span counted; the workgroup's four sums go to partials4[0..3].  WHOLE: len == SPAN and no element lies in torch's fp16 tail
// (a launch of whole spans), so neither test is made.
template <typename T, typename M, bool WHOLE>
__device__ __forceinline__ void span_sums(const M (&u)[VEC], const M (&c)[VEC], M g, double kc, double kp, int at, int len, int64_t start, int64_t tail_from,
                                          double* partials4) {
  double s1c = 0.0, s2c = 0.0, s1p = 0.0, s2p = 0.0;
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    if (WHOLE || at + i < len) {
      M p;
      if constexpr (WHOLE && !std::is_same<T, double>::value) p = guided_value<T>(u[i], c[i], g);
      else p = stat_guided<T, M>(u[i], c[i], g, start + at + i, tail_from);
      const double dc = sub_((double)c[i], kc);
      const double dp = sub_((double)p, kp);
      s1c = add_(s1c, dc);
      s2c = fma_(dc, dc, s2c);
      s1p = add_(s1p, dp);
      s2p = fma_(dp, dp, s2p);
    }
  }

  __shared__ double red[4][4];
  s1c = wave_sum(s1c), s2c = wave_sum(s2c), s1p = wave_sum(s1p), s2p = wave_sum(s2p);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][wave] = s1c; red[1][wave] = s2c; red[2][wave] = s1p; red[3][wave] = s2p; }
  __syncthreads();
  if (threadIdx.x < 4) {
    const double* r = red[threadIdx.x];
    partials4[threadIdx.x] = ((r[0] + r[1]) + r[2]) + r[3];
  }
}

__device__ __forceinline__ double unbiased_std(double s1, double s2, double n) {
  const double var = div_(sub_(s2, div_(mul_(s1, s1), n)), sub_(n, 1.0));
  return __dsqrt_rn(var > 0.0 || var != var ? var : 0.0);  // max(var, 0); a NaN stays one
}

// Stage 2 behind the sums (one lane): the two standard deviations and the factor of sample `smp`
template <typename T>
__device__ __forceinline__ void stats_finish(double s1c, double s2c, double s1p, double s2p, int64_t sample_numel, int64_t smp, void* factor, double* stats) {
  using M = typename OpMath<T>::type;
  const double n = (double)sample_numel;
  const double std_c = unbiased_std(s1c, s2c, n), std_p = unbiased_std(s1p, s2p, n);
  if (stats != nullptr) { stats[2 * smp] = std_c; stats[2 * smp + 1] = std_p; }
  if constexpr (std::is_same<T, double>::value) {
    reinterpret_cast<double*>(factor)[smp] = div_(std_c, std_p);
  } else {
    // torch: std() of a T tensor is its fp32 result rounded to T; T / T is an fp32 division rounded to T
    const M r = div_(rnd<T>((M)std_c), rnd<T>((M)std_p));
    store_scalar<T, M>(factor, smp, r);
  }
}

}  // namespace skr
