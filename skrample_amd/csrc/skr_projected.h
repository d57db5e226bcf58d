// What the statistic of adaptive projected guidance (skr_projected_coef.hip), its step (skr_step_projected.hip) and the row forms of both
// (skr_projected_rows.hip, skr_step_projected_rows.hip) share: the difference d and the projected prediction p of include/skrample_hip.h
// (skr_projected_guidance_coef), one rounded fp32 operation at a time.  Each fp32 result is pinned in a register of its own, as in
// guided_value (skr_step_guided.h): neither fused with a neighbour nor paired into a packed instruction, and for fp16 never folded into a
// multiply-and-convert.  Behind them the statistic's sums -- a lane's eight elements, the workgroup's three partials, a sample's spans --
// and the coefficient arithmetic: one body each, so that a sample has the same bits through the direct entry and through a row.
#pragma once
#include "skr_guidance_stats.h"

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

// Stage 1 behind d: this lane's elements `at .. at + 7` of its span, the first `len` of the span counted (`whole`: all of them), added in
// index order to three doubles that start at zero, each product formed in double by the fma that adds it; the shuffle tree, then the four
// waves as ((w0 + w1) + w2) + w3; the workgroup's Sdd, Sdc, Scc go to partials4[0..2].
__device__ __forceinline__ void projected_span_sums(const float (&d)[VEC], const float (&c)[VEC], bool whole, int at, int len, double* partials4) {
  double sdd = 0.0, sdc = 0.0, scc = 0.0;
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    if (whole || at + i < len) {
      const double dd = (double)d[i], cc = (double)c[i];
      sdd = fma_(dd, dd, sdd);
      sdc = fma_(dd, cc, sdc);
      scc = fma_(cc, cc, scc);
    }
  }
  __shared__ double red[3][4];
  sdd = wave_sum(sdd), sdc = wave_sum(sdc), scc = wave_sum(scc);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][wave] = sdd; red[1][wave] = sdc; red[2][wave] = scc; }
  __syncthreads();
  if (threadIdx.x < 3) {
    const double* r = red[threadIdx.x];
    partials4[threadIdx.x] = ((r[0] + r[1]) + r[2]) + r[3];
  }
}

// Stage 2, one wave per sample: lanes 0..2 each sum one quantity over the sample's spans in index order from zero; every lane gets the three
__device__ __forceinline__ void projected_sample_sums(const double* partials, int64_t smp, uint32_t spans, double& sdd, double& sdc, double& scc) {
  double acc = 0.0;
  if (threadIdx.x < 3) {
    const double* p = partials + smp * spans * 4 + threadIdx.x;
    for (uint32_t j = 0; j < spans; ++j) acc += p[(int64_t)j * 4];
  }
  sdd = __shfl(acc, 0), sdc = __shfl(acc, 1), scc = __shfl(acc, 2);
}

// Stage 2 behind the sums (one lane): the two coefficients of sample `smp`, in double, each narrowed once on store
__device__ __forceinline__ void projected_finish(double sdd, double sdc, double scc, double g, double eta, double r, int64_t smp, float* coef, double* stats) {
  if (stats != nullptr) { stats[3 * smp] = sdd; stats[3 * smp + 1] = sdc; stats[3 * smp + 2] = scc; }
  const double norm = __dsqrt_rn(sdd);
  const double scale = (r > 0.0 && norm > r) ? div_(r, norm) : 1.0;
  const double root = __dsqrt_rn(scc), den = root > 1e-12 ? root : 1e-12;
  const double alpha = div_(sdc, mul_(den, den));
  const double A = mul_(sub_(g, 1.0), scale);
  const double B = sub_(1.0, mul_(mul_(A, sub_(1.0, eta)), alpha));
  coef[2 * smp] = (float)A;
  coef[2 * smp + 1] = (float)B;
}

}  // namespace skr
