// The statistic of adaptive projected guidance (include/skrample_hip.h, skr_projected_guidance_coef): per sample the three dot products
// Sdd, Sdc, Scc of the difference d = rn_T((c - u) + beta * m) and cond, and from them the two coefficients A_s, B_s with which
// skr_projected_guided_step_launch forms p = rn_T(B_s c + A_s d).  d is formed in registers; with a momentum buffer it is stored back in
// place -- the buffer IS the running average, and the step reads it instead of uncond.
//
// Two stages, fixed order, double accumulation, no atomics: the summation order is that of skr_guidance_rescale_factor (skr_guidance_stats.h).
//   stage 1 (projected_spans<T, MODE>): one workgroup per 2048-element span of a sample, lane t owning the span's elements 8 t .. 8 t + 7
//     whichever way they are read: a whole, 16-byte aligned span with one (16-bit) or two (fp32) 16-byte non-temporal loads per operand
//     and lane -- u, c and m all issued before the first use --, any other span element by element with a bounds test.  The lane that
//     read m stores d over it.  Products are formed in double by the fma that adds them: exact, so only the additions round.
//   stage 2 (projected_final): one wave per sample; lanes 0..2 each sum one quantity over the sample's spans in index order, lane 0
//     finishes in double and narrows each coefficient once.
// MODE: 0 no buffer (d = rn_T(c - u), nothing stored); 1 a buffer without momentum (the same d, stored); 2 momentum (m read, d stored).
#include "skr_projected.h"
#include "skr_device.h"

namespace skr {

template <typename T, int MODE>
__global__ __launch_bounds__(BLOCK) void projected_spans(const void* uncond, const void* cond, void* mom, float beta, int64_t sample_numel, uint32_t spans,
                                                         double* partials) {
  const uint32_t smp = blockIdx.x / spans, j = blockIdx.x - smp * spans;
  const int64_t first = (int64_t)smp * sample_numel, start = first + (int64_t)j * SPAN;
  const int64_t left = first + sample_numel - start;  // elements of the sample from this span on: >= 1
  const int len = left < SPAN ? (int)left : (int)SPAN;
  const int at = (int)threadIdx.x * VEC;  // this lane's first element within the span

  float c[VEC], d[VEC];
  const bool whole = len == SPAN && ((uint64_t)start * sizeof(T)) % 16 == 0;  // (uniform; the base pointers are 16-byte aligned)
  if (whole) {
    const int64_t off = start * (int64_t)sizeof(T);
    const Raw<T> ru = load_raw<T, false>(reinterpret_cast<const char*>(uncond) + off, threadIdx.x);
    const Raw<T> rc = load_raw<T, false>(reinterpret_cast<const char*>(cond) + off, threadIdx.x);
    float u[VEC];
    if constexpr (MODE == 2) {
      const Raw<T> rm = load_raw<T, false>(reinterpret_cast<const char*>(mom) + off, threadIdx.x);
      float m[VEC];
      widen<T, float>(ru, u);
      widen<T, float>(rc, c);
      widen<T, float>(rm, m);
#pragma unroll
      for (int i = 0; i < VEC; ++i) d[i] = projected_diff<T>(u[i], c[i], beta, m[i]);
    } else {
      widen<T, float>(ru, u);
      widen<T, float>(rc, c);
#pragma unroll
      for (int i = 0; i < VEC; ++i) d[i] = projected_diff<T>(u[i], c[i]);
    }
    if constexpr (MODE != 0) store8<T, float, false>(reinterpret_cast<char*>(mom) + off, threadIdx.x, d);  // (d is a value of T: the store's rounding is exact)
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const bool in = at + i < len;
      const int64_t e = start + at + i;
      c[i] = d[i] = 0.f;
      if (in) {
        const float u = load_scalar<T>(uncond, e);
        c[i] = load_scalar<T>(cond, e);
        if constexpr (MODE == 2) d[i] = projected_diff<T>(u, c[i], beta, load_scalar<T>(mom, e));
        else d[i] = projected_diff<T>(u, c[i]);
        if constexpr (MODE != 0) store_scalar<T, float>(mom, e, d[i]);
      }
    }
  }

  projected_span_sums(d, c, whole, at, len, partials + (int64_t)blockIdx.x * 4);
}

__global__ __launch_bounds__(64) void projected_final(const double* partials, uint32_t spans, double g, double eta, double r, float* coef, double* stats) {
  const int64_t smp = blockIdx.x;
  double sdd, sdc, scc;
  projected_sample_sums(partials, smp, spans, sdd, sdc, scc);
  if (threadIdx.x != 0) return;
  projected_finish(sdd, sdc, scc, g, eta, r, smp, coef, stats);
}

}  // namespace skr

extern "C" int skr_projected_guidance_coef(const void* uncond, const void* cond, void* momentum_buf, int32_t dtype, double guidance_scale, double eta,
                                           double norm_threshold, double momentum, int64_t numel, int64_t sample_numel, float* coef_dev, double* stats_dev,
                                           double* partials_dev, void* stream) {
  using namespace skr;
  if (!uncond || !cond || !coef_dev || !partials_dev || (momentum != 0.0 && !momentum_buf)) return SKR_ERR_NULL;
  if (numel < 0 || sample_numel < 2 || numel % sample_numel != 0) return SKR_ERR_SHAPE;
  if (numel == 0) return SKR_OK;
  if (!aligned16(uncond) || !aligned16(cond) || !aligned16(momentum_buf) || (reinterpret_cast<uintptr_t>(coef_dev) & 3u) != 0) return SKR_ERR_ALIGN;
  if (!tensor_dtype(dtype) || dtype == SKR_F64) return SKR_ERR_DTYPE;
  const int64_t samples = numel / sample_numel, spans = (sample_numel + SPAN - 1) / SPAN;
  if (spans > 0x7fffffffll || samples > 0x7fffffffll / spans) return SKR_ERR_UNSUPPORTED;  // one workgroup per span: the grid's x extent
  DeviceGuard device_guard(coef_dev);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int mode = momentum != 0.0 ? 2 : (momentum_buf != nullptr ? 1 : 0);
  with_step_type<false>(dtype, [&](auto tt) {
    with_count<0, 2>(mode, [&](auto m) {
      using T = typename decltype(tt)::type;
      hipLaunchKernelGGL((projected_spans<T, decltype(m)::value>), dim3((unsigned)(samples * spans)), dim3(BLOCK), 0, s, uncond, cond, momentum_buf, (float)momentum,
                         sample_numel, (uint32_t)spans, partials_dev);
    });
  });
  hipLaunchKernelGGL(projected_final, dim3((unsigned)samples), dim3(64), 0, s, (const double*)partials_dev, (uint32_t)spans, guidance_scale, eta, norm_threshold,
                     coef_dev, stats_dev);
  return finish_launch();
}
