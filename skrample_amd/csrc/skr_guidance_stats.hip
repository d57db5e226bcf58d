// The statistic of rescaled guidance (include/skrample_hip.h, skr_guidance_rescale_factor): per sample, the unbiased standard deviations of
// cond and of the guided prediction p = rn_T(u + rn_T(g * rn_T(c - u))), and the factor rn_T(std_c / std_p) that
// skr_step_launch_guided_rescaled multiplies p by.  p is never stored: it is recomputed from the two operands, with the bits the step
// launch gives it (guided_value, skr_step_guided.h; the fp16 tail rule by the element's index in the whole launch).
//
// Two stages, fixed order, double accumulation, no atomics (as skr_reduce.hip): the order of summation is written down in the header and
// depends on sample_numel and the dtype alone, so a sample has the same bits alone and at any position of any batch.
//   stage 1 (rescale_stats_spans<T>): one workgroup per 2048-element span of a sample, lane t owning the span's elements 8 t .. 8 t + 7
//     whichever way they are read: a whole, 16-byte aligned span with one (16-bit), two (fp32) or four (fp64) 16-byte non-temporal
//     loads per operand and lane, any other span -- the last of a ragged sample, every span of a sample that starts off a 16-byte
//     boundary -- element by element with a bounds test.
//   stage 2 (rescale_stats_final<T>): one wave per sample; lanes 0..3 each sum one of the four quantities over the sample's spans.
// The sums behind the loads and the last operations are shared with the rolling form (skr_guidance_stats.h, skr_guidance_stats_rolling.hip).
#include "skr_guidance_stats.h"
#include "skr_device.h"

namespace skr {

template <typename T>
__global__ __launch_bounds__(BLOCK) void rescale_stats_spans(const void* uncond, const void* cond, double scale, int64_t numel, int64_t sample_numel, uint32_t spans,
                                                             double* partials) {
  using M = typename OpMath<T>::type;
  const uint32_t smp = blockIdx.x / spans, j = blockIdx.x - smp * spans;
  const int64_t first = (int64_t)smp * sample_numel, start = first + (int64_t)j * SPAN;
  const int64_t left = first + sample_numel - start;  // elements of the sample from this span on: >= 1
  const int len = left < SPAN ? (int)left : (int)SPAN;
  const int64_t tail_from = numel - numel % TORCH_TAIL;
  const M g = (M)scale;
  const int at = (int)threadIdx.x * VEC;  // this lane's first element within the span

  M u[VEC], c[VEC];
  const bool whole = len == SPAN && ((uint64_t)start * sizeof(T)) % 16 == 0;  // (uniform; the base pointers are 16-byte aligned)
  if (whole) {
    const Raw<T> ru = load_raw<T, false>(reinterpret_cast<const char*>(uncond) + start * (int64_t)sizeof(T), threadIdx.x);
    const Raw<T> rc = load_raw<T, false>(reinterpret_cast<const char*>(cond) + start * (int64_t)sizeof(T), threadIdx.x);
    widen<T, M>(ru, u);
    widen<T, M>(rc, c);
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const bool in = at + i < len;
      u[i] = in ? stat_load<T, M>(uncond, start + at + i) : (M)0;
      c[i] = in ? stat_load<T, M>(cond, start + at + i) : (M)0;
    }
  }
  // the pivots: the sample's first element of c and of p (uniform loads: every lane of every span of the sample has the same two)
  const M c_first = stat_load<T, M>(cond, first);
  const double kc = (double)c_first, kp = (double)stat_guided<T, M>(stat_load<T, M>(uncond, first), c_first, g, first, tail_from);

  span_sums<T, M, false>(u, c, g, kc, kp, at, len, start, tail_from, partials + (int64_t)blockIdx.x * 4);
}

template <typename T>
__global__ __launch_bounds__(64) void rescale_stats_final(const double* partials, uint32_t spans, int64_t sample_numel, void* factor, double* stats) {
  const int64_t smp = blockIdx.x;
  double acc = 0.0;
  if (threadIdx.x < 4) {
    const double* p = partials + smp * spans * 4 + threadIdx.x;
    for (uint32_t j = 0; j < spans; ++j) acc += p[(int64_t)j * 4];
  }
  const double s1c = __shfl(acc, 0), s2c = __shfl(acc, 1), s1p = __shfl(acc, 2), s2p = __shfl(acc, 3);
  if (threadIdx.x != 0) return;
  stats_finish<T>(s1c, s2c, s1p, s2p, sample_numel, smp, factor, stats);
}

}  // namespace skr

extern "C" int skr_guidance_rescale_factor(const void* uncond, const void* cond, int32_t dtype, double scale, int64_t numel, int64_t sample_numel,
                                           void* factor_dev, double* stats_dev, double* partials_dev, void* stream) {
  using namespace skr;
  if (!uncond || !cond || !factor_dev || !partials_dev) return SKR_ERR_NULL;
  if (numel < 0 || sample_numel < 2 || numel % sample_numel != 0) return SKR_ERR_SHAPE;
  if (numel == 0) return SKR_OK;
  if (!aligned16(uncond) || !aligned16(cond)) return SKR_ERR_ALIGN;
  if (!tensor_dtype(dtype)) return SKR_ERR_DTYPE;
  const int64_t samples = numel / sample_numel, spans = (sample_numel + SPAN - 1) / SPAN;
  if (spans > 0x7fffffffll || samples > 0x7fffffffll / spans) return SKR_ERR_UNSUPPORTED;  // one workgroup per span: the grid's x extent
  DeviceGuard device_guard(factor_dev);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  with_step_type(dtype, [&](auto tt) {
    using T = typename decltype(tt)::type;
    hipLaunchKernelGGL(rescale_stats_spans<T>, dim3((unsigned)(samples * spans)), dim3(BLOCK), 0, s, uncond, cond, scale, numel, sample_numel, (uint32_t)spans, partials_dev);
    hipLaunchKernelGGL(rescale_stats_final<T>, dim3((unsigned)samples), dim3(64), 0, s, (const double*)partials_dev, (uint32_t)spans, sample_numel, factor_dev, stats_dev);
  });
  return finish_launch();
}
