// The statistic of rescaled guidance for the slots of a rolling batch (include/skrample_hip.h, skr_guidance_rescale_factor_rolling):
// skr_guidance_rescale_factor (skr_guidance_stats.hip) with the guidance scale taken per sample from the sample's row -- convert_k[0] --
// and two rolling semantics, each decided from scalar loads in front of the first vector-memory instruction, in both stages:
//   inactive sample    a negative index entry (tested before row_offset is added): every workgroup of the sample returns; nothing of it
//                      is read, its factor, its stats and its partials keep their bytes;
//   unrescaled sample  the row's convert_k[1] (phi) is exactly zero, either sign: the same exit.  A request that does not rescale costs
//                      no statistics traffic and its factor is never written -- the step launch does not read it either.
// An active, rescaled sample has the bits skr_guidance_rescale_factor gives it alone: the sums are the shared body (skr_guidance_stats.h),
// in the documented order.  Coverage is the rolling step's: bf16 / fp16 / fp32, samples of whole 2048-element spans, so every span is whole
// and 16-byte aligned -- the kernels have the vector path only -- and torch's fp16 tail rule cannot arise.
//   stage 1 (rescale_stats_spans_rolling<T>): one workgroup per span; the pivots are the first element of the sample's first dword, a
//     uniform (scalar) load.
//   stage 2 (rescale_stats_final_rolling<T>): one wave per sample; lanes 0 and 1 each sum two of the four quantities over the sample's
//     spans, 16 bytes a load, each quantity in span order from zero.
#include "skr_guidance_stats.h"
#include "skr_device.h"

namespace skr {

// the row of sample `smp` when the sample is active and rescales, nullptr otherwise: two dependent scalar round trips
__device__ __forceinline__ const skr_step_row* rescaling_row(const RowRef& r, uint32_t smp) {
  const int32_t at = r.index[smp];
  if (at < 0) return nullptr;  // inactive: tested before row_offset is added
  const skr_step_row* row = r.rows + (at + r.row_offset);
  return (__builtin_bit_cast(uint64_t, row->convert_k[1]) << 1) != 0 ? row : nullptr;  // phi == +-0: the sample does not rescale
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void rescale_stats_spans_rolling(const void* uncond, const void* cond, int64_t sample_numel, uint32_t spans, const RowRef tab,
                                                                     double* partials) {
  const uint32_t smp = __builtin_amdgcn_readfirstlane(blockIdx.x / spans), j = blockIdx.x - smp * spans;
  const skr_step_row* row = rescaling_row(tab, smp);
  if (row == nullptr) return;  // nothing read, nothing written
  const float g = (float)row->convert_k[0];
  const int64_t first = (int64_t)smp * sample_numel, start = first + (int64_t)j * SPAN;
  const char* ub = reinterpret_cast<const char*>(uncond);
  const char* cb = reinterpret_cast<const char*>(cond);
  const Raw<T> ru = load_raw<T, false>(ub + start * (int64_t)sizeof(T), threadIdx.x);
  const Raw<T> rc = load_raw<T, false>(cb + start * (int64_t)sizeof(T), threadIdx.x);
  // the pivots: the sample's first element of c and of p
  const float c_first = first_of<T>(cb + first * (int64_t)sizeof(T));
  const double kc = (double)c_first, kp = (double)guided_value<T>(first_of<T>(ub + first * (int64_t)sizeof(T)), c_first, g);
  float u[VEC], c[VEC];
  widen<T, float>(ru, u);
  widen<T, float>(rc, c);
  span_sums<T, float, true>(u, c, g, kc, kp, (int)threadIdx.x * VEC, (int)SPAN, start, 0, partials + (int64_t)blockIdx.x * 4);
}

template <typename T>
__global__ __launch_bounds__(64) void rescale_stats_final_rolling(const double* partials, uint32_t spans, int64_t sample_numel, const RowRef tab, void* factor,
                                                                  double* stats) {
  const uint32_t smp = blockIdx.x;
  if (rescaling_row(tab, smp) == nullptr) return;
  f64x2_t acc = {0.0, 0.0};  // lane 0: S1c, S2c; lane 1: S1p, S2p
  if (threadIdx.x < 2) {
    const f64x2_t* p = reinterpret_cast<const f64x2_t*>(partials + (int64_t)smp * spans * 4) + threadIdx.x;
    for (uint32_t j = 0; j < spans; ++j) acc += p[(int64_t)j * 2];
  }
  const double s1c = __shfl(acc[0], 0), s2c = __shfl(acc[1], 0), s1p = __shfl(acc[0], 1), s2p = __shfl(acc[1], 1);
  if (threadIdx.x != 0) return;
  stats_finish<T>(s1c, s2c, s1p, s2p, sample_numel, (int64_t)smp, factor, stats);
}

}  // namespace skr

extern "C" int skr_guidance_rescale_factor_rolling(const void* uncond, const void* cond, int32_t dtype, int64_t numel, int64_t sample_numel,
                                                   const skr_step_row* rows_dev, const int32_t* sample_index_dev, int32_t row_offset, void* factor_dev,
                                                   double* stats_dev, double* partials_dev, void* stream) {
  using namespace skr;
  if (!uncond || !cond || !factor_dev || !partials_dev || !rows_dev || !sample_index_dev) return SKR_ERR_NULL;
  if (numel < 0 || sample_numel < 2 || numel % sample_numel != 0) return SKR_ERR_SHAPE;
  if (numel == 0) return SKR_OK;
  if (!aligned16(uncond) || !aligned16(cond)) return SKR_ERR_ALIGN;
  if (!tensor_dtype(dtype)) return SKR_ERR_DTYPE;
  if (dtype == SKR_F64 || sample_numel % SPAN != 0 || row_offset < 0) return SKR_ERR_UNSUPPORTED;  // what the rolling step covers
  const int64_t samples = numel / sample_numel, spans = sample_numel / SPAN;
  if (spans > 0x7fffffffll || samples > 0x7fffffffll / spans) return SKR_ERR_UNSUPPORTED;  // one workgroup per span: the grid's x extent
  DeviceGuard device_guard(factor_dev);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const RowRef tab{rows_dev, sample_index_dev, row_offset};
  with_step_type<false>(dtype, [&](auto tt) {
    using T = typename decltype(tt)::type;
    hipLaunchKernelGGL(rescale_stats_spans_rolling<T>, dim3((unsigned)(samples * spans)), dim3(BLOCK), 0, s, uncond, cond, sample_numel, (uint32_t)spans, tab, partials_dev);
    hipLaunchKernelGGL(rescale_stats_final_rolling<T>, dim3((unsigned)samples), dim3(64), 0, s, (const double*)partials_dev, (uint32_t)spans, sample_numel, tab, factor_dev, stats_dev);
  });
  return finish_launch();
}
