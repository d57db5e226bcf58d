// The statistic of rescaled guidance with device-resident scalars (include/skrample_hip.h, skr_guidance_rescale_factor_indexed[_per_sample]
// and skr_guidance_rescale_factor_rolling): skr_guidance_rescale_factor (skr_guidance_stats.hip) with the guidance scale taken from the row
// the guided row step reads (skr_step_guided.hip) -- convert_k[0] -- so that a captured rescaled loop, or a rolling batch, serves any
// schedule, any scale AND any guidance_rescale.  One pair of kernels for the three row forms (RowForm, skr_step_common.h):
//   WholeBatch  skr_guidance_rescale_factor_indexed              rows[index[0] + row_offset], one row for every sample
//   PerSample   skr_guidance_rescale_factor_indexed_per_sample   rows[index[sample] + row_offset], one entry per sample
//   Rolling     skr_guidance_rescale_factor_rolling              the same, for the slots of a rolling batch: a negative entry is an inactive sample
// Two semantics on top, each decided from scalar loads in front of the first vector-memory instruction, in both stages:
//   unrescaled row   the row's convert_k[1] (phi) is exactly zero, either sign: every workgroup that reads the row returns -- in the
//                    whole-batch form that is the whole launch.  Nothing is read; factor, stats and partials keep their bytes, and the step
//                    launch does not read the factor either.  A request that does not rescale costs no statistics traffic;
//   inactive sample  (Rolling alone) a negative index entry, tested before row_offset is added: the same exit.  In the other two forms
//                    every index names a row (a negative entry is as invalid as any other outside the table).
// An active, rescaled sample has the bits skr_guidance_rescale_factor gives it alone: the sums are the shared body (skr_guidance_stats.h), in
// the documented order.  Coverage is the row step's: bf16 / fp16 / fp32, samples of whole 2048-element spans, so every span is whole and
// 16-byte aligned -- the kernels have the vector path only -- and torch's fp16 tail rule cannot arise.
//   stage 1 (rescale_stats_spans_rows<T, RowForm>): one workgroup per span; the pivots are the first element of the sample's first
//     dword, a uniform (scalar) load.
//   stage 2 (rescale_stats_final_rows<T, RowForm>): one wave per sample; lanes 0 and 1 each sum two of the four quantities over the
//     sample's spans, 16 bytes a load, each quantity in span order from zero.
#include "skr_guidance_stats.h"
#include "skr_device.h"

namespace skr {

// the row of sample `smp` (uniform) when the sample is active and rescales, nullptr otherwise: scalar round trips, no bounds check, no clamp
template <RowForm F>
__device__ __forceinline__ const skr_step_row* rescaling_row_of(const RowRef& r, uint32_t smp) {
  static_assert(has_table(F), "the kernarg form is skr_guidance_stats.hip");
  const skr_step_row* row;
  if constexpr (F == RowForm::Rolling) {
    const int32_t at = r.index[smp];
    if (at < 0) return nullptr;  // inactive: tested before row_offset is added
    row = r.rows + (at + r.row_offset);
  } else if constexpr (F == RowForm::PerSample) {
    row = r.rows + (r.index[smp] + r.row_offset);
  } else {
    row = row_of(r);
  }
  return (__builtin_bit_cast(uint64_t, row->convert_k[1]) << 1) != 0 ? row : nullptr;  // phi == +-0: the row does not rescale
}

template <typename T, RowForm F>
__global__ __launch_bounds__(BLOCK) void rescale_stats_spans_rows(const void* uncond, const void* cond, int64_t sample_numel, uint32_t spans, const RowRef tab,
                                                                  double* partials) {
  const uint32_t smp = __builtin_amdgcn_readfirstlane(blockIdx.x / spans), j = blockIdx.x - smp * spans;
  const skr_step_row* row = rescaling_row_of<F>(tab, smp);
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

template <typename T, RowForm F>
__global__ __launch_bounds__(64) void rescale_stats_final_rows(const double* partials, uint32_t spans, int64_t sample_numel, const RowRef tab, void* factor,
                                                               double* stats) {
  const uint32_t smp = blockIdx.x;
  if (rescaling_row_of<F>(tab, smp) == nullptr) return;
  f64x2_t acc = {0.0, 0.0};  // lane 0: S1c, S2c; lane 1: S1p, S2p
  if (threadIdx.x < 2) {
    const f64x2_t* p = reinterpret_cast<const f64x2_t*>(partials + (int64_t)smp * spans * 4) + threadIdx.x;
    for (uint32_t j = 0; j < spans; ++j) acc += p[(int64_t)j * 2];
  }
  const double s1c = __shfl(acc[0], 0), s2c = __shfl(acc[1], 0), s1p = __shfl(acc[0], 1), s2p = __shfl(acc[1], 1);
  if (threadIdx.x != 0) return;
  stats_finish<T>(s1c, s2c, s1p, s2p, sample_numel, (int64_t)smp, factor, stats);
}

// The three entries.
static int rescale_factor_rows_impl(const void* uncond, const void* cond, int32_t dtype, int64_t numel, int64_t sample_numel, const skr_step_row* rows, const int32_t* index,
                                    int32_t row_offset, void* factor, double* stats, double* partials, void* stream, RowForm form) {
  if (!uncond || !cond || !factor || !partials || !rows || (per_sample_rows(form) && !index)) return SKR_ERR_NULL;
  if (numel < 0 || sample_numel < 2 || numel % sample_numel != 0) return SKR_ERR_SHAPE;
  if (numel == 0) return SKR_OK;
  if (!aligned16(uncond) || !aligned16(cond)) return SKR_ERR_ALIGN;
  if (!tensor_dtype(dtype)) return SKR_ERR_DTYPE;
  if (dtype == SKR_F64 || sample_numel % SPAN != 0 || row_offset < 0) return SKR_ERR_UNSUPPORTED;  // what the row step covers
  const int64_t samples = numel / sample_numel, spans = sample_numel / SPAN;
  if (spans > 0x7fffffffll || samples > 0x7fffffffll / spans) return SKR_ERR_UNSUPPORTED;  // one workgroup per span: the grid's x extent
  DeviceGuard device_guard(factor);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const RowRef tab{rows, index, row_offset};
  with_step_type<false>(dtype, [&](auto tt) {
    with_row_form(form, [&](auto fm) {
      using T = typename decltype(tt)::type;
      constexpr RowForm F = decltype(fm)::value;
      if constexpr (has_table(F)) {  // (no entry passes Kernarg)
        hipLaunchKernelGGL((rescale_stats_spans_rows<T, F>), dim3((unsigned)(samples * spans)), dim3(BLOCK), 0, s, uncond, cond, sample_numel, (uint32_t)spans, tab, partials);
        hipLaunchKernelGGL((rescale_stats_final_rows<T, F>), dim3((unsigned)samples), dim3(64), 0, s, (const double*)partials, (uint32_t)spans, sample_numel, tab, factor, stats);
      }
    });
  });
  return finish_launch();
}

}  // namespace skr

extern "C" int skr_guidance_rescale_factor_indexed(const void* uncond, const void* cond, int32_t dtype, int64_t numel, int64_t sample_numel,
                                                   const skr_step_row* rows_dev, const int32_t* index_dev, int32_t row_offset, void* factor_dev, double* stats_dev,
                                                   double* partials_dev, void* stream) {
  return skr::rescale_factor_rows_impl(uncond, cond, dtype, numel, sample_numel, rows_dev, index_dev, row_offset, factor_dev, stats_dev, partials_dev, stream, skr::RowForm::WholeBatch);
}

extern "C" int skr_guidance_rescale_factor_indexed_per_sample(const void* uncond, const void* cond, int32_t dtype, int64_t numel, int64_t sample_numel,
                                                              const skr_step_row* rows_dev, const int32_t* sample_index_dev, int32_t row_offset, void* factor_dev,
                                                              double* stats_dev, double* partials_dev, void* stream) {
  return skr::rescale_factor_rows_impl(uncond, cond, dtype, numel, sample_numel, rows_dev, sample_index_dev, row_offset, factor_dev, stats_dev, partials_dev, stream, skr::RowForm::PerSample);
}

extern "C" int skr_guidance_rescale_factor_rolling(const void* uncond, const void* cond, int32_t dtype, int64_t numel, int64_t sample_numel,
                                                   const skr_step_row* rows_dev, const int32_t* sample_index_dev, int32_t row_offset, void* factor_dev,
                                                   double* stats_dev, double* partials_dev, void* stream) {
  return skr::rescale_factor_rows_impl(uncond, cond, dtype, numel, sample_numel, rows_dev, sample_index_dev, row_offset, factor_dev, stats_dev, partials_dev, stream, skr::RowForm::Rolling);
}
