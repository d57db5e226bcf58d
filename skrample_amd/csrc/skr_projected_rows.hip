// The statistic of adaptive projected guidance with device-resident scalars (include/skrample_hip.h,
// skr_projected_guidance_coef_indexed[_per_sample]): skr_projected_guidance_coef (skr_projected_coef.hip) with the four scalars of a setting
// taken from the row the projected row step reads (skr_step_projected_rows.hip) --
//   convert_k[0] g (the guidance scale)   convert_k[1] eta   convert_k[2] r (norm_threshold)   convert_k[3] beta (momentum)
// -- so that a captured projected loop serves any schedule and any setting.  One pair of kernels for the two row forms (RowForm):
//   WholeBatch  skr_projected_guidance_coef_indexed              rows[(index ? index[0] : 0) + row_offset], one row for every sample
//   PerSample   skr_projected_guidance_coef_indexed_per_sample   rows[index[sample] + row_offset], one entry per sample
// The momentum buffer is required: a loop owns one whatever its rows say, and the ROW decides per sample what happens to it.
//   stage 1 (projected_spans_rows<T, RowForm>): one workgroup per 2048-element span.  The index entry and the row are scalar loads through
//     the constant address space; the two 16-byte non-temporal loads of u and c are issued before the row's beta is asked for, and a
//     workgroup-uniform branch on beta == +-0 follows:
//       zero-momentum row   m is not read, d = rn_T(c - u), NOTHING is stored: the sample's bytes of the buffer stay as they are (the row
//                           step forms the same d from uncond, and never reads the buffer for this sample)
//       momentum row        m is loaded, d = rn_T((c - u) + beta_f32 * m) stored over it; beta is narrowed on the device (v_cvt_f32_f64,
//                           round to nearest even: the host's (float) cast)
//   stage 2 (projected_final_rows<RowForm>): one wave per sample; g, eta and r are the row's.
// Sums, their order, the partials layout and the coefficient arithmetic are the direct entry's (skr_projected.h): a sample has, bit for
// bit, what skr_projected_guidance_coef gives it alone with the row's values, momentum_buf given exactly when beta != 0.  Coverage is the
// row step's: bf16 / fp16 / fp32, samples of whole 2048-element spans, so every span is whole and 16-byte aligned -- the kernels have the
// vector path only.
#include "skr_projected.h"
#include "skr_step_guided_kernel.h"
#include "skr_device.h"

namespace skr {

// the row of sample `smp` (uniform over the workgroup, through readfirstlane): scalar loads, no bounds check, no clamp
template <RowForm F>
__device__ __forceinline__ auto projected_row_of(const RowRef& r, uint32_t smp) {
  static_assert(row_behind_loads(F), "the two captured-loop forms");
  int32_t at = 0;
  if constexpr (F == RowForm::PerSample) at = uniform(r.index)[smp];
  else if (r.index != nullptr) at = uniform(r.index)[0];
  return uniform(r.rows + (at + r.row_offset));
}

template <typename T, RowForm F>
__global__ __launch_bounds__(BLOCK) void projected_spans_rows(const void* uncond, const void* cond, void* mom, int64_t sample_numel, uint32_t spans, const RowRef tab,
                                                              double* partials) {
  const uint32_t smp = __builtin_amdgcn_readfirstlane(blockIdx.x / spans), j = blockIdx.x - smp * spans;
  const auto row = projected_row_of<F>(tab, smp);
  const int64_t off = ((int64_t)smp * sample_numel + (int64_t)j * SPAN) * (int64_t)sizeof(T);  // (a whole span of a 16-byte aligned tensor: aligned)
  const Raw<T> ru = load_raw<T, false>(reinterpret_cast<const char*>(uncond) + off, threadIdx.x);
  const Raw<T> rc = load_raw<T, false>(reinterpret_cast<const char*>(cond) + off, threadIdx.x);
  const double beta = row->convert_k[3];
  float u[VEC], c[VEC], d[VEC];
  if (rescaling(beta)) {  // (uniform) beta != +-0: the running average is read, advanced and stored
    const Raw<T> rm = load_raw<T, false>(reinterpret_cast<const char*>(mom) + off, threadIdx.x);
    const float b = (float)beta;
    float m[VEC];
    widen<T, float>(ru, u);
    widen<T, float>(rc, c);
    widen<T, float>(rm, m);
#pragma unroll
    for (int i = 0; i < VEC; ++i) d[i] = projected_diff<T>(u[i], c[i], b, m[i]);
    store8<T, float, false>(reinterpret_cast<char*>(mom) + off, threadIdx.x, d);  // (d is a value of T: the store's rounding is exact)
  } else {
    widen<T, float>(ru, u);
    widen<T, float>(rc, c);
#pragma unroll
    for (int i = 0; i < VEC; ++i) d[i] = projected_diff<T>(u[i], c[i]);
  }
  projected_span_sums(d, c, true, (int)threadIdx.x * VEC, (int)SPAN, partials + (int64_t)blockIdx.x * 4);
}

template <RowForm F>
__global__ __launch_bounds__(64) void projected_final_rows(const double* partials, uint32_t spans, const RowRef tab, float* coef, double* stats) {
  const uint32_t smp = blockIdx.x;
  const auto row = projected_row_of<F>(tab, smp);
  double sdd, sdc, scc;
  projected_sample_sums(partials, (int64_t)smp, spans, sdd, sdc, scc);
  if (threadIdx.x != 0) return;
  projected_finish(sdd, sdc, scc, row->convert_k[0], row->convert_k[1], row->convert_k[2], (int64_t)smp, coef, stats);
}

// The two entries: the checks of skr_guidance_rescale_factor_indexed[_per_sample] in their order, the momentum buffer beside the operands.
static int projected_coef_rows_impl(const void* uncond, const void* cond, void* mom, int32_t dtype, int64_t numel, int64_t sample_numel, const skr_step_row* rows,
                                    const int32_t* index, int32_t row_offset, float* coef, double* stats, double* partials, void* stream, RowForm form) {
  if (!uncond || !cond || !mom || !coef || !partials || !rows || (per_sample_rows(form) && !index)) return SKR_ERR_NULL;
  if (numel < 0 || sample_numel < 2 || numel % sample_numel != 0) return SKR_ERR_SHAPE;
  if (numel == 0) return SKR_OK;
  if (!aligned16(uncond) || !aligned16(cond) || !aligned16(mom) || (reinterpret_cast<uintptr_t>(coef) & 3u) != 0) return SKR_ERR_ALIGN;
  if (!tensor_dtype(dtype)) return SKR_ERR_DTYPE;
  if (dtype == SKR_F64 || sample_numel % SPAN != 0 || row_offset < 0) return SKR_ERR_UNSUPPORTED;  // what the row step covers
  const int64_t samples = numel / sample_numel, spans = sample_numel / SPAN;
  if (spans > 0x7fffffffll || samples > 0x7fffffffll / spans) return SKR_ERR_UNSUPPORTED;  // one workgroup per span: the grid's x extent
  DeviceGuard device_guard(coef);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const RowRef tab{rows, index, row_offset};
  with_step_type<false>(dtype, [&](auto tt) {
    with_row_form(form, [&](auto fm) {
      using T = typename decltype(tt)::type;
      constexpr RowForm F = decltype(fm)::value;
      if constexpr (row_behind_loads(F)) {  // (no entry passes another form)
        hipLaunchKernelGGL((projected_spans_rows<T, F>), dim3((unsigned)(samples * spans)), dim3(BLOCK), 0, s, uncond, cond, mom, sample_numel, (uint32_t)spans, tab, partials);
        hipLaunchKernelGGL((projected_final_rows<F>), dim3((unsigned)samples), dim3(64), 0, s, (const double*)partials, (uint32_t)spans, tab, coef, stats);
      }
    });
  });
  return finish_launch();
}

}  // namespace skr

extern "C" int skr_projected_guidance_coef_indexed(const void* uncond, const void* cond, void* momentum_buf, int32_t dtype, int64_t numel, int64_t sample_numel,
                                                   const skr_step_row* rows_dev, const int32_t* index_dev, int32_t row_offset, float* coef_dev, double* stats_dev,
                                                   double* partials_dev, void* stream) {
  return skr::projected_coef_rows_impl(uncond, cond, momentum_buf, dtype, numel, sample_numel, rows_dev, index_dev, row_offset, coef_dev, stats_dev, partials_dev, stream,
                                       skr::RowForm::WholeBatch);
}

extern "C" int skr_projected_guidance_coef_indexed_per_sample(const void* uncond, const void* cond, void* momentum_buf, int32_t dtype, int64_t numel, int64_t sample_numel,
                                                              const skr_step_row* rows_dev, const int32_t* sample_index_dev, int32_t row_offset, float* coef_dev,
                                                              double* stats_dev, double* partials_dev, void* stream) {
  return skr::projected_coef_rows_impl(uncond, cond, momentum_buf, dtype, numel, sample_numel, rows_dev, sample_index_dev, row_offset, coef_dev, stats_dev, partials_dev,
                                       stream, skr::RowForm::PerSample);
}
