// The statistic of adaptive projected guidance for rolling batches (include/skrample_hip.h, skr_projected_guidance_coef_rolling): the
// per-sample row form of skr_projected_rows.hip for the slots of a rolling.RollingBatch -- rows[index[slot] + row_offset], a negative
// index entry an inactive slot -- with the one thing a slot adds: the running average of the difference is per-request state that LIVES in
// the slot, the slot is reused by the next request, and nothing zeroes it at admission.  The row says where a request's average starts:
//   convert_k[0..3]   g, eta, r, beta: the captured-loop projected row
//   stream1 != 0      this request's running average starts on this row (no single-output launch reads stream1 otherwise)
// Kernels of their own, because the statement order is the opposite of projected_spans_rows': there the two loads of u and c stand in front
// of everything the row says; here an inactive slot must issue none.
//   stage 1 (projected_spans_rolling<T>), one workgroup per 2048-element span:
//     the index entry   one scalar load through the constant address space, the first thing the workgroup asks for; the sign is tested
//                       before row_offset is added, and a negative entry ends the workgroup before any vector-memory instruction and
//                       before the LDS reduction is touched (threshold_*_rolling's exit, skr_threshold_rows.hip)
//     hiding the row    the entry names the row, but no address of u or c depends on the row: both 16-byte non-temporal loads are issued the
//                       moment the entry is known non-negative, and the row's two values (convert_k[3], stream1) are two scalar loads
//                       from one base issued right behind them and waited for while they are in flight (an empty statement that consumes
//                       stream1 keeps its load beside beta's: the compiler otherwise fetches it inside the momentum branch, a round trip
//                       of its own behind the wait for u and c).  The uniform branches on beta and stream1 follow.  An active workgroup
//                       therefore pays ONE exposed scalar round trip (the index entry) that the per-sample captured form runs under
//                       its loads; the row's round trip runs under them.
//     three uniform cases
//       zero-momentum row (beta == +-0)     the buffer is neither read nor written; d = rn_T(c - u)
//       momentum row, not starting          m is loaded; d = rn_T((c - u) + beta_f32 * m) is stored over it
//       momentum row, starting              m is NOT loaded: its register image is zero bits, which is +0.0 in every dtype, pinned so that
//                                           the compiler cannot fold the multiply or the add away; the same three rounded operations of
//                                           projected_diff<T>(u, c, beta, m) run -- (-0) + (+0) is +0, what the lone run stores from its
//                                           zeroed buffer -- and d is stored.  The slot's stale bytes, NaN patterns included, are never
//                                           in a register.
//   stage 2 (projected_final_rolling), one wave per slot: the entry's sign first; an inactive slot returns before reading partials, and
//     its coef and stats bytes stay as they are.  g, eta and r are the row's.
// Sums, their order, the partials layout (at capacity) and the coefficient arithmetic are skr_projected.h's: an active slot has, bit for
// bit, what skr_projected_guidance_coef gives that sample alone.  Coverage is the per-sample row form's: bf16 / fp16 / fp32, samples of
// whole 2048-element spans, so every span is whole and 16-byte aligned.
#include "skr_projected.h"
#include "skr_step_guided_kernel.h"
#include "skr_device.h"

namespace skr {

// eight elements of +0.0 as a loaded register image, opaque to the compiler: what a starting row takes for m
template <typename T>
__device__ __forceinline__ Raw<T> zero_image() {
  Raw<T> r;
  if constexpr (sizeof(T) == 2) {
    r.q = u32x4_t{0u, 0u, 0u, 0u};
  } else {
    r.q[0] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    r.q[1] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  pin_raw<T>(r);
  return r;
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void projected_spans_rolling(const void* uncond, const void* cond, void* mom, int64_t sample_numel, uint32_t spans, const RowRef tab,
                                                                 double* partials) {
  const uint32_t smp = __builtin_amdgcn_readfirstlane(blockIdx.x / spans);
  const int32_t at = uniform(tab.index)[smp];
  if (at < 0) return;  // inactive: nothing read, nothing written, the reduction's LDS untouched
  const auto row = uniform(tab.rows + (at + tab.row_offset));
  const double beta = row->convert_k[3];  // asked for here, used behind the loads of u and c
  const uint64_t starts = row->stream1;
  const uint32_t j = blockIdx.x - smp * spans;
  const int64_t off = ((int64_t)smp * sample_numel + (int64_t)j * SPAN) * (int64_t)sizeof(T);  // (a whole span of a 16-byte aligned tensor: aligned)
  const Raw<T> ru = load_raw<T, false>(reinterpret_cast<const char*>(uncond) + off, threadIdx.x);
  const Raw<T> rc = load_raw<T, false>(reinterpret_cast<const char*>(cond) + off, threadIdx.x);
  asm volatile("" ::"s"(starts));  // both of the row's values are in SGPRs here: left alone, stream1 is fetched inside the momentum branch, behind the wait for u and c
  float u[VEC], c[VEC], d[VEC];
  if (rescaling(beta)) {  // (uniform) beta != +-0: the running average is advanced and stored
    Raw<T> rm = zero_image<T>();
    if (starts == 0) rm = load_raw<T, false>(reinterpret_cast<const char*>(mom) + off, threadIdx.x);  // (uniform) a starting row never reads the slot's stale bytes
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

__global__ __launch_bounds__(64) void projected_final_rolling(const double* partials, uint32_t spans, const RowRef tab, float* coef, double* stats) {
  const uint32_t smp = blockIdx.x;
  const int32_t at = uniform(tab.index)[smp];
  if (at < 0) return;  // inactive: no partial read, coef and stats keep their bytes
  const auto row = uniform(tab.rows + (at + tab.row_offset));
  double sdd, sdc, scc;
  projected_sample_sums(partials, (int64_t)smp, spans, sdd, sdc, scc);
  if (threadIdx.x != 0) return;
  projected_finish(sdd, sdc, scc, row->convert_k[0], row->convert_k[1], row->convert_k[2], (int64_t)smp, coef, stats);
}

}  // namespace skr

// The checks of skr_projected_guidance_coef_indexed_per_sample in their order.
extern "C" int skr_projected_guidance_coef_rolling(const void* uncond, const void* cond, void* momentum_buf, int32_t dtype, int64_t numel, int64_t sample_numel,
                                                   const skr_step_row* rows_dev, const int32_t* sample_index_dev, int32_t row_offset, float* coef_dev, double* stats_dev,
                                                   double* partials_dev, void* stream) {
  using namespace skr;
  if (!uncond || !cond || !momentum_buf || !coef_dev || !partials_dev || !rows_dev || !sample_index_dev) return SKR_ERR_NULL;
  if (numel < 0 || sample_numel < 2 || numel % sample_numel != 0) return SKR_ERR_SHAPE;
  if (numel == 0) return SKR_OK;
  if (!aligned16(uncond) || !aligned16(cond) || !aligned16(momentum_buf) || (reinterpret_cast<uintptr_t>(coef_dev) & 3u) != 0) return SKR_ERR_ALIGN;
  if (!tensor_dtype(dtype)) return SKR_ERR_DTYPE;
  if (dtype == SKR_F64 || sample_numel % SPAN != 0 || row_offset < 0) return SKR_ERR_UNSUPPORTED;  // what the rolling step covers
  const int64_t slots = numel / sample_numel, spans = sample_numel / SPAN;
  if (spans > 0x7fffffffll || slots > 0x7fffffffll / spans) return SKR_ERR_UNSUPPORTED;  // one workgroup per span: the grid's x extent
  DeviceGuard device_guard(coef_dev);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const RowRef tab{rows_dev, sample_index_dev, row_offset};
  with_step_type<false>(dtype, [&](auto tt) {
    using T = typename decltype(tt)::type;
    hipLaunchKernelGGL(projected_spans_rolling<T>, dim3((unsigned)(slots * spans)), dim3(BLOCK), 0, s, uncond, cond, momentum_buf, sample_numel, (uint32_t)spans, tab, partials_dev);
    hipLaunchKernelGGL(projected_final_rolling, dim3((unsigned)slots), dim3(64), 0, s, (const double*)partials_dev, (uint32_t)spans, tab, coef_dev, stats_dev);
  });
  return finish_launch();
}
