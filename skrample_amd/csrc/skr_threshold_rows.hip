// The statistic of dynamic thresholding with device-resident scalars (include/skrample_hip.h, skr_threshold_scale_indexed[_per_sample]):
// skr_threshold_scale (skr_threshold.hip) with a, b, ratio and the maximum taken from the row the thresholded row step reads
// (skr_step_thresholded_rows.hip) -- convert_k[0..3] -- so that a captured thresholded loop serves any schedule and any thresholding
// setting.  One set of kernels for the two row forms (RowForm, skr_step_common.h):
//   WholeBatch  skr_threshold_scale_indexed              rows[index[0] + row_offset], one row for every sample
//   PerSample   skr_threshold_scale_indexed_per_sample   rows[index[sample] + row_offset], one entry per sample
// The passes are skr_threshold.hip's (skr_threshold_select.h holds them behind their scalars); what is this file's own:
//   the row        one scalar load per workgroup, two dependent ones in the per-sample form (the index entry, then the row), through the
//                  constant address space.  A workgroup lies inside one sample in every pass (smp = blockIdx.x / groups), so the row is
//                  uniform over it.  Grid geometry (run, groups) is the host's, from shapes alone.
//   histogram      only a, b and the plain-clip test depend on the row.  The row is asked for at the top and USED behind the clearing of
//                  the four sub-histograms (32 LDS stores a lane and a barrier): the round trips run under the clearing, not in front of
//                  the span loads, which wait for nothing the direct kernel does not wait for.
//   zero, candidates, finish   need the row first: the plain-clip test, and k, k1 and w, which the device forms in double exactly as the
//                  host does (rank_of: one multiplication, a floor, one subtraction, nothing contracted).
//   plain-clip row the row's convert_k[3] (the maximum) is <= 1: every workgroup that reads the row, in all four kernels, returns before
//                  its first vector-memory instruction -- in the whole-batch form the whole launch.  scale[s] and the sample's part of the
//                  workspace keep their bytes; the step launch does not read scale[s] either.  That is why the clearing is per sample here
//                  (threshold_zero_rows: one workgroup a sample) and not one grid-stride fill.
// LDS as in skr_threshold.hip: histogram 4 x 8 KiB, finish 2 x 4 KiB.
//
// Rolling batches (skr_threshold_scale_rolling): kernels of their own, threshold_*_rolling below -- the passes and the geometry are the
// same, the front of every kernel is not:
//   Rolling     skr_threshold_scale_rolling              rows[index[slot] + row_offset]; a negative entry is an inactive slot
//   inactive exit   in all four kernels the workgroup loads its index entry (one scalar load), tests the sign and ends: before any
//                   vector-memory instruction and, in the histogram pass, before the LDS clearing.  scale[slot], the slot's histogram, its
//                   counters and its candidate slice keep every byte, and a free slot costs a launch slot and nothing else.
//   histogram       an active slot asks for its row right behind the sign test and uses it behind the clearing and its barrier, as
//                   threshold_histogram_rows does.  What the rolling form pays is the ONE index round trip in front of the clearing: the
//                   per-sample form runs both of its round trips under the clearing, this one only the second.
//   geometry        run, groups and the per-slot clearing grid are threshold_scale_rows_impl's, from the capacity and the shapes alone:
//                   the grid never depends on which slots are active, and the statistic never depends on the grid (integer counting).
#include "skr_threshold_select.h"
#include "skr_step_guided_kernel.h"  // uniform()

namespace skr {

// the row of sample `smp` (uniform): scalar round trips, no bounds check, no clamp
template <RowForm F>
__device__ __forceinline__ auto threshold_row(const RowRef& r, uint32_t smp) {
  static_assert(row_behind_loads(F), "the two captured-loop forms");
  int32_t at = 0;
  if constexpr (F == RowForm::PerSample) at = uniform(r.index)[smp];
  else if (r.index != nullptr) at = uniform(r.index)[0];
  return uniform(r.rows + (at + r.row_offset));
}

// a row selects unless its maximum is <= 1 (what the eager path decides on the host: s is then identically 1); a NaN maximum selects
__device__ __forceinline__ bool selects(double max_value) { return !(max_value <= 1.0); }

// r = ratio * (n - 1), k = floor(r), k1 = min(k + 1, n - 1), w = r - k: the host's IEEE double operations (skr_threshold_scale), nothing
// contracted.  k is clamped to n - 1, so that no row value names a rank past the sample (a valid ratio never reaches the clamp).
struct Rank { uint32_t k, k1; double w; };
__device__ __forceinline__ Rank rank_of(double ratio, int64_t n) {
  const double r = mul_(ratio, (double)(n - 1)), kf = floor(r);
  uint32_t k = (uint32_t)kf;  // (saturating: a NaN or negative r gives 0)
  if ((int64_t)k > n - 1) k = (uint32_t)(n - 1);
  return Rank{k, (int64_t)k + 1 < n ? k + 1 : k, sub_(r, kf)};
}

template <RowForm F>
__global__ __launch_bounds__(BLOCK) void threshold_zero_rows(uint32_t* hist, uint32_t* meta, const RowRef tab) {
  const uint32_t smp = blockIdx.x;
  if (!selects(threshold_row<F>(tab, smp)->convert_k[3])) return;
  for (int i = threadIdx.x; i < TOP_BINS; i += BLOCK) hist[(int64_t)smp * TOP_BINS + i] = 0u;
  if (threadIdx.x < META) meta[(int64_t)smp * META + threadIdx.x] = 0u;
}

template <typename T, RowForm F>
__global__ __launch_bounds__(BLOCK) void threshold_histogram_rows(const void* sample, const void* output, int64_t sample_numel, uint32_t spans, uint32_t run,
                                                                  uint32_t groups, const RowRef tab, uint32_t* hist, uint32_t* meta) {
  __shared__ uint32_t sub[4][TOP_BINS];
  const uint32_t smp = __builtin_amdgcn_readfirstlane(blockIdx.x / groups), g = blockIdx.x - smp * groups;
  const auto row = threshold_row<F>(tab, smp);
  const double a = row->convert_k[0], b = row->convert_k[1], max_value = row->convert_k[3];  // asked for here, used behind the barrier
  for (int i = threadIdx.x; i < 4 * TOP_BINS; i += BLOCK) (&sub[0][0])[i] = 0u;
  __syncthreads();
  if (!selects(max_value)) return;  // (uniform) nothing read, nothing written
  histogram_spans<T>(sample, output, (float)a, (float)b, sample_numel, spans, run, smp, g, sub, hist, meta);
}

template <typename T, RowForm F>
__global__ __launch_bounds__(BLOCK) void threshold_candidates_rows(const void* sample, const void* output, int64_t sample_numel, uint32_t spans, uint32_t run,
                                                                   uint32_t groups, const RowRef tab, const uint32_t* hist, uint32_t* meta, uint32_t* candidates) {
  __shared__ uint32_t wave_total[4];
  __shared__ Found top[2];
  const uint32_t smp = __builtin_amdgcn_readfirstlane(blockIdx.x / groups), g = blockIdx.x - smp * groups;
  const auto row = threshold_row<F>(tab, smp);
  if (!selects(row->convert_k[3])) return;
  const Rank rk = rank_of(row->convert_k[2], sample_numel);
  candidate_spans<T>(sample, output, (float)row->convert_k[0], (float)row->convert_k[1], sample_numel, spans, run, smp, g, rk.k, rk.k1, hist, meta, candidates,
                     wave_total, top);
}

template <RowForm F>
__global__ __launch_bounds__(BLOCK) void threshold_finish_rows(int64_t sample_numel, const RowRef tab, const uint32_t* hist, const uint32_t* meta,
                                                               const uint32_t* candidates, float* scale) {
  __shared__ uint32_t low[2][LOW_BINS];
  __shared__ uint32_t wave_total[4];
  __shared__ Found top[2], mid[2], last[2];
  const uint32_t smp = blockIdx.x;
  const auto row = threshold_row<F>(tab, smp);
  const double max_value = row->convert_k[3];
  if (!selects(max_value)) return;
  const Rank rk = rank_of(row->convert_k[2], sample_numel);
  finish_sample(sample_numel, smp, rk.k, rk.k1, rk.w, (float)max_value, hist, meta, candidates, scale, low, wave_total, top, mid, last);
}

// ---- rolling batches: the index entry in front of everything, an inactive slot gone before its first vector-memory instruction ----------

// the index entry of slot `smp` (uniform, one scalar load): negative for an inactive slot, tested before row_offset is added
__device__ __forceinline__ int32_t rolling_entry(const RowRef& r, uint32_t smp) { return uniform(r.index)[smp]; }
// the row an active slot's entry names (uniform: scalar loads through the constant address space)
__device__ __forceinline__ auto rolling_threshold_row(const RowRef& r, int32_t at) { return uniform(r.rows + (at + r.row_offset)); }

__global__ __launch_bounds__(BLOCK) void threshold_zero_rolling(uint32_t* hist, uint32_t* meta, const RowRef tab) {
  const uint32_t smp = blockIdx.x;
  const int32_t at = rolling_entry(tab, smp);
  if (at < 0) return;  // inactive: nothing read, nothing written
  if (!selects(rolling_threshold_row(tab, at)->convert_k[3])) return;
  for (int i = threadIdx.x; i < TOP_BINS; i += BLOCK) hist[(int64_t)smp * TOP_BINS + i] = 0u;
  if (threadIdx.x < META) meta[(int64_t)smp * META + threadIdx.x] = 0u;
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void threshold_histogram_rolling(const void* sample, const void* output, int64_t sample_numel, uint32_t spans, uint32_t run,
                                                                     uint32_t groups, const RowRef tab, uint32_t* hist, uint32_t* meta) {
  __shared__ uint32_t sub[4][TOP_BINS];
  const uint32_t smp = __builtin_amdgcn_readfirstlane(blockIdx.x / groups), g = blockIdx.x - smp * groups;
  const int32_t at = rolling_entry(tab, smp);
  if (at < 0) return;  // inactive: in front of the clearing, nothing read, nothing written
  const auto row = rolling_threshold_row(tab, at);
  const double a = row->convert_k[0], b = row->convert_k[1], max_value = row->convert_k[3];  // asked for here, used behind the barrier
  for (int i = threadIdx.x; i < 4 * TOP_BINS; i += BLOCK) (&sub[0][0])[i] = 0u;
  __syncthreads();
  if (!selects(max_value)) return;  // (uniform) nothing read, nothing written
  histogram_spans<T>(sample, output, (float)a, (float)b, sample_numel, spans, run, smp, g, sub, hist, meta);
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void threshold_candidates_rolling(const void* sample, const void* output, int64_t sample_numel, uint32_t spans, uint32_t run,
                                                                      uint32_t groups, const RowRef tab, const uint32_t* hist, uint32_t* meta, uint32_t* candidates) {
  __shared__ uint32_t wave_total[4];
  __shared__ Found top[2];
  const uint32_t smp = __builtin_amdgcn_readfirstlane(blockIdx.x / groups), g = blockIdx.x - smp * groups;
  const int32_t at = rolling_entry(tab, smp);
  if (at < 0) return;
  const auto row = rolling_threshold_row(tab, at);
  if (!selects(row->convert_k[3])) return;
  const Rank rk = rank_of(row->convert_k[2], sample_numel);
  candidate_spans<T>(sample, output, (float)row->convert_k[0], (float)row->convert_k[1], sample_numel, spans, run, smp, g, rk.k, rk.k1, hist, meta, candidates,
                     wave_total, top);
}

__global__ __launch_bounds__(BLOCK) void threshold_finish_rolling(int64_t sample_numel, const RowRef tab, const uint32_t* hist, const uint32_t* meta,
                                                                  const uint32_t* candidates, float* scale) {
  __shared__ uint32_t low[2][LOW_BINS];
  __shared__ uint32_t wave_total[4];
  __shared__ Found top[2], mid[2], last[2];
  const uint32_t smp = blockIdx.x;
  const int32_t at = rolling_entry(tab, smp);
  if (at < 0) return;
  const auto row = rolling_threshold_row(tab, at);
  const double max_value = row->convert_k[3];
  if (!selects(max_value)) return;
  const Rank rk = rank_of(row->convert_k[2], sample_numel);
  finish_sample(sample_numel, smp, rk.k, rk.k1, rk.w, (float)max_value, hist, meta, candidates, scale, low, wave_total, top, mid, last);
}

// The three entries.
static int threshold_scale_rows_impl(const void* sample, const void* output, int32_t dtype, int64_t numel, int64_t sample_numel, const skr_step_row* rows,
                                     const int32_t* index, int32_t row_offset, float* scale_dev, void* workspace_dev, void* stream, RowForm form) {
  if (!sample || !output || !scale_dev || !workspace_dev || !rows || (per_sample_rows(form) && !index)) return SKR_ERR_NULL;
  if (numel < 0 || sample_numel < 1 || numel % sample_numel != 0) return SKR_ERR_SHAPE;
  if (numel == 0) return SKR_OK;
  if (!aligned16(sample) || !aligned16(output) || !aligned16(workspace_dev) || (reinterpret_cast<uintptr_t>(scale_dev) & 3u) != 0) return SKR_ERR_ALIGN;
  if (dtype != SKR_BF16 && dtype != SKR_F16 && dtype != SKR_F32) return SKR_ERR_DTYPE;
  if (sample_numel % SPAN != 0 || row_offset < 0) return SKR_ERR_UNSUPPORTED;  // what the row step covers
  const int64_t samples = numel / sample_numel, spans = sample_numel / SPAN;
  if (sample_numel >= (1ll << 31) || samples > 0x7fffffffll / spans) return SKR_ERR_UNSUPPORTED;  // 32-bit counts; the grid's x extent
  const int64_t run = threshold_run(samples, spans), groups = (spans + run - 1) / run;
  uint32_t* hist = reinterpret_cast<uint32_t*>(workspace_dev);
  uint32_t* meta = hist + samples * TOP_BINS;
  uint32_t* candidates = meta + samples * META;
  DeviceGuard device_guard(scale_dev);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const RowRef tab{rows, index, row_offset};
  const dim3 grid((unsigned)(samples * groups)), per_sample((unsigned)samples);
  with_step_type<false>(dtype, [&](auto tt) {
    with_row_form(form, [&](auto fm) {
      using T = typename decltype(tt)::type;
      constexpr RowForm F = decltype(fm)::value;
      if constexpr (row_behind_loads(F)) {
        hipLaunchKernelGGL(threshold_zero_rows<F>, per_sample, dim3(BLOCK), 0, s, hist, meta, tab);
        hipLaunchKernelGGL((threshold_histogram_rows<T, F>), grid, dim3(BLOCK), 0, s, sample, output, sample_numel, (uint32_t)spans, (uint32_t)run, (uint32_t)groups, tab,
                           hist, meta);
        hipLaunchKernelGGL((threshold_candidates_rows<T, F>), grid, dim3(BLOCK), 0, s, sample, output, sample_numel, (uint32_t)spans, (uint32_t)run, (uint32_t)groups, tab,
                           (const uint32_t*)hist, meta, candidates);
        hipLaunchKernelGGL(threshold_finish_rows<F>, per_sample, dim3(BLOCK), 0, s, sample_numel, tab, (const uint32_t*)hist, (const uint32_t*)meta,
                           (const uint32_t*)candidates, scale_dev);
      } else if constexpr (F == RowForm::Rolling) {  // the same four launches on the same geometry
        hipLaunchKernelGGL(threshold_zero_rolling, per_sample, dim3(BLOCK), 0, s, hist, meta, tab);
        hipLaunchKernelGGL(threshold_histogram_rolling<T>, grid, dim3(BLOCK), 0, s, sample, output, sample_numel, (uint32_t)spans, (uint32_t)run, (uint32_t)groups, tab, hist,
                           meta);
        hipLaunchKernelGGL(threshold_candidates_rolling<T>, grid, dim3(BLOCK), 0, s, sample, output, sample_numel, (uint32_t)spans, (uint32_t)run, (uint32_t)groups, tab,
                           (const uint32_t*)hist, meta, candidates);
        hipLaunchKernelGGL(threshold_finish_rolling, per_sample, dim3(BLOCK), 0, s, sample_numel, tab, (const uint32_t*)hist, (const uint32_t*)meta,
                           (const uint32_t*)candidates, scale_dev);
      }
    });
  });
  return finish_launch();
}

}  // namespace skr

extern "C" int skr_threshold_scale_indexed(const void* sample, const void* output, int32_t dtype, int64_t numel, int64_t sample_numel, const skr_step_row* rows_dev,
                                           const int32_t* index_dev, int32_t row_offset, float* scale_dev, void* workspace_dev, void* stream) {
  return skr::threshold_scale_rows_impl(sample, output, dtype, numel, sample_numel, rows_dev, index_dev, row_offset, scale_dev, workspace_dev, stream, skr::RowForm::WholeBatch);
}

extern "C" int skr_threshold_scale_indexed_per_sample(const void* sample, const void* output, int32_t dtype, int64_t numel, int64_t sample_numel,
                                                      const skr_step_row* rows_dev, const int32_t* sample_index_dev, int32_t row_offset, float* scale_dev,
                                                      void* workspace_dev, void* stream) {
  return skr::threshold_scale_rows_impl(sample, output, dtype, numel, sample_numel, rows_dev, sample_index_dev, row_offset, scale_dev, workspace_dev, stream, skr::RowForm::PerSample);
}

extern "C" int skr_threshold_scale_rolling(const void* sample, const void* output, int32_t dtype, int64_t numel, int64_t sample_numel, const skr_step_row* rows_dev,
                                           const int32_t* sample_index_dev, int32_t row_offset, float* scale_dev, void* workspace_dev, void* stream) {
  return skr::threshold_scale_rows_impl(sample, output, dtype, numel, sample_numel, rows_dev, sample_index_dev, row_offset, scale_dev, workspace_dev, stream, skr::RowForm::Rolling);
}
