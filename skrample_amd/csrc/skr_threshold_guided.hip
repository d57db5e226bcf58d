// The statistic of guided dynamic thresholding (include/skrample_hip.h, skr_guided_threshold_scale): skr_threshold_scale over the guided
// prediction pg = rn_T(u + rn_T(g * rn_T(c - u))), formed in registers from uncond and cond -- the tensor of the guidance-only launch is
// never written and never read back.
//
// The select is the one of skr_threshold.hip, over what skr_threshold_select.h shares: count_bin, find_rank, finish_sample,
// threshold_run and the workspace layout.  Counting is integer addition, so s has the bits of skr_threshold_scale over the stored tensor
// whenever the magnitudes are the same values, and they are: stat_guided (the guided value with torch's fp16 tail rule by the element's
// index in the whole launch), then x0_value and magnitude_bits, in a file built without packed fp32 operations like its neighbours.
//   zero        guided_threshold_zero            restated here (five lines): the direct entry's code object stays as it is
//   histogram   guided_threshold_histogram<T, TAIL>   skr_threshold.hip's pass behind a three-operand span loader: a whole 16-byte
//               aligned span is three 16-byte non-temporal loads per lane (six for fp32), all issued before the first use; any other
//               span is read element by element in the same lane ownership (lane t owns the span's elements 8 t .. 8 t + 7).
//   candidates  guided_threshold_candidates<T, TAIL>  the same loader; bins of rank k and k + 1 re-derived per workgroup, as there
//   finish      guided_threshold_finish          finish_sample behind its kernel's scalars: it has no operand of its own
// TAIL is a compile-time split, as span_sums<..., WHOLE> is: a launch with numel % 2048 == 0 has no fp16 tail and makes no per-element
// test; only an fp16 launch with a ragged numel instantiates the test, and then EVERY span makes it -- a span can be whole and aligned
// and still straddle the tail (sample_numel 2056, three samples: the last sample's first span starts at 4112, the tail at 6144).
// LDS: histogram 32 KiB (4 sub-histograms of 2048 uint32); candidates 16 bytes + 2 records; finish 8 KiB (two 1024-bin histograms).
#include "skr_threshold_select.h"

namespace skr {

// the magnitudes of this lane's eight elements of the span that starts at element `start` of the launch (`len` of them counted), the
// network output being the guided value of uncond and cond
template <typename T, bool TAIL>
__device__ __forceinline__ void guided_span_magnitudes(const void* sample, const void* uncond, const void* cond, float g, float a, float b, int64_t start, int len,
                                                       int64_t tail_from, uint32_t (&m)[VEC]) {
  const int at = (int)threadIdx.x * VEC;
  float x[VEC], u[VEC], c[VEC];
  const bool whole = len == SPAN && ((uint64_t)start * sizeof(T)) % 16 == 0;  // (uniform; the base pointers are 16-byte aligned)
  if (whole) {
    const int64_t off = start * (int64_t)sizeof(T);
    Raw<T> rx = load_raw<T, false>(reinterpret_cast<const char*>(sample) + off, threadIdx.x);
    Raw<T> ru = load_raw<T, false>(reinterpret_cast<const char*>(uncond) + off, threadIdx.x);
    Raw<T> rc = load_raw<T, false>(reinterpret_cast<const char*>(cond) + off, threadIdx.x);
    pin_raw(rx), pin_raw(ru), pin_raw(rc);  // all three are out before the first of them is consumed
    widen<T, float>(rx, x);
    widen<T, float>(ru, u);
    widen<T, float>(rc, c);
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const bool in = at + i < len;
      x[i] = in ? load_scalar<T>(sample, start + at + i) : 0.f;
      u[i] = in ? load_scalar<T>(uncond, start + at + i) : 0.f;
      c[i] = in ? load_scalar<T>(cond, start + at + i) : 0.f;
    }
  }
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    float pg;
    if constexpr (TAIL) pg = stat_guided<T, float>(u[i], c[i], g, start + at + i, tail_from);
    else pg = guided_value<T>(u[i], c[i], g);
    m[i] = whole || at + i < len ? magnitude_bits(x0_value(a, x[i], b, pg)) : NO_ELEMENT;
  }
}

__global__ __launch_bounds__(BLOCK) void guided_threshold_zero(uint32_t* words, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) words[i] = 0u;
}

struct GuidedStatArgs {
  const void* sample;
  const void* uncond;
  const void* cond;
  int64_t sample_numel, tail_from;
  float g, a, b;
  uint32_t spans, run, groups;
};

template <typename T, bool TAIL>
__global__ __launch_bounds__(BLOCK) void guided_threshold_histogram(const GuidedStatArgs q, uint32_t* hist, uint32_t* meta) {
  __shared__ uint32_t sub[4][TOP_BINS];
  const uint32_t smp = blockIdx.x / q.groups, g = blockIdx.x - smp * q.groups;
  for (int i = threadIdx.x; i < 4 * TOP_BINS; i += BLOCK) (&sub[0][0])[i] = 0u;
  __syncthreads();
  uint32_t* mine = sub[threadIdx.x >> 6];
  uint32_t nans = 0;
  const int64_t first = (int64_t)smp * q.sample_numel;
  const uint32_t j_end = (g + 1) * q.run < q.spans ? (g + 1) * q.run : q.spans;
  for (uint32_t j = g * q.run; j < j_end; ++j) {
    const int64_t start = first + (int64_t)j * SPAN, left = first + q.sample_numel - start;
    uint32_t m[VEC];
    guided_span_magnitudes<T, TAIL>(q.sample, q.uncond, q.cond, q.g, q.a, q.b, start, left < SPAN ? (int)left : (int)SPAN, q.tail_from, m);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const bool is = m[i] != NO_ELEMENT, nan = is && magnitude_is_nan(m[i]);
      nans += nan ? 1u : 0u;
      count_bin(mine, m[i] >> 20, is && !nan);
    }
  }
  __syncthreads();
  for (int bin = threadIdx.x; bin < TOP_BINS; bin += BLOCK) {
    const uint32_t total = sub[0][bin] + sub[1][bin] + sub[2][bin] + sub[3][bin];
    if (total != 0) atomicAdd(&hist[(int64_t)smp * TOP_BINS + bin], total);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nans += __shfl_down(nans, o);
  if ((threadIdx.x & 63) == 0 && nans != 0) atomicAdd(&meta[(int64_t)smp * META], nans);
}

template <typename T, bool TAIL>
__global__ __launch_bounds__(BLOCK) void guided_threshold_candidates(const GuidedStatArgs q, uint32_t k, uint32_t k1, const uint32_t* hist, uint32_t* meta,
                                                                     uint32_t* candidates) {
  __shared__ uint32_t wave_total[4];
  __shared__ Found top[2];
  const uint32_t smp = blockIdx.x / q.groups, g = blockIdx.x - smp * q.groups;
  if (meta[(int64_t)smp * META] != 0) return;  // (uniform) a sample that holds a NaN selects nothing: its scale is NaN
  find_rank<TOP_BINS / BLOCK>(hist + (int64_t)smp * TOP_BINS, k, wave_total, &top[0]);
  find_rank<TOP_BINS / BLOCK>(hist + (int64_t)smp * TOP_BINS, k1, wave_total, &top[1]);
  const uint32_t bin_k = top[0].bin, bin_k1 = top[1].bin;
  uint32_t* cursor = meta + (int64_t)smp * META + 1;
  uint32_t* list = candidates + (int64_t)smp * q.sample_numel;
  const int lane = threadIdx.x & 63;
  const int64_t first = (int64_t)smp * q.sample_numel;
  const uint32_t j_end = (g + 1) * q.run < q.spans ? (g + 1) * q.run : q.spans;
  for (uint32_t j = g * q.run; j < j_end; ++j) {
    const int64_t start = first + (int64_t)j * SPAN, left = first + q.sample_numel - start;
    uint32_t m[VEC];
    guided_span_magnitudes<T, TAIL>(q.sample, q.uncond, q.cond, q.g, q.a, q.b, start, left < SPAN ? (int)left : (int)SPAN, q.tail_from, m);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const uint32_t bin = m[i] >> 20;
      const bool take = m[i] != NO_ELEMENT && (bin == bin_k || bin == bin_k1);
      const uint64_t takers = __ballot(take);
      if (takers != 0) {  // (uniform) one atomic per wave and element slot
        const int leader = __ffsll((long long)takers) - 1;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(cursor, (uint32_t)__popcll(takers));
        base = __shfl(base, leader);
        const uint32_t at = base + (uint32_t)__popcll(takers & ((1ull << lane) - 1ull));
        if (take && (int64_t)at < q.sample_numel) list[at] = m[i];  // (the candidates are elements of the sample: the test never fails)
      }
    }
  }
}

__global__ __launch_bounds__(BLOCK) void guided_threshold_finish(int64_t sample_numel, uint32_t k, uint32_t k1, double w, float max_value, const uint32_t* hist,
                                                                 const uint32_t* meta, const uint32_t* candidates, float* scale) {
  __shared__ uint32_t low[2][LOW_BINS];
  __shared__ uint32_t wave_total[4];
  __shared__ Found top[2], mid[2], last[2];
  finish_sample(sample_numel, blockIdx.x, k, k1, w, max_value, hist, meta, candidates, scale, low, wave_total, top, mid, last);
}

}  // namespace skr

extern "C" int skr_guided_threshold_scale(const void* sample, const void* uncond, const void* cond, int32_t dtype, double guidance_scale, double a, double b,
                                          double ratio, double sample_max_value, int64_t numel, int64_t sample_numel, float* scale_dev, void* workspace_dev,
                                          void* stream) {
  using namespace skr;
  if (!sample || !uncond || !cond || !scale_dev || !workspace_dev) return SKR_ERR_NULL;
  if (numel < 0 || sample_numel < 1 || numel % sample_numel != 0) return SKR_ERR_SHAPE;
  if (numel == 0) return SKR_OK;
  if (!aligned16(sample) || !aligned16(uncond) || !aligned16(cond) || !aligned16(workspace_dev) || (reinterpret_cast<uintptr_t>(scale_dev) & 3u) != 0)
    return SKR_ERR_ALIGN;
  if (dtype != SKR_BF16 && dtype != SKR_F16 && dtype != SKR_F32) return SKR_ERR_DTYPE;
  if (!(ratio > 0.0 && ratio <= 1.0)) return SKR_ERR_UNSUPPORTED;  // (a NaN fails both)
  const int64_t samples = numel / sample_numel, spans = (sample_numel + SPAN - 1) / SPAN;
  if (sample_numel >= (1ll << 31) || samples > 0x7fffffffll / spans) return SKR_ERR_UNSUPPORTED;  // 32-bit counts; the grid's x extent
  const int64_t run = threshold_run(samples, spans), groups = (spans + run - 1) / run;
  const double r = ratio * (double)(sample_numel - 1), kf = floor(r);
  const uint32_t k = (uint32_t)kf, k1 = (int64_t)k + 1 < sample_numel ? k + 1 : k;
  uint32_t* hist = reinterpret_cast<uint32_t*>(workspace_dev);
  uint32_t* meta = hist + samples * TOP_BINS;
  uint32_t* candidates = meta + samples * META;
  DeviceGuard device_guard(scale_dev);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t words = samples * (TOP_BINS + META);
  hipLaunchKernelGGL(guided_threshold_zero, dim3((unsigned)grid_blocks(words, BLOCK, 1024)), dim3(BLOCK), 0, s, hist, words);
  const dim3 grid((unsigned)(samples * groups));
  const GuidedStatArgs q{sample, uncond, cond, sample_numel, numel - numel % TORCH_TAIL, (float)guidance_scale, (float)a, (float)b,
                         (uint32_t)spans,  (uint32_t)run, (uint32_t)groups};
  const bool tail = dtype == SKR_F16 && numel % TORCH_TAIL != 0;  // (no other dtype has the rule: one instantiation each)
  with_step_type<false>(dtype, [&](auto tt) {
    using T = typename decltype(tt)::type;
    auto passes = [&](auto tl) {
      constexpr bool TAIL = decltype(tl)::value;
      hipLaunchKernelGGL((guided_threshold_histogram<T, TAIL>), grid, dim3(BLOCK), 0, s, q, hist, meta);
      hipLaunchKernelGGL((guided_threshold_candidates<T, TAIL>), grid, dim3(BLOCK), 0, s, q, k, k1, (const uint32_t*)hist, meta, candidates);
    };
    if constexpr (std::is_same<T, f16_t>::value) {
      if (tail) passes(bool_c<true>{});
      else passes(bool_c<false>{});
    } else {
      passes(bool_c<false>{});
    }
  });
  hipLaunchKernelGGL(guided_threshold_finish, dim3((unsigned)samples), dim3(BLOCK), 0, s, sample_numel, k, k1, r - kf, (float)sample_max_value,
                     (const uint32_t*)hist, (const uint32_t*)meta, (const uint32_t*)candidates, scale_dev);
  return finish_launch();
}
