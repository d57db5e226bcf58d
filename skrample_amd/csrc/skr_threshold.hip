// The statistic of dynamic thresholding (include/skrample_hip.h, skr_threshold_scale): per sample, the `ratio` quantile of |x0| with
// x0 = rn32(rn32(a x) + rn32(b o)), linearly interpolated between two EXACT order statistics, clamped to [1, sample_max_value].
//
// A non-negative fp32 orders as its bit pattern, so the order statistics are a radix select over the 31 magnitude bits, 11 + 10 + 10.
// Counting is integer addition: the result depends on no grid size, span run, atomic order or candidate order.
//   zero        threshold_zero         clears the per-sample histograms, NaN counts and cursors inside the workspace (a kernel, not a memset
//                                      node: the entry is recorded into captured graphs)
//   histogram   threshold_histogram<T> a workgroup of 256 lanes takes a run of 2048-element spans of one sample (lane t the span's elements
//                                      8 t .. 8 t + 7, whole aligned spans by 16-byte non-temporal loads, any other element by element, as
//                                      skr_guidance_stats.hip reads them), forms x0 in registers and counts the top 11 magnitude bits (8
//                                      exponent, 3 mantissa) into an LDS histogram.  A latent's magnitudes fall into a couple of dozen of
//                                      the 2048 bins, so the contention is the design problem: each wave owns a sub-histogram (4 x 8 KiB),
//                                      and the lanes of a wave that hit one bin are combined by ballot before ONE LDS atomic per distinct
//                                      bin (count_bin).  Only the non-empty bins are flushed, with vector integer atomics, to the sample's
//                                      global histogram (8 KiB, L2-resident).  NaNs are counted on the side and never enter a histogram.
//   candidates  threshold_candidates<T> every workgroup re-derives the bins of rank k and rank k + 1 from the finished histogram (one block
//                                      scan each), re-reads its spans and appends the magnitudes that fall into those bins to the sample's
//                                      candidate list through a wave-aggregated atomic cursor.  The list's order is free.
//   finish      threshold_finish       one workgroup per sample selects both ranks among the candidates with two further 10-bit LDS
//                                      histogram passes, reading the list from global memory (one path whatever the count: a sample whose
//                                      elements are all equal has every element a candidate, which is why the list holds sample_numel
//                                      values), then forms q and s in double and writes scale_dev[sample].
// LDS: histogram 32 KiB (4 sub-histograms of 2048 uint32); candidates 16 bytes + 2 records; finish 8 KiB (two 1024-bin histograms).
#include "skr_threshold.h"
#include "skr_guidance_stats.h"
#include "skr_device.h"
#include <math.h>

namespace skr {

constexpr int TOP_BINS = 2048, LOW_BINS = 1024;  // 11 + 10 + 10 bits
constexpr int META = 4;                          // uint32 per sample behind the histograms: NaN count, candidate cursor, two spare
constexpr uint32_t NO_ELEMENT = 0xffffffffu;     // not a magnitude: a lane's slot past the end of a ragged span
static_assert(SKR_THRESHOLD_WORKSPACE(4096, 2048) == 2 * (TOP_BINS + META) * 4 + 4096 * 4, "the workspace layout below is the header's macro");

struct Found { uint32_t bin, below, count; };  // the bin that holds a rank, the elements in the bins below it, the elements in it

// the magnitudes of this lane's eight elements of the span that starts at element `start` of the launch (`len` of them counted)
template <typename T>
__device__ __forceinline__ void span_magnitudes(const void* sample, const void* output, float a, float b, int64_t start, int len, uint32_t (&m)[VEC]) {
  const int at = (int)threadIdx.x * VEC;
  float x[VEC], o[VEC];
  const bool whole = len == SPAN && ((uint64_t)start * sizeof(T)) % 16 == 0;  // (uniform; the base pointers are 16-byte aligned)
  if (whole) {
    const Raw<T> rx = load_raw<T, false>(reinterpret_cast<const char*>(sample) + start * (int64_t)sizeof(T), threadIdx.x);
    const Raw<T> ro = load_raw<T, false>(reinterpret_cast<const char*>(output) + start * (int64_t)sizeof(T), threadIdx.x);
    widen<T, float>(rx, x);
    widen<T, float>(ro, o);
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const bool in = at + i < len;
      x[i] = in ? load_scalar<T>(sample, start + at + i) : 0.f;
      o[i] = in ? load_scalar<T>(output, start + at + i) : 0.f;
    }
  }
#pragma unroll
  for (int i = 0; i < VEC; ++i) m[i] = whole || at + i < len ? magnitude_bits(x0_value(a, x[i], b, o[i])) : NO_ELEMENT;
}

// One count per valid lane into h[bin], the lanes of the wave that share a bin combined into one LDS atomic.  Called by whole waves.
__device__ __forceinline__ void count_bin(uint32_t* h, uint32_t bin, bool valid) {
  uint64_t todo = __ballot(valid);
  while (todo != 0) {  // (uniform: one trip per distinct bin of the wave)
    const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
    const uint32_t its = __builtin_amdgcn_readlane(bin, leader);
    const uint64_t same = __ballot(valid && bin == its);
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&h[its], (uint32_t)__popcll(same));
    todo &= ~same;
  }
}

// exclusive prefix sum of one value per lane over the workgroup's 256 lanes
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t* wave_total /* LDS [4] */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wave_total[wave] = inc;
  __syncthreads();
  uint32_t base = 0;
  for (int w = 0; w < wave; ++w) base += wave_total[w];
  return base + inc - v;
}

// the bin of h[0 .. 256 * PER) that holds rank r (0-based, ascending), by the whole workgroup; *out is left zero when r is past the total
template <int PER>
__device__ __forceinline__ void find_rank(const uint32_t* h, uint32_t r, uint32_t* wave_total, Found* out) {
  uint32_t c[PER], sum = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) { c[i] = h[threadIdx.x * PER + i]; sum += c[i]; }
  if (threadIdx.x == 0) *out = Found{0u, 0u, 0u};
  uint32_t cum = block_exclusive(sum, wave_total);  // (its barrier orders the line above before the one match below)
  if (r >= cum && r - cum < sum) {
    bool done = false;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      if (!done && r - cum < c[i]) { *out = Found{(uint32_t)(threadIdx.x * PER + i), cum, c[i]}; done = true; }
      if (!done) cum += c[i];
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(BLOCK) void threshold_zero(uint32_t* words, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) words[i] = 0u;
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void threshold_histogram(const void* sample, const void* output, float a, float b, int64_t sample_numel, uint32_t spans,
                                                             uint32_t run, uint32_t groups, uint32_t* hist, uint32_t* meta) {
  __shared__ uint32_t sub[4][TOP_BINS];
  const uint32_t smp = blockIdx.x / groups, g = blockIdx.x - smp * groups;
  for (int i = threadIdx.x; i < 4 * TOP_BINS; i += BLOCK) (&sub[0][0])[i] = 0u;
  __syncthreads();
  uint32_t* mine = sub[threadIdx.x >> 6];
  uint32_t nans = 0;
  const int64_t first = (int64_t)smp * sample_numel;
  const uint32_t j_end = (g + 1) * run < spans ? (g + 1) * run : spans;
  for (uint32_t j = g * run; j < j_end; ++j) {
    const int64_t start = first + (int64_t)j * SPAN, left = first + sample_numel - start;
    uint32_t m[VEC];
    span_magnitudes<T>(sample, output, a, b, start, left < SPAN ? (int)left : (int)SPAN, m);
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

template <typename T>
__global__ __launch_bounds__(BLOCK) void threshold_candidates(const void* sample, const void* output, float a, float b, int64_t sample_numel, uint32_t spans,
                                                              uint32_t run, uint32_t groups, uint32_t k, uint32_t k1, const uint32_t* hist, uint32_t* meta,
                                                              uint32_t* candidates) {
  __shared__ uint32_t wave_total[4];
  __shared__ Found top[2];
  const uint32_t smp = blockIdx.x / groups, g = blockIdx.x - smp * groups;
  if (meta[(int64_t)smp * META] != 0) return;  // (uniform) a sample that holds a NaN selects nothing: its scale is NaN
  find_rank<TOP_BINS / BLOCK>(hist + (int64_t)smp * TOP_BINS, k, wave_total, &top[0]);
  find_rank<TOP_BINS / BLOCK>(hist + (int64_t)smp * TOP_BINS, k1, wave_total, &top[1]);
  const uint32_t bin_k = top[0].bin, bin_k1 = top[1].bin;
  uint32_t* cursor = meta + (int64_t)smp * META + 1;
  uint32_t* list = candidates + (int64_t)smp * sample_numel;
  const int lane = threadIdx.x & 63;
  const int64_t first = (int64_t)smp * sample_numel;
  const uint32_t j_end = (g + 1) * run < spans ? (g + 1) * run : spans;
  for (uint32_t j = g * run; j < j_end; ++j) {
    const int64_t start = first + (int64_t)j * SPAN, left = first + sample_numel - start;
    uint32_t m[VEC];
    span_magnitudes<T>(sample, output, a, b, start, left < SPAN ? (int)left : (int)SPAN, m);
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
        if (take && (int64_t)at < sample_numel) list[at] = m[i];  // (the candidates are elements of the sample: the test never fails)
      }
    }
  }
}

__global__ __launch_bounds__(BLOCK) void threshold_finish(int64_t sample_numel, uint32_t k, uint32_t k1, double w, float max_value, const uint32_t* hist,
                                                          const uint32_t* meta, const uint32_t* candidates, float* scale) {
  __shared__ uint32_t low[2][LOW_BINS];
  __shared__ uint32_t wave_total[4];
  __shared__ Found top[2], mid[2], last[2];
  const uint32_t smp = blockIdx.x;
  if (meta[(int64_t)smp * META] != 0) {  // (uniform)
    if (threadIdx.x == 0) scale[smp] = __builtin_nanf("");
    return;
  }
  find_rank<TOP_BINS / BLOCK>(hist + (int64_t)smp * TOP_BINS, k, wave_total, &top[0]);
  find_rank<TOP_BINS / BLOCK>(hist + (int64_t)smp * TOP_BINS, k1, wave_total, &top[1]);
  const uint32_t* list = candidates + (int64_t)smp * sample_numel;
  uint32_t count = top[0].count + (top[1].bin != top[0].bin ? top[1].count : 0u);
  if ((int64_t)count > sample_numel) count = (uint32_t)sample_numel;  // (never: the list's bound, whatever the histogram holds)
  uint32_t prefix[2] = {top[0].bin, top[1].bin};         // the bits of each rank's value found so far
  uint32_t rank[2] = {k - top[0].below, k1 - top[1].below};  // each rank among the elements that share its prefix
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int shift = pass == 0 ? 10 : 0;
    for (int i = threadIdx.x; i < 2 * LOW_BINS; i += BLOCK) (&low[0][0])[i] = 0u;
    __syncthreads();
    for (uint32_t at = 0; at < count; at += BLOCK) {  // (uniform trips: count_bin is called by whole waves)
      const bool in = at + threadIdx.x < count;
      const uint32_t v = in ? list[at + threadIdx.x] : 0u;
      const uint32_t head = v >> (shift + 10), digit = (v >> shift) & (LOW_BINS - 1);
      count_bin(low[0], digit, in && head == prefix[0]);
      count_bin(low[1], digit, in && head == prefix[1]);
    }
    __syncthreads();
    Found* found = pass == 0 ? mid : last;
    find_rank<LOW_BINS / BLOCK>(low[0], rank[0], wave_total, &found[0]);
    find_rank<LOW_BINS / BLOCK>(low[1], rank[1], wave_total, &found[1]);
#pragma unroll
    for (int q = 0; q < 2; ++q) { prefix[q] = (prefix[q] << 10) | found[q].bin; rank[q] -= found[q].below; }
  }
  if (threadIdx.x != 0) return;
  const float lo = __uint_as_float(prefix[0]), hi = __uint_as_float(prefix[1]);
  // q in double, rounded once: three IEEE operations as written, so w == 0 and equal finite neighbours give the order statistic itself,
  // an infinite upper neighbour gives inf (w > 0) or NaN (w == 0: 0 * inf), two infinite ones NaN; the clamp is made of comparisons and
  // keeps a NaN
  const double q = add_((double)lo, mul_(w, sub_((double)hi, (double)lo)));
  const float qf = (float)q;
  float s = qf < 1.f ? 1.f : qf;
  s = s > max_value ? max_value : s;
  scale[smp] = s;
}

}  // namespace skr

extern "C" int skr_threshold_scale(const void* sample, const void* output, int32_t dtype, double a, double b, double ratio, double sample_max_value,
                                   int64_t numel, int64_t sample_numel, float* scale_dev, void* workspace_dev, void* stream) {
  using namespace skr;
  if (!sample || !output || !scale_dev || !workspace_dev) return SKR_ERR_NULL;
  if (numel < 0 || sample_numel < 1 || numel % sample_numel != 0) return SKR_ERR_SHAPE;
  if (numel == 0) return SKR_OK;
  if (!aligned16(sample) || !aligned16(output) || !aligned16(workspace_dev) || (reinterpret_cast<uintptr_t>(scale_dev) & 3u) != 0) return SKR_ERR_ALIGN;
  if (dtype != SKR_BF16 && dtype != SKR_F16 && dtype != SKR_F32) return SKR_ERR_DTYPE;
  if (!(ratio > 0.0 && ratio <= 1.0)) return SKR_ERR_UNSUPPORTED;  // (a NaN fails both)
  const int64_t samples = numel / sample_numel, spans = (sample_numel + SPAN - 1) / SPAN;
  if (sample_numel >= (1ll << 31) || samples > 0x7fffffffll / spans) return SKR_ERR_UNSUPPORTED;  // 32-bit counts; the grid's x extent
  // spans per workgroup: enough workgroups to fill the device, few enough that a sub-histogram's zeroing and flush are shared by several spans
  int64_t run = samples * spans / 1024;
  run = run < 1 ? 1 : (run > 8 ? 8 : run);
  const int64_t groups = (spans + run - 1) / run;
  const double r = ratio * (double)(sample_numel - 1), kf = floor(r);
  const uint32_t k = (uint32_t)kf, k1 = (int64_t)k + 1 < sample_numel ? k + 1 : k;
  uint32_t* hist = reinterpret_cast<uint32_t*>(workspace_dev);
  uint32_t* meta = hist + samples * TOP_BINS;
  uint32_t* candidates = meta + samples * META;
  DeviceGuard device_guard(scale_dev);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t words = samples * (TOP_BINS + META);
  hipLaunchKernelGGL(threshold_zero, dim3((unsigned)grid_blocks(words, BLOCK, 1024)), dim3(BLOCK), 0, s, hist, words);
  const dim3 grid((unsigned)(samples * groups));
  with_step_type<false>(dtype, [&](auto tt) {
    using T = typename decltype(tt)::type;
    hipLaunchKernelGGL(threshold_histogram<T>, grid, dim3(BLOCK), 0, s, sample, output, (float)a, (float)b, sample_numel, (uint32_t)spans, (uint32_t)run,
                       (uint32_t)groups, hist, meta);
    hipLaunchKernelGGL(threshold_candidates<T>, grid, dim3(BLOCK), 0, s, sample, output, (float)a, (float)b, sample_numel, (uint32_t)spans, (uint32_t)run,
                       (uint32_t)groups, k, k1, (const uint32_t*)hist, meta, candidates);
  });
  hipLaunchKernelGGL(threshold_finish, dim3((unsigned)samples), dim3(BLOCK), 0, s, sample_numel, k, k1, r - kf, (float)sample_max_value, (const uint32_t*)hist,
                     (const uint32_t*)meta, (const uint32_t*)candidates, scale_dev);
  return finish_launch();
}
