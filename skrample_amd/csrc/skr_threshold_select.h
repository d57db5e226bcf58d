// The radix select of dynamic thresholding behind its scalars, as the row forms of the statistic run it (skr_threshold_rows.hip): each pass
// of skr_threshold.hip as a body that takes its scalars -- a, b, k, k1, w, the maximum -- as arguments, whatever they were fetched from,
// so that WholeBatch and PerSample are one kernel each.  The operations and their order are skr_threshold.hip's, statement for statement:
// a sample has the same histogram, the same candidates and the same scale through either entry.  The direct kernels keep their own text:
// rebuilt over these bodies they computed the same but compiled to other register allocation and LDS access order in the finish pass,
// and the direct entries' code objects stay as they are.
#pragma once
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

// ---- the three passes, each behind its kernel's scalars; `smp` the workgroup's sample, `g` its group of spans within the sample ----------

// histogram: `sub` is the workgroup's four cleared sub-histograms (a barrier behind the clearing)
template <typename T>
__device__ __forceinline__ void histogram_spans(const void* sample, const void* output, float a, float b, int64_t sample_numel, uint32_t spans, uint32_t run,
                                                uint32_t smp, uint32_t g, uint32_t (*sub)[TOP_BINS], uint32_t* hist, uint32_t* meta) {
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

// candidates: the magnitudes of the workgroup's spans that fall into the bins of rank k and rank k1, appended to the sample's list
// (the LDS of this pass and the next is declared by the kernel)
template <typename T>
__device__ __forceinline__ void candidate_spans(const void* sample, const void* output, float a, float b, int64_t sample_numel, uint32_t spans, uint32_t run,
                                                uint32_t smp, uint32_t g, uint32_t k, uint32_t k1, const uint32_t* hist, uint32_t* meta, uint32_t* candidates,
                                                uint32_t* wave_total /* LDS [4] */, Found* top /* LDS [2] */) {
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

// finish: both ranks among the sample's candidates, then q and s
__device__ __forceinline__ void finish_sample(int64_t sample_numel, uint32_t smp, uint32_t k, uint32_t k1, double w, float max_value, const uint32_t* hist,
                                              const uint32_t* meta, const uint32_t* candidates, float* scale, uint32_t (*low)[LOW_BINS] /* LDS [2] */,
                                              uint32_t* wave_total /* LDS [4] */, Found* top, Found* mid, Found* last /* LDS [2] each */) {
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

// spans per workgroup of the histogram and candidate passes, from shapes alone: enough workgroups to fill the device, few enough that a
// sub-histogram's zeroing and flush are shared by several spans
static inline int64_t threshold_run(int64_t samples, int64_t spans) {
  const int64_t run = samples * spans / 1024;
  return run < 1 ? 1 : (run > 8 ? 8 : run);
}

}  // namespace skr
