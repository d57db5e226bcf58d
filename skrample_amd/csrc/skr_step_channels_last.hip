// Channels-last step launches for MI355X (gfx950): skr_step_launch_channels_last (include/skrample_hip.h).
//
// A step is elementwise, so over operands that share one dense layout it runs on the storage order as it stands; only the fused Philox
// draw numbers a sample's elements logically.  Storage position p of a sample (plane x channels, channel innermost) is the logical
// element l(p) = (p % C) * plane + p / C, which takes lane l & 3 of Philox block l >> 2.  A launch that does not draw is skr_step_launch
// itself; a launch that draws takes one of the two kernels of this file, which give every position the bits skr_step_launch gives
// its logical element.
#include "skr_device.h"
#include "skr_channels_last.h"
#include <atomic>

namespace skr {

std::atomic<int64_t> g_cl_one_trip_launches{0}, g_cl_general_launches{0};  // skr_stat("channels_last_one_trip" / "channels_last_general")

// ---- one-trip kernel ---------------------------------------------------------------------------------------------------------------
// step_kernel_k1's unpaced Kernarg form (skr_step_fast.hip) -- a lane owns one 16-byte vector of 8 storage elements, XCD chunk map,
// every load first, scalars and Philox while they are in flight, store8 -- with the draw distributed over lane groups (cl_draw8,
// skr_channels_last.h).
template <int KMAX>
struct ClOneTripArgs {
  const void* in[KMAX];
  void* out0;
  const uint64_t* seeds;
  int32_t xmap_lr;      // log2(run length) of the XCD chunk map
  int32_t bps_shift;    // chunks per sample: sample_of
  uint64_t stream0;
  float c0[KMAX];
  float zeta0;
  uint32_t quads;       // plane / 4: Philox blocks per channel
};

template <typename T, int K, int C>
__global__ __launch_bounds__(BLOCK) void step_kernel_cl1(const ClOneTripArgs<(K <= 4 ? 4 : 8)> a) {
  static_assert(C == 4 || C == 8 || C == 16, "lane groups of 2, 4 or 8");
  const uint32_t c = chunk_of(blockIdx.x, a.xmap_lr);
  const int64_t v = (int64_t)c * BLOCK + threadIdx.x;
  Raw<T> raw[K];
#pragma unroll
  for (int j = 0; j < K; ++j) raw[j] = load_raw<T, false>(a.in[j], v);
  __builtin_amdgcn_sched_barrier(0);  // every load is out before the first scalar of the arithmetic is fetched
  float cf[K];
  const float zeta0 = a.zeta0;
  const uint64_t stream0 = a.stream0;
#pragma unroll
  for (int j = 0; j < K; ++j) cf[j] = a.c0[j];
  uint32_t smp, within;
  sample_of(c, a.bps_shift, smp, within);
  const uint64_t seed = a.seeds[smp];
  const uint32_t vs = within * BLOCK + threadIdx.x;  // lane-vector within the sample
  float z[VEC];
  cl_draw8<C>(seed, stream0, a.quads, vs, threadIdx.x, z);
  float s[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) s[i] = 0.f;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    float w[VEC];
    widen<T, float>(raw[j], w);
    const float cj = cf[j];
#pragma unroll
    for (int i = 0; i < VEC; ++i) s[i] = fma_(cj, w[i], s[i]);
  }
  if (zeta0 != 0.f) fma_noise8<float>(zeta0, z, s);
  store8<T, float, false>(a.out0, v, s);
}

// ---- general grid-stride kernel ----------------------------------------------------------------------------------------------------
// Everything else skr_step_launch draws for: two outputs with chain and zeta1, two dtype groups, fp32 / fp64 arithmetic, any channel
// count, any plane, launches that are no whole chunks.  One element per lane and trip, l(p) worked out element by element, dtypes at
// run time.  The arithmetic is step_kernel's (skr_step.hip): one fma per operand in slot order from zero, noise last, chain on the
// unrounded out0, one rounding per output.
template <typename Acc>
struct ClGeneralArgs {
  StepArgs<Acc> s;
  int64_t channels, plane;
  int32_t dtype_a, dtype_b, out0_dtype, out1_dtype;
};

__device__ __forceinline__ float pick4(const float z[4], uint32_t i) {  // z[i] without a run-time register index
  const float lo = (i & 1) ? z[1] : z[0], hi = (i & 1) ? z[3] : z[2];
  return (i & 2) ? hi : lo;
}

template <typename Acc, bool HAS1>
__global__ __launch_bounds__(BLOCK) void step_kernel_cl(const ClGeneralArgs<Acc> g) {
  constexpr bool F64 = std::is_same<Acc, double>::value;
  const StepArgs<Acc>& a = g.s;
  const int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < a.numel; e += stride) {
    const int64_t smp = e / a.sample_numel, p = e - smp * a.sample_numel;
    const int64_t x = p / g.channels, ch = p - x * g.channels;
    const uint64_t l = (uint64_t)(ch * g.plane + x);
    Acc s0 = 0, s1 = 0;
    for (int k = 0; k < a.n_terms; ++k) {
      const Acc w = load_elem<Acc, F64>(a.in[k], e, k < a.n_a ? g.dtype_a : g.dtype_b);
      s0 = fma_(a.c0[k], w, s0);
      if constexpr (HAS1) s1 = fma_(a.c1[k], w, s1);
    }
    const uint64_t seed = a.seeds[smp];
    if (a.zeta0 != (Acc)0) {
      float z[4];
      normal4(seed, a.stream0, l >> 2, z);
      s0 = fma_(a.zeta0, (Acc)pick4(z, (uint32_t)l & 3u), s0);
    }
    if constexpr (HAS1) {
      s1 = fma_(a.chain, s0, s1);
      if (a.zeta1 != (Acc)0) {
        float z[4];
        normal4(seed, a.stream1, l >> 2, z);
        s1 = fma_(a.zeta1, (Acc)pick4(z, (uint32_t)l & 3u), s1);
      }
      store_any<Acc>(a.out1, e, g.out1_dtype, s1);
    }
    if (a.out0 != nullptr) store_any<Acc>(a.out0, e, g.out0_dtype, s0);
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
int layout_check(const skr_step_plan& p, const skr_step_layout* layout) {
  if (!layout) return SKR_ERR_NULL;
  if (layout->channels < 1 || layout->plane < 1 || p.sample_numel % layout->channels != 0 || p.sample_numel / layout->channels != layout->plane)
    return SKR_ERR_SHAPE;  // (this refuses every sample_numel < 1 as well)
  return SKR_OK;
}

int channels_last_checks(const skr_step_plan& p, const skr_step_layout* layout) {
  if (const int rc = layout_check(p, layout)) return rc;
  if (plan_draws(p) && (p.convert_to != 0 || p.convert_from != 0)) return SKR_ERR_UNSUPPORTED;
  return SKR_OK;
}

// layout plays no part: no draw, or a sample whose storage order is its logical order
static bool layout_blind(const skr_step_plan& p, const skr_step_layout& l) { return !plan_draws(p) || l.channels == 1 || l.plane == 1; }

// what the one-trip kernel takes (the header's list): one output, and a sample whose Philox block numbers fit 32 bits
static bool cl_one_trip_ok(const skr_step_plan& p, const skr_step_layout& l, int64_t numel, int* bps_shift) {
  return p.out1_dtype == SKR_NONE && cl_one_trip_geometry(p, l, numel, 1ll << 32, bps_shift);
}

template <typename T>
static int launch_cl1(const skr_step_plan& p, const skr_step_layout& l, const void* const* inputs, void* out0, const uint64_t* seeds, int64_t numel,
                      int bps_shift, hipStream_t stream) {
  const int64_t chunks = numel / ((int64_t)BLOCK * VEC);
  float c0[8];
  for (int k = 0; k < p.n_terms; ++k) c0[k] = (float)p.coef0[k];
  with_count<1, 8>(p.n_terms, [&](auto n) {
    constexpr int N = decltype(n)::value;
    ClOneTripArgs<(N <= 4 ? 4 : 8)> fa;
    fill_operands(inputs, c0, N, fa.in, fa.c0);
    fa.out0 = out0; fa.seeds = seeds; fa.zeta0 = (float)p.zeta0; fa.stream0 = p.stream0;
    fa.bps_shift = bps_shift; fa.xmap_lr = xmap_lr_for(chunks); fa.quads = (uint32_t)(l.plane / 4);
    const dim3 grid((unsigned)chunks), block(BLOCK);
    with_channels(l.channels, [&](auto c) { hipLaunchKernelGGL((step_kernel_cl1<T, N, decltype(c)::value>), grid, block, 0, stream, fa); });
  });
  return finish_launch();
}

template <typename Acc>
static int launch_cl_general(const skr_step_plan& p, const skr_step_layout& l, const void* const* inputs, void* out0, void* out1, const uint64_t* seeds,
                             int64_t numel, hipStream_t stream) {
  constexpr bool F64 = std::is_same<Acc, double>::value;
  const int32_t da = p.dtype_a, db = p.n_group_a == p.n_terms ? p.dtype_a : p.dtype_b;
  const bool st0 = p.out0_dtype != SKR_NONE, has1 = p.out1_dtype != SKR_NONE;
  if (!step_inputs_ok(da, db, F64)) return SKR_ERR_DTYPE;
  if ((st0 && !step_output_ok(p.out0_dtype, da, F64)) || (has1 && !step_output_ok(p.out1_dtype, da, F64))) return SKR_ERR_DTYPE;
  ClGeneralArgs<Acc> g;
  StepArgs<Acc>& a = g.s;
  memset(&g, 0, sizeof g);
  for (int k = 0; k < p.n_terms; ++k) { a.in[k] = inputs[k]; a.c0[k] = (Acc)p.coef0[k]; a.c1[k] = (Acc)p.coef1[k]; }
  a.out0 = st0 ? out0 : nullptr; a.out1 = has1 ? out1 : nullptr; a.seeds = seeds;
  a.chain = (Acc)p.chain; a.zeta0 = (Acc)p.zeta0; a.zeta1 = has1 ? (Acc)p.zeta1 : (Acc)0;
  a.stream0 = p.stream0; a.stream1 = p.stream1;
  a.numel = numel; a.sample_numel = p.sample_numel;
  a.n_a = p.n_group_a; a.n_terms = p.n_terms;
  g.channels = l.channels; g.plane = l.plane;
  g.dtype_a = da; g.dtype_b = db; g.out0_dtype = p.out0_dtype; g.out1_dtype = p.out1_dtype;
  const dim3 grid((unsigned)grid_blocks(numel, BLOCK, 256 * 32)), block(BLOCK);
  if (has1) hipLaunchKernelGGL((step_kernel_cl<Acc, true>), grid, block, 0, stream, g);
  else hipLaunchKernelGGL((step_kernel_cl<Acc, false>), grid, block, 0, stream, g);
  return finish_launch();
}

}  // namespace skr

extern "C" int skr_step_launch_channels_last(const skr_step_plan* plan, const void* const* inputs, void* out0, void* out1,
                                             const uint64_t* seeds_dev, const skr_step_layout* layout, int64_t numel, void* stream) {
  skr::DeviceGuard device_guard(out0 ? out0 : out1);
  bool empty = false;
  if (const int rc = skr::step_launch_checks(plan, inputs, out0, out1, seeds_dev, numel, skr::RowForm::Kernarg, nullptr, nullptr, empty)) return rc;
  const skr_step_plan& p = *plan;
  if (const int rc = skr::channels_last_checks(p, layout)) return rc;
  if (empty) return SKR_OK;
  if (skr::layout_blind(p, *layout)) return skr_step_launch(plan, inputs, out0, out1, seeds_dev, numel, stream);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int bps_shift = 0;
  if (skr::cl_one_trip_ok(p, *layout, numel, &bps_shift)) {
    ++skr::g_cl_one_trip_launches;
    return p.dtype_a == SKR_BF16 ? skr::launch_cl1<skr::bf16_t>(p, *layout, inputs, out0, seeds_dev, numel, bps_shift, s)
                                 : skr::launch_cl1<skr::f16_t>(p, *layout, inputs, out0, seeds_dev, numel, bps_shift, s);
  }
  ++skr::g_cl_general_launches;
  return p.acc_f64 ? skr::launch_cl_general<double>(p, *layout, inputs, out0, out1, seeds_dev, numel, s)
                   : skr::launch_cl_general<float>(p, *layout, inputs, out0, out1, seeds_dev, numel, s);
}
