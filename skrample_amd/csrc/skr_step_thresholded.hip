// The thresholded solver step (include/skrample_hip.h, skr_thresholded_step_launch): Imagen-style dynamic thresholding fused into the step
// launch, a sibling of the guided step (skr_step_guided.hip) under the same plan contract.
//
//   x0  = rn32( rn32(a x) + rn32(b o) )                  x = inputs[xslot], o = inputs[slot]; a, b narrowed to fp32 once (x0_value)
//   p   = rn_T( min(max(x0, -s), s) / s )                s = scale_dev[sample], what skr_threshold_scale wrote (1 without one)
//   out = sum_k c0[k] * v_k + zeta0 * N(stream0)         v_slot = p, v_k = in_k otherwise (x among them, with its own coefficient):
//                                                        accumulated exactly as skr_step_launch does
//   x0_out = p                                           (when asked for: what history and pred_original_sample read)
//
//   * one-trip kernel (thresholded_kernel_v1<T, K, NOISE>): whole 2048-element chunks, thr->sample_numel a multiple of 2048 -- a workgroup
//     then lies inside one sample and s is one uniform load behind the operand loads --, one 16- or 32-bit dtype, <= 16 operands.  Lane
//     ownership, XCD chunk map, loads, stores and Philox numbering are guided_kernel_v1's.  `slot` and `xslot` are kernarg scalars that
//     each unrolled operand compares its own number with, so the register arrays are never indexed at run time; whether the step output
//     and p are stored are uniform branches on the pointers (the thresholding-only form takes this kernel too: it is UniPC's hot path).
//   * general kernel (thresholded_kernel_gen): grid-stride, one element per lane and trip: ragged sizes, small samples, two dtype groups.
// Both evaluate the same operations in the same order on every element, so they agree bit for bit where both apply.
#include "skr_threshold.h"
#include "skr_step_guided_kernel.h"

namespace skr {

template <int KMAX>
struct ThresholdedArgs {  // what the first instructions need leads, as in GuidedArgs
  const void* in[KMAX];
  void* out;            // nullptr: the thresholding-only form
  void* x0_out;         // nullptr: p is not stored
  int32_t xmap_lr;
  int32_t bps_shift;    // chunks per sample of the statistic (and of the draw)
  const uint64_t* seeds;
  const float* scale;   // nullptr: s = 1
  uint64_t stream0;
  float zeta0;
  float a, b;
  int32_t slot, xslot;
  float c0[KMAX];
};

template <typename T, int K, bool NOISE>
__global__ __launch_bounds__(BLOCK) void thresholded_kernel_v1(const ThresholdedArgs<guided_kmax(K)> a) {
  constexpr bool TILE = sizeof(T) == 4;
  const uint32_t c = chunk_of(blockIdx.x, a.xmap_lr);
  const int64_t v = (int64_t)c * BLOCK + threadIdx.x;
  Raw<T> raw[K];
#pragma unroll
  for (int j = 0; j < K; ++j) raw[j] = load_raw<T, TILE>(a.in[j], v);
  __builtin_amdgcn_sched_barrier(0);  // every load is out before the sample's scale is asked for
  uint32_t smp, within;
  sample_of(c, a.bps_shift, smp, within);
  smp = __builtin_amdgcn_readfirstlane(smp);
  const float s = a.scale != nullptr ? uniform(a.scale)[smp] : 1.f;  // (read-only for the launch: a scalar load)
  const int32_t slot = a.slot, xslot = a.xslot;
  float z[VEC];
  if constexpr (NOISE) {
    const uint32_t vs = within * BLOCK + threadIdx.x;  // lane-vector within the sample (sample_numel < 2^31)
    const uint64_t seed = a.seeds[smp];
    normal4(seed, a.stream0, (uint64_t)group0<TILE>((int64_t)vs), z);
    normal4(seed, a.stream0, (uint64_t)group1<TILE>((int64_t)vs), z + 4);
  }
  float x[VEC];
#pragma unroll
  for (int j = 0; j < K; ++j) if (j == xslot) widen<T, float>(raw[j], x);  // (uniform: a kernarg scalar against the unrolled operand's number)
  float acc[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
  const bool step_out = a.out != nullptr;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    float w[VEC];
    widen<T, float>(raw[j], w);
    if (j == slot) {  // (uniform) the thresholded prediction takes this operand's place
#pragma unroll
      for (int i = 0; i < VEC; ++i) w[i] = thresholded_value<T>(x0_value(a.a, x[i], a.b, w[i]), s);
      if (a.x0_out != nullptr) store8<T, float, TILE>(a.x0_out, v, w);  // (p is a value of T: the store's rounding is exact)
    }
    if (step_out) {
      const float w0 = a.c0[j];
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = fma_(w0, w[i], acc[i]);
    }
  }
  if (!step_out) return;
  if constexpr (NOISE) fma_noise8<float>(a.zeta0, z, acc);
  store8<T, float, TILE>(a.out, v, acc);
}

// ---- general kernel: per-element accesses, run-time dtypes, fp32 arithmetic -----------------------------------------------------------
struct ThresholdedGenArgs {
  const void* in[SKR_ROW_TERMS];
  double c0[SKR_ROW_TERMS];
  void* out;      // nullptr: the thresholding-only form
  void* x0_out;   // nullptr: p is not stored
  const uint64_t* seeds;
  const float* scale;
  double zeta0;
  uint64_t stream0;
  int64_t numel, sample_numel, stat_numel;  // the draw's sample and the statistic's (equal when the launch draws)
  float a, b;
  int32_t n, n_a, dt_a, dt_b, dt_out, dt_g, dt_x, slot, xslot, noise;
};

__global__ __launch_bounds__(BLOCK) void thresholded_kernel_gen(const ThresholdedGenArgs a) {
  for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < a.numel; e += (int64_t)gridDim.x * BLOCK) {
    const float s = a.scale != nullptr ? a.scale[e / a.stat_numel] : 1.f;
    const float x = load_elem<float, false>(a.in[a.xslot], e, a.dt_x), o = load_elem<float, false>(a.in[a.slot], e, a.dt_g);
    const float x0 = x0_value(a.a, x, a.b, o);
    float p;
    if (a.dt_g == SKR_BF16) p = thresholded_value<bf16_t>(x0, s);
    else if (a.dt_g == SKR_F16) p = thresholded_value<f16_t>(x0, s);
    else p = thresholded_value<float>(x0, s);
    if (a.x0_out != nullptr) store_any<float>(a.x0_out, e, a.dt_g, p);  // (p is a value of that dtype: exact)
    if (a.out == nullptr) continue;
    float acc = 0.f;
    for (int j = 0; j < a.n; ++j) {
      float w = load_elem<float, false>(a.in[j], e, j < a.n_a ? a.dt_a : a.dt_b);
      if (j == a.slot) w = p;
      acc = fma_((float)a.c0[j], w, acc);
    }
    if (a.noise) {  // element r of the sample: Philox block r >> 2, lane r & 3 (sample_numel % 8 == 0, checked on the host)
      const int64_t smp = e / a.sample_numel, r = e - smp * a.sample_numel;
      float z[4];
      normal4(a.seeds[smp], a.stream0, (uint64_t)r >> 2, z);
      const int lane = (int)(r & 3);
      const float zz = lane == 0 ? z[0] : (lane == 1 ? z[1] : (lane == 2 ? z[2] : z[3]));
      acc = fma_((float)a.zeta0, zz, acc);
    }
    store_any<float>(a.out, e, a.dt_out, acc);
  }
}

}  // namespace skr

extern "C" int skr_thresholded_step_launch(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_threshold* thr,
                                           const uint64_t* seeds_dev, int64_t numel, void* stream) {
  using namespace skr;
  if (!plan || !thr) return SKR_ERR_NULL;
  const skr_step_plan& p = *plan;
  const bool step_out = p.out0_dtype != SKR_NONE;
  const bool noise = step_out && p.noise_mode == 1 && p.zeta0 != 0.0;
  if (noise && numel > 0 && !seeds_dev) return SKR_ERR_NULL;
  if (p.n_terms < 0 || p.n_terms > SKR_ROW_TERMS || p.n_group_a < 0 || p.n_group_a > p.n_terms) return SKR_ERR_TERMS;
  if (thr->slot < 0 || thr->slot >= p.n_terms || thr->xslot < 0 || thr->xslot >= p.n_terms || thr->slot == thr->xslot) return SKR_ERR_TERMS;
  if (numel < 0) return SKR_ERR_SHAPE;
  if (!step_out && !thr->x0_out) return SKR_ERR_NULL;  // no output at all
  if (p.noise_mode != 0 && p.noise_mode != 1) return SKR_ERR_UNSUPPORTED;
  if (p.out1_dtype != SKR_NONE || p.chain != 0.0 || p.zeta1 != 0.0 || p.convert_to != 0 || p.convert_from != 0 || thr->reserved != 0) return SKR_ERR_UNSUPPORTED;
  if (p.acc_f64 != 0) return SKR_ERR_UNSUPPORTED;
  if (!step_out && (out != nullptr || p.n_terms != 2)) return SKR_ERR_UNSUPPORTED;  // the thresholding-only form: the two operands, p alone
  if (noise && numel > 0) {  // fused Philox needs every 8-element group inside one sample, as in skr_step_launch
    if (p.sample_numel <= 0 || numel % p.sample_numel != 0) return SKR_ERR_SHAPE;
    if (p.sample_numel % 8 != 0) return SKR_ERR_UNSUPPORTED;
  }
  if (thr->sample_numel < 1 || numel % thr->sample_numel != 0) return SKR_ERR_SHAPE;
  if (noise && numel > 0 && p.sample_numel != thr->sample_numel) return SKR_ERR_SHAPE;
  if (numel == 0) return SKR_OK;
  if (!inputs || (step_out && !out)) return SKR_ERR_NULL;
  if (const int rc = check_ptrs(inputs, p.n_terms)) return rc;
  if ((step_out && !aligned16(out)) || !aligned16(thr->x0_out) || (reinterpret_cast<uintptr_t>(thr->scale_dev) & 3u) != 0) return SKR_ERR_ALIGN;
  const int32_t db = p.n_group_a == p.n_terms ? p.dtype_a : p.dtype_b;
  if (p.dtype_a == SKR_F64 || db == SKR_F64 || p.out0_dtype == SKR_F64) return SKR_ERR_UNSUPPORTED;
  if (!step_inputs_ok(p.dtype_a, db, false) || (step_out && !step_output_ok(p.out0_dtype, p.dtype_a, false))) return SKR_ERR_DTYPE;

  constexpr int64_t CHUNK = (int64_t)BLOCK * VEC;
  const int t = p.dtype_a;
  const bool one_dtype = db == t && (!step_out || p.out0_dtype == t);
  const bool one_trip = g_tune.one_trip && one_dtype && (t != SKR_F32 || g_tune.tile) && numel % CHUNK == 0 && numel / CHUNK <= 0x7fffffffll &&
                        thr->sample_numel % CHUNK == 0 && thr->sample_numel < (1ll << 31);
  DeviceGuard device_guard(step_out ? out : thr->x0_out);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (one_trip) {
    const int64_t chunks = numel / CHUNK;
    with_step_type<false>(t, [&](auto tt) {
      with_bools([&](auto nz) {
        with_count<2, SKR_ROW_TERMS>(p.n_terms, [&](auto n) {
          using T = typename decltype(tt)::type;
          constexpr int N = decltype(n)::value, KMAX = guided_kmax(N);
          ThresholdedArgs<KMAX> a;
          for (int k = 0; k < KMAX; ++k) { a.in[k] = k < N ? inputs[k] : nullptr; a.c0[k] = k < N ? (float)p.coef0[k] : 0.f; }
          a.out = step_out ? out : nullptr; a.x0_out = thr->x0_out; a.seeds = seeds_dev; a.scale = thr->scale_dev;
          a.xmap_lr = xmap_lr_for(chunks); a.bps_shift = bps_shift_of(thr->sample_numel / CHUNK);
          a.stream0 = p.stream0; a.zeta0 = (float)p.zeta0; a.a = (float)thr->a; a.b = (float)thr->b; a.slot = thr->slot; a.xslot = thr->xslot;
          hipLaunchKernelGGL((thresholded_kernel_v1<T, N, decltype(nz)::value>), dim3((unsigned)chunks), dim3(BLOCK), 0, s, a);
        });
      }, noise);
    });
  } else {
    ThresholdedGenArgs a;
    for (int k = 0; k < SKR_ROW_TERMS; ++k) {
      const bool live = k < p.n_terms;
      a.in[k] = live ? inputs[k] : nullptr;
      a.c0[k] = live ? p.coef0[k] : 0.0;
    }
    a.out = step_out ? out : nullptr; a.x0_out = thr->x0_out; a.seeds = seeds_dev; a.scale = thr->scale_dev;
    a.zeta0 = p.zeta0; a.stream0 = p.stream0;
    a.numel = numel; a.sample_numel = noise ? p.sample_numel : numel; a.stat_numel = thr->sample_numel;
    a.a = (float)thr->a; a.b = (float)thr->b;
    a.n = p.n_terms; a.n_a = p.n_group_a; a.dt_a = p.dtype_a; a.dt_b = db; a.dt_out = p.out0_dtype;
    a.dt_g = thr->slot < p.n_group_a ? p.dtype_a : db; a.dt_x = thr->xslot < p.n_group_a ? p.dtype_a : db;
    a.slot = thr->slot; a.xslot = thr->xslot; a.noise = noise ? 1 : 0;
    hipLaunchKernelGGL(thresholded_kernel_gen, dim3((unsigned)grid_blocks(numel, BLOCK, 256 * 64)), dim3(BLOCK), 0, s, a);
  }
  return finish_launch();
}
