// The step of adaptive projected guidance (include/skrample_hip.h, skr_projected_guided_step_launch): the projected prediction formed in
// registers from cond, the difference and the two per-sample coefficients of skr_projected_guidance_coef, inside the step launch.
//
//   d   = diff[e]  (the momentum buffer the statistic left)   or   rn_T(c - u)   u = inputs[slot], c = guide->cond
//   p   = rn_T( (B_s * c) + (A_s * d) )                       A_s, B_s = coef_dev[2 s], coef_dev[2 s + 1]; three separate fp32 operations
//   out = sum_k c0[k] * v_k + zeta0 * N(stream0)              v_slot = p, v_k = in_k otherwise: accumulated exactly as skr_step_launch does
//   guided_out = p                                            (when asked for)
//
//   * one-trip kernel (projected_kernel_v1<T, K, NOISE, DIFF>): whole 2048-element chunks, proj->sample_numel a multiple of 2048, one 16-
//     or 32-bit dtype, 1..16 operands, a step output.  Lane ownership, XCD chunk map, Philox numbering, fp32 tile layout and stores are
//     guided_thresholded_kernel_v1's.  A launch holds K + 1 operand images: the K operand loads and the cond load are issued in front of
//     the scheduling barrier, A_s and B_s are two scalar loads through the constant address space behind them.  DIFF is a compile-time
//     split: the image at `slot` is the difference itself (the host puts proj->diff into that operand's place, and uncond is never
//     loaded) or uncond, from which d is formed.  16-bit launches of more than 12 operands keep 12 loads in flight (11 operands and
//     cond): operand j + 11 is loaded where operand j has been summed, into the registers that frees.  `slot` is a kernarg scalar
//     compared against the unrolled operand's number, so the register arrays are never indexed at run time.
//   * general kernel (projected_kernel_gen): grid-stride, one element per lane and trip: ragged sizes, small samples, two dtype groups,
//     and the guidance-only form (no step output).
// Both evaluate the same operations in the same order on every element, so they agree bit for bit where both apply.
#include "skr_projected.h"
#include "skr_step_guided_kernel.h"

namespace skr {

template <int KMAX>
struct ProjectedArgs {  // what the first instructions need leads, as in GuidedThresholdedArgs
  const void* in[KMAX];  // in[slot]: diff under DIFF, uncond otherwise
  const void* cond;
  void* out;
  void* guided;          // nullptr: p is not stored
  int32_t xmap_lr;
  int32_t bps_shift;     // chunks per sample of the statistic (and of the draw)
  const uint64_t* seeds;
  const float* coef;     // [2 * samples]: A_s, B_s
  uint64_t stream0;
  float zeta0;
  int32_t slot;
  float c0[KMAX];
};

// operand images in flight beside cond: 16-bit launches of more than 12 operands stage the rest
template <typename T, int K>
constexpr int projected_ahead() { return (sizeof(T) == 2 && K > 12) ? 11 : K; }

template <typename T, int K, bool NOISE, bool DIFF>
__global__ __launch_bounds__(BLOCK) void projected_kernel_v1(const ProjectedArgs<guided_kmax(K)> a) {
  constexpr bool TILE = sizeof(T) == 4;
  constexpr int AHEAD = projected_ahead<T, K>();
  const uint32_t c = chunk_of(blockIdx.x, a.xmap_lr);
  const int64_t v = (int64_t)c * BLOCK + threadIdx.x;
  const int32_t slot = a.slot;
  Raw<T> raw[K];
#pragma unroll
  for (int j = 0; j < AHEAD; ++j) raw[j] = load_raw<T, TILE>(a.in[j], v);
  const Raw<T> rc = load_raw<T, TILE>(a.cond, v);
  __builtin_amdgcn_sched_barrier(0);  // every load is out before the sample's coefficients are asked for
  uint32_t smp, within;
  sample_of(c, a.bps_shift, smp, within);
  smp = __builtin_amdgcn_readfirstlane(smp);
  const float A = uniform(a.coef)[2 * smp], B = uniform(a.coef)[2 * smp + 1];  // (read-only for the launch: two scalar loads)
  float z[VEC];
  if constexpr (NOISE) {
    const uint32_t vs = within * BLOCK + threadIdx.x;  // lane-vector within the sample (sample_numel < 2^31)
    const uint64_t seed = a.seeds[smp];
    normal4(seed, a.stream0, (uint64_t)group0<TILE>((int64_t)vs), z);
    normal4(seed, a.stream0, (uint64_t)group1<TILE>((int64_t)vs), z + 4);
  }
  float acc[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    float w[VEC];
    widen<T, float>(raw[j], w);
    if (j == slot) {  // (uniform) the difference, or uncond, stands here: the projected prediction takes its place
      float cf[VEC];
      widen<T, float>(rc, cf);
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        float d = w[i];
        if constexpr (!DIFF) d = projected_diff<T>(w[i], cf[i]);
        w[i] = projected_value<T>(cf[i], d, A, B);
      }
      if (a.guided != nullptr) store8<T, float, TILE>(a.guided, v, w);  // (p is a value of T: the store's rounding is exact)
    }
    const float w0 = a.c0[j];
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = fma_(w0, w[i], acc[i]);
    if constexpr (AHEAD < K) {  // operand j + AHEAD is loaded where operand j has been summed, into the registers that frees
      if (j + AHEAD < K) raw[j + AHEAD] = load_raw<T, TILE>(a.in[j + AHEAD], v);
    }
  }
  if constexpr (NOISE) fma_noise8<float>(a.zeta0, z, acc);
  store8<T, float, TILE>(a.out, v, acc);
}

// ---- general kernel: per-element accesses, run-time dtypes, fp32 arithmetic -----------------------------------------------------------
struct ProjectedGenArgs {
  const void* in[SKR_ROW_TERMS];
  double c0[SKR_ROW_TERMS];
  const void* cond;
  const void* diff;  // nullptr: d is formed from in[slot] and cond
  void* out;         // nullptr: the guidance-only form
  void* guided;      // nullptr: p is not stored
  const uint64_t* seeds;
  const float* coef;
  double zeta0;
  uint64_t stream0;
  int64_t numel, sample_numel, stat_numel;  // the draw's sample and the statistic's (equal when the launch draws)
  int32_t n, n_a, dt_a, dt_b, dt_out, dt_g, slot, noise;
};

template <typename T>
__device__ __forceinline__ float projected_gen_value(const ProjectedGenArgs& a, int64_t e, float cv, float A, float B) {
  const float d = a.diff != nullptr ? load_scalar<T>(a.diff, e) : projected_diff<T>(load_scalar<T>(a.in[a.slot], e), cv);
  return projected_value<T>(cv, d, A, B);
}

__global__ __launch_bounds__(BLOCK) void projected_kernel_gen(const ProjectedGenArgs a) {
  for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < a.numel; e += (int64_t)gridDim.x * BLOCK) {
    const int64_t stat_smp = e / a.stat_numel;
    const float A = a.coef[2 * stat_smp], B = a.coef[2 * stat_smp + 1];
    const float cv = load_elem<float, false>(a.cond, e, a.dt_g);
    float p;
    if (a.dt_g == SKR_BF16) p = projected_gen_value<bf16_t>(a, e, cv, A, B);
    else if (a.dt_g == SKR_F16) p = projected_gen_value<f16_t>(a, e, cv, A, B);
    else p = projected_gen_value<float>(a, e, cv, A, B);
    if (a.guided != nullptr) store_any<float>(a.guided, e, a.dt_g, p);  // (p is a value of that dtype: exact)
    if (a.out == nullptr) continue;
    float acc = 0.f;
    for (int j = 0; j < a.n; ++j) {
      float w = p;
      if (j != a.slot) w = load_elem<float, false>(a.in[j], e, j < a.n_a ? a.dt_a : a.dt_b);
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

extern "C" int skr_projected_guided_step_launch(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                                const skr_step_projection* proj, const uint64_t* seeds_dev, int64_t numel, void* stream) {
  using namespace skr;
  if (!plan || !guide || !proj) return SKR_ERR_NULL;
  const skr_step_plan& p = *plan;
  const bool step_out = p.out0_dtype != SKR_NONE;
  const bool noise = step_out && p.noise_mode == 1 && p.zeta0 != 0.0;
  if (noise && numel > 0 && !seeds_dev) return SKR_ERR_NULL;
  if (p.n_terms < 0 || p.n_terms > SKR_ROW_TERMS || p.n_group_a < 0 || p.n_group_a > p.n_terms) return SKR_ERR_TERMS;
  if (guide->slot < 0 || guide->slot >= p.n_terms) return SKR_ERR_TERMS;
  if (numel < 0) return SKR_ERR_SHAPE;
  if (!step_out && !guide->guided_out) return SKR_ERR_NULL;  // no output at all
  if (p.noise_mode != 0 && p.noise_mode != 1) return SKR_ERR_UNSUPPORTED;
  if (p.out1_dtype != SKR_NONE || p.chain != 0.0 || p.zeta1 != 0.0 || p.convert_to != 0 || p.convert_from != 0 || guide->reserved != 0) return SKR_ERR_UNSUPPORTED;
  if (proj->reserved != 0 || p.acc_f64 != 0) return SKR_ERR_UNSUPPORTED;
  if (!step_out && (out != nullptr || p.n_terms != 1)) return SKR_ERR_UNSUPPORTED;  // the guidance-only form: one operand, p alone
  if (noise && numel > 0) {  // fused Philox needs every 8-element group inside one sample, as in skr_step_launch
    if (p.sample_numel <= 0 || numel % p.sample_numel != 0) return SKR_ERR_SHAPE;
    if (p.sample_numel % 8 != 0) return SKR_ERR_UNSUPPORTED;
  }
  if (proj->sample_numel < 2 || numel % proj->sample_numel != 0) return SKR_ERR_SHAPE;  // the statistic's sample, and the one the noise is drawn by
  if (noise && numel > 0 && p.sample_numel != proj->sample_numel) return SKR_ERR_SHAPE;
  if (numel == 0) return SKR_OK;
  if (!inputs || (step_out && !out) || !guide->cond || !proj->coef_dev) return SKR_ERR_NULL;
  if (const int rc = check_ptrs(inputs, p.n_terms)) return rc;
  if ((step_out && !aligned16(out)) || !aligned16(guide->cond) || !aligned16(guide->guided_out) || !aligned16(proj->diff) ||
      (reinterpret_cast<uintptr_t>(proj->coef_dev) & 3u) != 0)
    return SKR_ERR_ALIGN;
  const int32_t db = p.n_group_a == p.n_terms ? p.dtype_a : p.dtype_b;
  if (!step_inputs_ok(p.dtype_a, db, false) || (step_out && !step_output_ok(p.out0_dtype, p.dtype_a, false))) return SKR_ERR_DTYPE;  // (an fp64 tensor among them)

  constexpr int64_t CHUNK = (int64_t)BLOCK * VEC;
  const int t = p.dtype_a;
  const bool one_dtype = db == t && p.out0_dtype == t;
  const bool one_trip = g_tune.one_trip && step_out && one_dtype && (t != SKR_F32 || g_tune.tile) && p.n_terms >= 1 && numel % CHUNK == 0 &&
                        numel / CHUNK <= 0x7fffffffll && proj->sample_numel % CHUNK == 0 && proj->sample_numel < (1ll << 31);
  DeviceGuard device_guard(step_out ? out : guide->guided_out);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (one_trip) {
    const int64_t chunks = numel / CHUNK;
    with_step_type<false>(t, [&](auto tt) {
      with_bools([&](auto nz, auto df) {
        with_count<1, SKR_ROW_TERMS>(p.n_terms, [&](auto n) {
          using T = typename decltype(tt)::type;
          constexpr int N = decltype(n)::value, KMAX = guided_kmax(N);
          ProjectedArgs<KMAX> a;
          for (int k = 0; k < KMAX; ++k) { a.in[k] = k < N ? inputs[k] : nullptr; a.c0[k] = k < N ? (float)p.coef0[k] : 0.f; }
          if constexpr (decltype(df)::value) a.in[guide->slot] = proj->diff;  // the difference in uncond's place: uncond is never loaded
          a.cond = guide->cond; a.out = out; a.guided = guide->guided_out; a.seeds = seeds_dev; a.coef = proj->coef_dev;
          a.xmap_lr = xmap_lr_for(chunks); a.bps_shift = bps_shift_of(proj->sample_numel / CHUNK);
          a.stream0 = p.stream0; a.zeta0 = (float)p.zeta0; a.slot = guide->slot;
          hipLaunchKernelGGL((projected_kernel_v1<T, N, decltype(nz)::value, decltype(df)::value>), dim3((unsigned)chunks), dim3(BLOCK), 0, s, a);
        });
      }, noise, proj->diff != nullptr);
    });
  } else {
    ProjectedGenArgs a;
    for (int k = 0; k < SKR_ROW_TERMS; ++k) {
      const bool live = k < p.n_terms;
      a.in[k] = live ? inputs[k] : nullptr;
      a.c0[k] = live ? p.coef0[k] : 0.0;
    }
    a.cond = guide->cond; a.diff = proj->diff; a.out = step_out ? out : nullptr; a.guided = guide->guided_out; a.seeds = seeds_dev; a.coef = proj->coef_dev;
    a.zeta0 = p.zeta0; a.stream0 = p.stream0;
    a.numel = numel; a.sample_numel = noise ? p.sample_numel : numel; a.stat_numel = proj->sample_numel;
    a.n = p.n_terms; a.n_a = p.n_group_a; a.dt_a = p.dtype_a; a.dt_b = db; a.dt_out = p.out0_dtype;
    a.dt_g = guide->slot < p.n_group_a ? p.dtype_a : db; a.slot = guide->slot; a.noise = noise ? 1 : 0;
    hipLaunchKernelGGL(projected_kernel_gen, dim3((unsigned)grid_blocks(numel, BLOCK, 256 * 64)), dim3(BLOCK), 0, s, a);
  }
  return finish_launch();
}
