// The guided solver step (include/skrample_hip.h, skr_step_launch_guided): classifier-free guidance fused into the step launch.
//
//   p   = rn_T( u + rn_T( g * rn_T(c - u) ) )       u = inputs[slot], c = cond: torch's three tensor ops, one rounded op at a time in
//                                                   the op-math type of T (fp32; fp64 for fp64 tensors), g converted to it once
//   out = sum_k c0[k]*v_k + zeta0*N(stream0)        v_slot = p, v_k = in_k otherwise: accumulated exactly as skr_step_launch does
//   guided_out = p                                  (when asked for: the tensor the unfused loop hands to the step and keeps as history)
//
//   * one-trip kernel (guided_kernel_v1<T, K, NOISE>): whole 2048-element chunks, samples made of whole chunks when it draws, operands /
//     cond / both outputs of one 16- or 32-bit dtype, fp32 arithmetic, <= 16 operands.  Lane ownership, XCD chunk map, loads, stores and
//     Philox block numbering are those of masked_kernel_v1's kernarg form (skr_step_masked.hip): every operand load is issued first, the
//     cond vector right behind them, the scalars and the Philox rounds while they are in flight.  `slot` is a kernarg scalar: each
//     unrolled operand compares its own number with it (a uniform branch), so the register arrays are never indexed at run time.
//     Whether p is stored is a uniform branch on the pointer, not a template flag: 3 dtypes x 16 operand counts x 2 (noise) = 96 instantiations.
//   * general kernel (guided_kernel_gen): grid-stride, one element per lane and trip, any size, any dtype combination skr_step_launch
//     takes, fp32 or fp64 arithmetic, and the guidance-only form (no step output).
// Both evaluate the same operations in the same order on every element, so they agree bit for bit where both apply.
// One exception follows torch's own device op: for fp16 the elements past the last whole 2048 of the tensor have  g * d  rounded once
// (mul_once_f16, skr_step_guided.h).  Only the general kernel meets such elements.
// The row forms of the one-trip kernel (skr_step_launch_guided_indexed[_per_sample]) are skr_step_guided_rows.hip, the rescaled step
// (skr_step_launch_guided_rescaled) skr_step_guided_rescaled.hip; the guided value and the entry checks, which they share, are
// skr_step_guided.h.
#include "skr_step_guided.h"
#include "skr_device.h"

namespace skr {

// Kernarg of the one-trip kernel: what the first instructions need (operand pointers, chunk map) leads, as in MaskedArgs.
template <int KMAX>
struct GuidedArgs {
  const void* in[KMAX];
  const void* cond;
  void* out;
  void* guided;         // nullptr: p is not stored
  int32_t xmap_lr;      // log2(run length) of the XCD chunk map
  int32_t bps_shift;    // chunks per sample: log2 when >= 0, minus the count otherwise (see sample_of); read by a launch that draws only
  const uint64_t* seeds;
  uint64_t stream0;
  float zeta0;
  float scale;          // g in the op-math type
  int32_t slot;         // the operand that p replaces in the sum
  float c0[KMAX];
};

template <typename T, int K, bool NOISE>
__global__ __launch_bounds__(BLOCK) void guided_kernel_v1(const GuidedArgs<guided_kmax(K)> a) {
  constexpr bool TILE = sizeof(T) == 4;  // whole chunks are whole tiles: 32-bit tensors take the whole-line layout, as in launch_k1
  const uint32_t c = chunk_of(blockIdx.x, a.xmap_lr);
  const int64_t v = (int64_t)c * BLOCK + threadIdx.x;
  Raw<T> raw[K];
#pragma unroll
  for (int j = 0; j < K; ++j) raw[j] = load_raw<T, TILE>(a.in[j], v);
  Raw<T> rc = load_raw<T, TILE>(a.cond, v);
  __builtin_amdgcn_sched_barrier(0);  // every load is out before the first scalar of the arithmetic is fetched
  float c0[K];
#pragma unroll
  for (int j = 0; j < K; ++j) c0[j] = a.c0[j];
  const float zeta0 = a.zeta0, g = a.scale;
  const int32_t slot = a.slot;
  float z[VEC];
  if constexpr (NOISE) {
    uint32_t smp, within;
    sample_of(c, a.bps_shift, smp, within);
    const uint32_t vs = within * BLOCK + threadIdx.x;  // lane-vector within the sample (sample_numel < 2^31)
    const uint64_t seed = a.seeds[smp];
    normal4(seed, a.stream0, (uint64_t)group0<TILE>((int64_t)vs), z);
    normal4(seed, a.stream0, (uint64_t)group1<TILE>((int64_t)vs), z + 4);
  }
  float s[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) s[i] = 0.f;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    float w[VEC];
    widen<T, float>(raw[j], w);
    if (j == slot) {  // (uniform: a kernarg scalar against the unrolled operand's number) the guided value takes this operand's place
      float cf[VEC];
      widen<T, float>(rc, cf);
#pragma unroll
      for (int i = 0; i < VEC; ++i) w[i] = guided_value<T>(w[i], cf[i], g);
      if (a.guided != nullptr) store8<T, float, TILE>(a.guided, v, w);  // (p is a value of T: the store's rounding is exact)
    }
    const float w0 = c0[j];
#pragma unroll
    for (int i = 0; i < VEC; ++i) s[i] = fma_(w0, w[i], s[i]);
  }
  if constexpr (NOISE) fma_noise8<float>(zeta0, z, s);
  store8<T, float, TILE>(a.out, v, s);
}

// ---- general kernel: per-element accesses, run-time dtypes -----------------------------------------------------------------
struct GuidedGenArgs {
  const void* in[SKR_ROW_TERMS];
  double c0[SKR_ROW_TERMS];
  const void* cond;
  void* out;      // nullptr: the guidance-only form
  void* guided;   // nullptr: p is not stored
  const uint64_t* seeds;
  double zeta0, scale;
  uint64_t stream0;
  int64_t numel, sample_numel;
  int32_t n, n_a, dt_a, dt_b, dt_out, dt_g, slot, noise;
};

template <typename Acc>
__global__ __launch_bounds__(BLOCK) void guided_kernel_gen(const GuidedGenArgs a) {
  constexpr bool F64 = std::is_same<Acc, double>::value;  // (an fp64 tensor takes part in fp64 arithmetic only)
  const int64_t tail_from = a.numel - a.numel % TORCH_TAIL;  // fp16: torch rounds g * d once from here on (mul_once_f16)
  for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < a.numel; e += (int64_t)gridDim.x * BLOCK) {
    // the guided value, in the op-math type of the slot's dtype whatever the accumulate type is; then widened exactly
    Acc p;
    bool wide_p = false;
    if constexpr (F64) wide_p = a.dt_g == SKR_F64;
    if (wide_p) {
      const double* up = reinterpret_cast<const double*>(a.in[a.slot]);
      const double* cp = reinterpret_cast<const double*>(a.cond);
      p = (Acc)guide_d(up[e], cp[e], a.scale);
    } else {
      const float u = load_elem<float, false>(a.in[a.slot], e, a.dt_g), cv = load_elem<float, false>(a.cond, e, a.dt_g);
      const float g = (float)a.scale;
      float pf;
      if (a.dt_g == SKR_BF16) pf = guided_value<bf16_t>(u, cv, g);
      else if (a.dt_g == SKR_F16) pf = e >= tail_from ? guided_value_f16_tail(u, cv, g) : guided_value<f16_t>(u, cv, g);
      else pf = guided_value<float>(u, cv, g);
      p = (Acc)pf;
    }
    if (a.guided != nullptr) store_any<Acc>(a.guided, e, a.dt_g, p);  // (p is a value of that dtype: exact)
    if (a.out == nullptr) continue;
    Acc s = 0;
    for (int j = 0; j < a.n; ++j) {
      Acc x = load_elem<Acc, F64>(a.in[j], e, j < a.n_a ? a.dt_a : a.dt_b);
      if (j == a.slot) x = p;
      s = fma_((Acc)a.c0[j], x, s);
    }
    if (a.noise) {  // element r of the sample: Philox block r >> 2, lane r & 3 (sample_numel % 8 == 0, checked on the host)
      const int64_t smp = e / a.sample_numel, r = e - smp * a.sample_numel;
      float z[4];
      normal4(a.seeds[smp], a.stream0, (uint64_t)r >> 2, z);
      const int lane = (int)(r & 3);
      const float zz = lane == 0 ? z[0] : (lane == 1 ? z[1] : (lane == 2 ? z[2] : z[3]));
      s = fma_((Acc)a.zeta0, (Acc)zz, s);
    }
    store_any<Acc>(a.out, e, a.dt_out, s);
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// the one-trip launch: dtype x noise x operand count to the instantiation, and its kernarg
static void launch_guided_v1(const skr_step_plan& p, const void* const* inputs, void* out, const skr_step_guidance& gd, const uint64_t* seeds, bool noise,
                             int64_t chunks, int bps_shift, hipStream_t s) {
  with_step_type<false>(p.dtype_a, [&](auto tt) {
    with_bools([&](auto nz) {
      with_count<1, SKR_ROW_TERMS>(p.n_terms, [&](auto n) {
        using T = typename decltype(tt)::type;
        constexpr int N = decltype(n)::value, KMAX = guided_kmax(N);
        GuidedArgs<KMAX> a;
        for (int k = 0; k < KMAX; ++k) { a.in[k] = k < N ? inputs[k] : nullptr; a.c0[k] = k < N ? (float)p.coef0[k] : 0.f; }
        a.cond = gd.cond; a.out = out; a.guided = gd.guided_out; a.seeds = seeds;
        a.xmap_lr = xmap_lr_for(chunks); a.bps_shift = bps_shift;
        a.stream0 = p.stream0; a.zeta0 = (float)p.zeta0; a.scale = (float)gd.scale; a.slot = gd.slot;
        hipLaunchKernelGGL((guided_kernel_v1<T, N, decltype(nz)::value>), dim3((unsigned)chunks), dim3(BLOCK), 0, s, a);
      });
    }, noise);
  });
}

// Every check of a guided launch behind its NULL plan / guide tests: those of skr_step_launch in its order, with what the guidance adds
// where the like of it stands there.  (Declared in skr_step_guided.h: the row entries ask it too.)
int guided_prepare(const skr_step_plan& p, const skr_step_guidance& gd, const void* const* inputs, void* out, const uint64_t* seeds_dev, int64_t numel,
                   bool rows, GuidedLaunch* launch, const skr_step_rescale* rescale) {
  launch->step_out = launch->noise = launch->one_trip = false;
  const bool step_out = p.out0_dtype != SKR_NONE;
  const bool noise = step_out && p.noise_mode == 1 && (rows || p.zeta0 != 0.0);
  if (noise && numel > 0 && !seeds_dev) return SKR_ERR_NULL;
  if (p.n_terms < 0 || p.n_terms > SKR_ROW_TERMS || p.n_group_a < 0 || p.n_group_a > p.n_terms) return SKR_ERR_TERMS;
  if (gd.slot < 0 || gd.slot >= p.n_terms) return SKR_ERR_TERMS;
  if (numel < 0) return SKR_ERR_SHAPE;
  if (!step_out && !gd.guided_out) return SKR_ERR_NULL;  // no output at all
  if (p.noise_mode != 0 && p.noise_mode != 1) return SKR_ERR_UNSUPPORTED;
  if (p.out1_dtype != SKR_NONE || p.chain != 0.0 || p.zeta1 != 0.0 || p.convert_to != 0 || p.convert_from != 0 || gd.reserved != 0) return SKR_ERR_UNSUPPORTED;
  if (rescale && rescale->reserved != 0) return SKR_ERR_UNSUPPORTED;
  if (!step_out && (out != nullptr || p.n_terms != 1)) return SKR_ERR_UNSUPPORTED;  // the guidance-only form: one operand, p alone
  if (noise && numel > 0) {  // fused Philox needs every 8-element group inside one sample, as in skr_step_launch
    if (p.sample_numel <= 0 || numel % p.sample_numel != 0) return SKR_ERR_SHAPE;
    if (p.sample_numel % 8 != 0) return SKR_ERR_UNSUPPORTED;
  }
  if (rescale) {  // the statistic's sample: at least two elements (an unbiased std), and the one the noise is drawn by
    if (rescale->sample_numel < 2 || numel % rescale->sample_numel != 0) return SKR_ERR_SHAPE;
    if (noise && numel > 0 && p.sample_numel != rescale->sample_numel) return SKR_ERR_SHAPE;
  }
  if (numel == 0) return SKR_OK;
  if (!inputs || (step_out && !out) || !gd.cond || (rescale && !rescale->factor_dev)) return SKR_ERR_NULL;
  if (const int rc = check_ptrs(inputs, p.n_terms)) return rc;
  if ((step_out && !aligned16(out)) || !aligned16(gd.cond) || !aligned16(gd.guided_out)) return SKR_ERR_ALIGN;
  // the dtype combinations of skr_step_launch, with one output; an fp64 group (the slot's or not) needs fp64 arithmetic
  const int32_t db = p.n_group_a == p.n_terms ? p.dtype_a : p.dtype_b;
  if (!step_inputs_ok(p.dtype_a, db, p.acc_f64) || (step_out && !step_output_ok(p.out0_dtype, p.dtype_a, p.acc_f64))) return SKR_ERR_DTYPE;
  launch->step_out = step_out; launch->noise = noise;
  launch->dtype_b = db; launch->dtype_g = gd.slot < p.n_group_a ? p.dtype_a : db;

  constexpr int64_t CHUNK = (int64_t)BLOCK * VEC;
  const int t = p.dtype_a;
  const bool one_dtype = db == t && p.out0_dtype == t && t != SKR_F64;
  if (g_tune.one_trip && step_out && !p.acc_f64 && one_dtype && (t != SKR_F32 || g_tune.tile) && numel % CHUNK == 0 && numel / CHUNK <= 0x7fffffffll &&
      (!noise || (p.sample_numel % CHUNK == 0 && p.sample_numel < (1ll << 31)))) {
    launch->one_trip = true; launch->chunks = numel / CHUNK; launch->bps_shift = noise ? bps_shift_of(p.sample_numel / CHUNK) : 0;
  }
  return SKR_OK;
}

static int guided_launch_impl(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide, const uint64_t* seeds_dev,
                              int64_t numel, void* stream) {
  if (!plan || !guide) return SKR_ERR_NULL;
  const skr_step_plan& p = *plan;
  const skr_step_guidance& gd = *guide;
  GuidedLaunch l;
  if (const int rc = guided_prepare(p, gd, inputs, out, seeds_dev, numel, false, &l)) return rc;
  if (numel == 0) return SKR_OK;
  const bool step_out = l.step_out, noise = l.noise;
  const int32_t db = l.dtype_b, dt_g = l.dtype_g;

  DeviceGuard device_guard(step_out ? out : gd.guided_out);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (l.one_trip) {
    launch_guided_v1(p, inputs, out, gd, seeds_dev, noise, l.chunks, l.bps_shift, s);
    return finish_launch();
  }

  GuidedGenArgs a;
  for (int k = 0; k < SKR_ROW_TERMS; ++k) {
    const bool live = k < p.n_terms;
    a.in[k] = live ? inputs[k] : nullptr;
    a.c0[k] = live ? p.coef0[k] : 0.0;
  }
  a.cond = gd.cond; a.out = step_out ? out : nullptr; a.guided = gd.guided_out; a.seeds = seeds_dev;
  a.zeta0 = p.zeta0; a.scale = gd.scale; a.stream0 = p.stream0;
  a.numel = numel; a.sample_numel = noise ? p.sample_numel : numel;
  a.n = p.n_terms; a.n_a = p.n_group_a; a.dt_a = p.dtype_a; a.dt_b = db; a.dt_out = p.out0_dtype; a.dt_g = dt_g; a.slot = gd.slot;
  a.noise = noise ? 1 : 0;
  const dim3 grid((unsigned)grid_blocks(numel, BLOCK, 256 * 64));
  with_bools([&](auto f64) { hipLaunchKernelGGL((guided_kernel_gen<std::conditional_t<decltype(f64)::value, double, float>>), grid, dim3(BLOCK), 0, s, a); }, p.acc_f64 != 0);
  return finish_launch();
}

}  // namespace skr

extern "C" int skr_step_launch_guided(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                      const uint64_t* seeds_dev, int64_t numel, void* stream) {
  return skr::guided_launch_impl(plan, inputs, out, guide, seeds_dev, numel, stream);
}
