// The rescaled guided step (include/skrample_hip.h, skr_step_launch_guided_rescaled): skr_step_launch_guided with the guided prediction p
// replaced by diffusers' rescale_noise_cfg of it, the per-sample factor r = rn_T(std(cond) / std(p)) coming from the statistics launch
// (skr_guidance_stats.hip):
//
//   resc = rn_T(p * r);   a = rn_T(phi * resc);   b = rn_T(psi * p);   p' = rn_T(a + b)        psi = 1 - phi, formed in double
//   out = sum_k c0[k]*v_k + zeta0*N(stream0)        v_slot = p', v_k = in_k otherwise
//   guided_out = p'
//
//   * one-trip kernel (guided_rescaled_kernel_v1<T, K, NOISE>): guided_kernel_v1 (skr_step_guided.hip) -- same lane ownership, XCD chunk
//     map, loads ahead of the barrier, `slot` compared per unrolled operand, fp32 tile layout -- where the statistic's sample is made of
//     whole 2048-element chunks: a workgroup then lies inside one sample, and its factor is one uniform load behind the operand loads.
//   * general kernel (guided_rescaled_kernel_gen): guided_kernel_gen with the same four operations; ragged sizes, small samples, two dtype
//     groups, fp64, the guidance-only form.  For fp16 the two scalar products are torch's tensor-times-number kernel, as g * d is: from
//     the last multiple of 2048 below numel on they are rounded once (mul_once_f16, skr_step_guided.h).
// Both evaluate the same operations in the same order on every element, so they agree bit for bit where both apply.
#include "skr_step_guided.h"
#include "skr_device.h"

namespace skr {

// fp16 elements of the partial last block of torch's elementwise kernels: the scalar products are rounded once (p * r is exact in fp32,
// a + b is a sum of two fp16 values: neither is changed by its second rounding).  Measured against torch on the device: the fused
// multiply-and-convert of that block is a multiply-ADD with +0 (v_fma_mixlo_f16 k, x, 0), so a product that is exactly zero comes out
// as +0 whatever its sign -- (-0) + (+0) = +0 -- while a product that only underflows in the rounding keeps its sign.  It shows where
// phi or psi is 0: psi * p = 0 * (negative p) is +0 there and -0 in the whole blocks, and a + b = (-0) + that differs in the sign bit.
__device__ __forceinline__ float mul_once_f16_add0(float k, float x) {
  const float m = mul_once_f16(k, x);
  return (k == 0.f || x == 0.f) && m == 0.f ? 0.f : m;  // (0 * inf is NaN and stays one)
}
__device__ __forceinline__ float rescaled_value_f16_tail(float p, float r, float phi, float psi) {
  float resc = mul_(p, r);
  asm("" : "+v"(resc));
  resc = rnd<f16_t>(resc);
  const float a = mul_once_f16_add0(phi, resc), b = mul_once_f16_add0(psi, p);
  float q = add_(a, b);
  asm("" : "+v"(q));
  return rnd<f16_t>(q);
}
__device__ __forceinline__ double rescaled_d(double p, double r, double phi, double psi) { return add_(mul_(phi, mul_(p, r)), mul_(psi, p)); }

// Kernarg of the one-trip kernel: GuidedArgs with the factor and the two blend scalars
template <int KMAX>
struct GuidedRescaledArgs {
  const void* in[KMAX];
  const void* cond;
  void* out;
  void* guided;         // nullptr: p' is not stored
  int32_t xmap_lr;      // log2(run length) of the XCD chunk map
  int32_t bps_shift;    // chunks per sample of the statistic (and of the draw): log2 when >= 0, minus the count otherwise (see sample_of)
  const uint64_t* seeds;
  const void* factor;   // T[samples]
  uint64_t stream0;
  float zeta0;
  float scale;          // g in the op-math type
  float phi, psi;       // guidance_rescale and 1 - guidance_rescale, each narrowed once
  int32_t slot;         // the operand that p' replaces in the sum
  float c0[KMAX];
};

template <typename T, int K, bool NOISE>
__global__ __launch_bounds__(BLOCK) void guided_rescaled_kernel_v1(const GuidedRescaledArgs<guided_kmax(K)> a) {
  constexpr bool TILE = sizeof(T) == 4;
  const uint32_t c = chunk_of(blockIdx.x, a.xmap_lr);
  const int64_t v = (int64_t)c * BLOCK + threadIdx.x;
  Raw<T> raw[K];
#pragma unroll
  for (int j = 0; j < K; ++j) raw[j] = load_raw<T, TILE>(a.in[j], v);
  Raw<T> rc = load_raw<T, TILE>(a.cond, v);
  __builtin_amdgcn_sched_barrier(0);  // every load is out before the first scalar of the arithmetic is fetched
  uint32_t smp, within;
  sample_of(c, a.bps_shift, smp, within);
  const float r = load_scalar<T>(a.factor, (int64_t)smp);  // (uniform: one sample per workgroup)
  float c0[K];
#pragma unroll
  for (int j = 0; j < K; ++j) c0[j] = a.c0[j];
  const float zeta0 = a.zeta0, g = a.scale, phi = a.phi, psi = a.psi;
  const int32_t slot = a.slot;
  float z[VEC];
  if constexpr (NOISE) {
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
    if (j == slot) {  // (uniform: a kernarg scalar against the unrolled operand's number) the rescaled guided value takes this operand's place
      float cf[VEC];
      widen<T, float>(rc, cf);
#pragma unroll
      for (int i = 0; i < VEC; ++i) w[i] = rescaled_value<T>(guided_value<T>(w[i], cf[i], g), r, phi, psi);
      if (a.guided != nullptr) store8<T, float, TILE>(a.guided, v, w);  // (p' is a value of T: the store's rounding is exact)
    }
    const float w0 = c0[j];
#pragma unroll
    for (int i = 0; i < VEC; ++i) s[i] = fma_(w0, w[i], s[i]);
  }
  if constexpr (NOISE) fma_noise8<float>(zeta0, z, s);
  store8<T, float, TILE>(a.out, v, s);
}

// ---- general kernel: per-element accesses, run-time dtypes -----------------------------------------------------------------
struct GuidedRescaledGenArgs {
  const void* in[SKR_ROW_TERMS];
  double c0[SKR_ROW_TERMS];
  const void* cond;
  void* out;      // nullptr: the guidance-only form
  void* guided;   // nullptr: p' is not stored
  const uint64_t* seeds;
  const void* factor;
  double zeta0, scale, phi, psi;
  uint64_t stream0;
  int64_t numel, sample_numel, stat_numel;  // the draw's sample and the statistic's (equal when the launch draws)
  int32_t n, n_a, dt_a, dt_b, dt_out, dt_g, slot, noise;
};

template <typename Acc>
__global__ __launch_bounds__(BLOCK) void guided_rescaled_kernel_gen(const GuidedRescaledGenArgs a) {
  constexpr bool F64 = std::is_same<Acc, double>::value;  // (an fp64 tensor takes part in fp64 arithmetic only)
  const int64_t tail_from = a.numel - a.numel % TORCH_TAIL;  // fp16: torch rounds a tensor-times-number product once from here on
  for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < a.numel; e += (int64_t)gridDim.x * BLOCK) {
    const int64_t stat_smp = e / a.stat_numel;
    // the rescaled guided value, in the op-math type of the slot's dtype whatever the accumulate type is; then widened exactly
    Acc p;
    bool wide_p = false;
    if constexpr (F64) wide_p = a.dt_g == SKR_F64;
    if (wide_p) {
      const double* up = reinterpret_cast<const double*>(a.in[a.slot]);
      const double* cp = reinterpret_cast<const double*>(a.cond);
      p = (Acc)rescaled_d(guide_d(up[e], cp[e], a.scale), reinterpret_cast<const double*>(a.factor)[stat_smp], a.phi, a.psi);
    } else {
      const float u = load_elem<float, false>(a.in[a.slot], e, a.dt_g), cv = load_elem<float, false>(a.cond, e, a.dt_g);
      const float r = load_elem<float, false>(a.factor, stat_smp, a.dt_g);
      const float g = (float)a.scale, phi = (float)a.phi, psi = (float)a.psi;
      float pf;
      if (a.dt_g == SKR_BF16) pf = rescaled_value<bf16_t>(guided_value<bf16_t>(u, cv, g), r, phi, psi);
      else if (a.dt_g == SKR_F16) pf = e >= tail_from ? rescaled_value_f16_tail(guided_value_f16_tail(u, cv, g), r, phi, psi) : rescaled_value<f16_t>(guided_value<f16_t>(u, cv, g), r, phi, psi);
      else pf = rescaled_value<float>(guided_value<float>(u, cv, g), r, phi, psi);
      p = (Acc)pf;
    }
    if (a.guided != nullptr) store_any<Acc>(a.guided, e, a.dt_g, p);  // (p' is a value of that dtype: exact)
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
static void launch_guided_rescaled_v1(const skr_step_plan& p, const void* const* inputs, void* out, const skr_step_guidance& gd, const skr_step_rescale& rs,
                                      const uint64_t* seeds, bool noise, int64_t chunks, hipStream_t s) {
  with_step_type<false>(p.dtype_a, [&](auto tt) {
    with_bools([&](auto nz) {
      with_count<1, SKR_ROW_TERMS>(p.n_terms, [&](auto n) {
        using T = typename decltype(tt)::type;
        constexpr int N = decltype(n)::value, KMAX = guided_kmax(N);
        GuidedRescaledArgs<KMAX> a;
        for (int k = 0; k < KMAX; ++k) { a.in[k] = k < N ? inputs[k] : nullptr; a.c0[k] = k < N ? (float)p.coef0[k] : 0.f; }
        a.cond = gd.cond; a.out = out; a.guided = gd.guided_out; a.seeds = seeds; a.factor = rs.factor_dev;
        a.xmap_lr = xmap_lr_for(chunks); a.bps_shift = bps_shift_of(rs.sample_numel / ((int64_t)BLOCK * VEC));
        a.stream0 = p.stream0; a.zeta0 = (float)p.zeta0; a.scale = (float)gd.scale; a.slot = gd.slot;
        a.phi = (float)rs.phi; a.psi = (float)(1.0 - rs.phi);
        hipLaunchKernelGGL((guided_rescaled_kernel_v1<T, N, decltype(nz)::value>), dim3((unsigned)chunks), dim3(BLOCK), 0, s, a);
      });
    }, noise);
  });
}

static int guided_rescaled_launch_impl(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide, const skr_step_rescale* rescale,
                                       const uint64_t* seeds_dev, int64_t numel, void* stream) {
  if (!plan || !guide || !rescale) return SKR_ERR_NULL;
  const skr_step_plan& p = *plan;
  const skr_step_guidance& gd = *guide;
  const skr_step_rescale& rs = *rescale;
  GuidedLaunch l;
  if (const int rc = guided_prepare(p, gd, inputs, out, seeds_dev, numel, false, &l, rescale)) return rc;
  if (numel == 0) return SKR_OK;
  const bool step_out = l.step_out, noise = l.noise;

  DeviceGuard device_guard(step_out ? out : gd.guided_out);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  constexpr int64_t CHUNK = (int64_t)BLOCK * VEC;
  if (l.one_trip && rs.sample_numel % CHUNK == 0 && rs.sample_numel < (1ll << 31)) {  // a workgroup inside one sample of the statistic
    launch_guided_rescaled_v1(p, inputs, out, gd, rs, seeds_dev, noise, l.chunks, s);
    return finish_launch();
  }

  GuidedRescaledGenArgs a;
  for (int k = 0; k < SKR_ROW_TERMS; ++k) {
    const bool live = k < p.n_terms;
    a.in[k] = live ? inputs[k] : nullptr;
    a.c0[k] = live ? p.coef0[k] : 0.0;
  }
  a.cond = gd.cond; a.out = step_out ? out : nullptr; a.guided = gd.guided_out; a.seeds = seeds_dev; a.factor = rs.factor_dev;
  a.zeta0 = p.zeta0; a.scale = gd.scale; a.phi = rs.phi; a.psi = 1.0 - rs.phi; a.stream0 = p.stream0;
  a.numel = numel; a.sample_numel = noise ? p.sample_numel : numel; a.stat_numel = rs.sample_numel;
  a.n = p.n_terms; a.n_a = p.n_group_a; a.dt_a = p.dtype_a; a.dt_b = l.dtype_b; a.dt_out = p.out0_dtype; a.dt_g = l.dtype_g; a.slot = gd.slot;
  a.noise = noise ? 1 : 0;
  const dim3 grid((unsigned)grid_blocks(numel, BLOCK, 256 * 64));
  with_bools([&](auto f64) { hipLaunchKernelGGL((guided_rescaled_kernel_gen<std::conditional_t<decltype(f64)::value, double, float>>), grid, dim3(BLOCK), 0, s, a); }, p.acc_f64 != 0);
  return finish_launch();
}

}  // namespace skr

extern "C" int skr_step_launch_guided_rescaled(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                               const skr_step_rescale* rescale, const uint64_t* seeds_dev, int64_t numel, void* stream) {
  return skr::guided_rescaled_launch_impl(plan, inputs, out, guide, rescale, seeds_dev, numel, stream);
}
