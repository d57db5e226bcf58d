// The masked solver step (include/skrample_hip.h, skr_step_launch_masked): the in-painting blend fused into the step launch.
//
//   s = sum_k c0[k]*in_k + zeta0*N(stream0)      the solver step, accumulated exactly as skr_step_launch accumulates it
//   k = sum_k c1[k]*in_k                         the re-noised known region, over the operands whose c1 is not exactly zero
//   out = fma(m, s, (1 - m) * k)                 one pass over HBM, one store, one rounding (store8's)
//
//   * one-trip kernel (masked_kernel_v1): whole 2048-element chunks, samples made of whole chunks, operands / mask / output of one
//     16- or 32-bit dtype, fp32 arithmetic, <= 16 operands, mask_numel % 8 == 0.  Lane ownership, XCD chunk map, loads, stores and
//     Philox block numbering are those of step_kernel_k1's unpaced form (skr_step_fast.hip): every operand load is issued first, the
//     mask vector right behind them, the scalars and the Philox rounds while they are in flight.
//   * general kernel (masked_kernel_gen): grid-stride, one element per lane and trip, any size, any dtype combination skr_step_launch
//     takes, fp32 or fp64 arithmetic.
// Both evaluate the same operations in the same order on every element, so they agree bit for bit where both apply.
#include "skr_step_masked.h"
#include "skr_device.h"

namespace skr {

template <typename T, int K, bool NOISE>
__global__ __launch_bounds__(BLOCK) void masked_kernel_v1(const MaskedArgs<masked_kmax(K)> a) {
  constexpr bool TILE = sizeof(T) == 4;  // whole chunks are whole tiles: 32-bit tensors take the whole-line layout, as in launch_k1
  const uint32_t c = chunk_of(blockIdx.x, a.xmap_lr);
  const int64_t v = (int64_t)c * BLOCK + threadIdx.x;
  Raw<T> raw[K];
#pragma unroll
  for (int j = 0; j < K; ++j) raw[j] = load_raw<T, TILE>(a.in[j], v);
  // The mask index belongs to the lane-vector, not to the workgroup: a chunk may hold several wraps of the mask, or one in its middle.
  // With mask_numel % 8 == 0 a group of 4 consecutive elements never straddles a wrap, and the tile layout's two groups
  // (group0 / group1 of the lane-vector WITHIN the sample) are looked up separately.
  uint32_t smp, within;
  chunk_sample(c, a.bps_shift, smp, within);
  const uint32_t vs = within * BLOCK + threadIdx.x;  // lane-vector within the sample (sample_numel < 2^31)
  const uint32_t e0 = 4u * (uint32_t)group0<TILE>((int64_t)vs);
  const uint32_t m0 = e0 % a.mask_numel;
  uint32_t m1 = m0 + 4u;
  if constexpr (TILE) m1 = (4u * (uint32_t)group1<TILE>((int64_t)vs)) % a.mask_numel;
  const int64_t mbase = (int64_t)smp * a.mask_stride;
  Raw<T> rm = load_mask8<T>(a.mask, mbase + m0, mbase + m1);
  __builtin_amdgcn_sched_barrier(0);  // every load is out before the first scalar of the arithmetic is fetched
  float cf0[K], cf1[K];
#pragma unroll
  for (int j = 0; j < K; ++j) { cf0[j] = a.c0[j]; cf1[j] = a.c1[j]; }
  const float zeta0 = a.zeta0;
  float z[VEC];
  if constexpr (NOISE) {
    const uint64_t seed = a.seeds[smp];
    normal4(seed, a.stream0, (uint64_t)group0<TILE>((int64_t)vs), z);
    normal4(seed, a.stream0, (uint64_t)group1<TILE>((int64_t)vs), z + 4);
  }
  float s[VEC], kn[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) { s[i] = 0.f; kn[i] = 0.f; }
#pragma unroll
  for (int j = 0; j < K; ++j) {
    float w[VEC];
    widen<T, float>(raw[j], w);
    const float w0 = cf0[j], w1 = cf1[j];
#pragma unroll
    for (int i = 0; i < VEC; ++i) s[i] = fma_(w0, w[i], s[i]);
    if (w1 != 0.f) {  // (uniform: a kernarg scalar) an operand absent from the known form adds nothing to it, not even 0 * x
#pragma unroll
      for (int i = 0; i < VEC; ++i) kn[i] = fma_(w1, w[i], kn[i]);
    }
  }
  if constexpr (NOISE) fma_noise8<float>(zeta0, z, s);
  float m[VEC], o[VEC];
  widen<T, float>(rm, m);
#pragma unroll
  for (int i = 0; i < VEC; ++i) o[i] = fma_(m[i], s[i], mul_(sub_(1.f, m[i]), kn[i]));
  store8<T, float, TILE>(a.out, v, o);
}

// ---- general kernel: per-element accesses, run-time dtypes -----------------------------------------------------------------
struct MaskedGenArgs {
  const void* in[SKR_ROW_TERMS];
  double c0[SKR_ROW_TERMS];
  double c1[SKR_ROW_TERMS];
  const void* mask;
  void* out;
  const uint64_t* seeds;
  double zeta0;
  uint64_t stream0;
  int64_t numel, sample_numel, mask_numel, mask_stride;
  int32_t n, n_a, dt_a, dt_b, dt_out, dt_mask, noise;
};

// one rounding from Acc, the conversions of store8 (to a 16-bit dtype through the fp32 value, pinned in a register so that no fused
// multiply-add-and-convert rounds the exact sum instead).  The same function as store_any of skr_step_common.h (the backward kernels' store), kept apart: either
// body, used by both general kernels, changes the instructions of the other one.
template <typename Acc> __device__ __forceinline__ void store_elem(void* base, int64_t i, int dt, Acc v) {
  if (dt == SKR_BF16 || dt == SKR_F16) {
    float f = (float)v;
    asm("" : "+v"(f));
    if (dt == SKR_BF16) store_scalar<bf16_t, float>(base, i, f);
    else store_scalar<f16_t, float>(base, i, f);
  } else if (dt == SKR_F32) {
    store_scalar<float, Acc>(base, i, v);
  } else {
    store_scalar<double, Acc>(base, i, v);
  }
}

template <typename Acc>
__global__ __launch_bounds__(BLOCK) void masked_kernel_gen(const MaskedGenArgs a) {
  constexpr bool F64 = std::is_same<Acc, double>::value;  // (an fp64 tensor takes part in fp64 arithmetic only)
  for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < a.numel; e += (int64_t)gridDim.x * BLOCK) {
    const int64_t smp = e / a.sample_numel, r = e - smp * a.sample_numel;
    const Acc m = load_elem<Acc, F64>(a.mask, smp * a.mask_stride + r % a.mask_numel, a.dt_mask);
    Acc s = 0, kn = 0;
    for (int j = 0; j < a.n; ++j) {
      const Acc x = load_elem<Acc, F64>(a.in[j], e, j < a.n_a ? a.dt_a : a.dt_b);
      const Acc w0 = (Acc)a.c0[j], w1 = (Acc)a.c1[j];
      s = fma_(w0, x, s);
      if (w1 != (Acc)0) kn = fma_(w1, x, kn);
    }
    if (a.noise) {  // element r of the sample: Philox block r >> 2, lane r & 3 (sample_numel % 8 == 0, checked on the host)
      float z[4];
      normal4(a.seeds[smp], a.stream0, (uint64_t)r >> 2, z);
      const int lane = (int)(r & 3);
      const float zz = lane == 0 ? z[0] : (lane == 1 ? z[1] : (lane == 2 ? z[2] : z[3]));
      s = fma_((Acc)a.zeta0, (Acc)zz, s);
    }
    store_elem<Acc>(a.out, e, a.dt_out, fma_(m, s, mul_(sub_((Acc)1, m), kn)));
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
template <typename T, bool NOISE>
static void launch_masked_v1(const skr_step_plan& p, const void* const* inputs, void* out, const skr_step_mask& mk, const uint64_t* seeds,
                             int64_t chunks, int bps_shift, hipStream_t s) {
  with_count<1, SKR_ROW_TERMS>(p.n_terms, [&](auto n) {
    constexpr int N = decltype(n)::value;
    MaskedArgs<masked_kmax(N)> a;
    float c0[N], c1[N];
    for (int k = 0; k < N; ++k) { c0[k] = (float)p.coef0[k]; c1[k] = (float)p.coef1[k]; }
    fill_operands(inputs, c0, N, a.in, a.c0);
    fill_operands(inputs, c1, N, a.in, a.c1);
    a.mask = mk.mask; a.out = out; a.seeds = seeds;
    a.xmap_lr = xmap_lr_for(chunks); a.bps_shift = bps_shift;
    a.mask_numel = (uint32_t)mk.mask_numel; a.mask_stride = (uint32_t)mk.batch_stride;
    a.stream0 = p.stream0; a.zeta0 = (float)p.zeta0;
    hipLaunchKernelGGL((masked_kernel_v1<T, N, NOISE>), dim3((unsigned)chunks), dim3(BLOCK), 0, s, a);
  });
}

int masked_prepare(const skr_step_plan& p, const skr_step_mask& mk, const void* const* inputs, void* out, const uint64_t* seeds_dev, int64_t numel,
                   bool rows, MaskedLaunch* launch) {
  launch->noise = launch->one_trip = false;
  if (p.n_terms < 0 || p.n_group_a < 0 || p.n_group_a > p.n_terms || p.n_terms > SKR_ROW_TERMS) return SKR_ERR_TERMS;
  if (numel < 0) return SKR_ERR_SHAPE;
  if (p.out0_dtype == SKR_NONE) return SKR_ERR_NULL;
  if (p.out1_dtype != SKR_NONE || p.chain != 0.0 || p.zeta1 != 0.0 || p.convert_to != 0 || p.convert_from != 0 || mk.reserved != 0 ||
      (p.noise_mode != 0 && p.noise_mode != 1))
    return SKR_ERR_UNSUPPORTED;
  if (p.sample_numel <= 0 || numel % p.sample_numel != 0) return SKR_ERR_SHAPE;
  if (mk.mask_numel < 1 || p.sample_numel % mk.mask_numel != 0 || (mk.batch_stride != 0 && mk.batch_stride != mk.mask_numel)) return SKR_ERR_SHAPE;
  const bool noise = p.noise_mode == 1 && (rows || p.zeta0 != 0.0);
  if (noise && p.sample_numel % 8 != 0) return SKR_ERR_UNSUPPORTED;  // fused Philox needs every 8-element group inside one sample, as in skr_step_launch
  // the dtype combinations of skr_step_launch, with one output; the mask: a 16-bit dtype or the arithmetic's
  const int32_t db = p.n_group_a == p.n_terms ? p.dtype_a : p.dtype_b;
  if (!step_inputs_ok(p.dtype_a, db, p.acc_f64) || !step_output_ok(p.out0_dtype, p.dtype_a, p.acc_f64)) return SKR_ERR_DTYPE;
  if (mk.dtype != SKR_BF16 && mk.dtype != SKR_F16 && mk.dtype != SKR_F32 && !(mk.dtype == SKR_F64 && p.acc_f64)) return SKR_ERR_DTYPE;
  if (numel == 0) return SKR_OK;
  if ((p.n_terms > 0 && !inputs) || !out || !mk.mask || (noise && !seeds_dev)) return SKR_ERR_NULL;
  if (const int rc = check_ptrs(inputs, p.n_terms)) return rc;
  if (!aligned16(out) || !aligned16(mk.mask)) return SKR_ERR_ALIGN;
  launch->noise = noise;

  constexpr int64_t CHUNK = (int64_t)BLOCK * VEC;
  const int t = p.dtype_a;
  const bool one_dtype = (p.n_group_a == p.n_terms || p.dtype_b == t) && p.out0_dtype == t && mk.dtype == t && t != SKR_F64;
  if (g_tune.one_trip && !p.acc_f64 && one_dtype && p.n_terms >= 1 && (t != SKR_F32 || g_tune.tile) && numel % CHUNK == 0 &&
      numel / CHUNK <= 0x7fffffffll && p.sample_numel % CHUNK == 0 && p.sample_numel < (1ll << 31) && mk.mask_numel % 8 == 0) {
    const int64_t bps = p.sample_numel / CHUNK;
    int bps_shift = 0;
    if ((bps & (bps - 1)) == 0) { while ((1ll << bps_shift) < bps) ++bps_shift; }
    else bps_shift = -(int)bps;  // any chunk count per sample: the kernel divides
    launch->one_trip = true; launch->chunks = numel / CHUNK; launch->bps_shift = bps_shift;
  }
  return SKR_OK;
}

}  // namespace skr

extern "C" int skr_step_launch_masked(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_mask* mask,
                                      const uint64_t* seeds_dev, int64_t numel, void* stream) {
  using namespace skr;
  if (!plan || !mask) return SKR_ERR_NULL;
  const skr_step_plan& p = *plan;
  const skr_step_mask& mk = *mask;
  MaskedLaunch l;
  if (const int rc = masked_prepare(p, mk, inputs, out, seeds_dev, numel, false, &l)) return rc;
  if (numel == 0) return SKR_OK;
  const bool noise = l.noise;
  DeviceGuard device_guard(out);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);

  if (l.one_trip) {
    with_step_type<false>(p.dtype_a, [&](auto tt) {
      with_bools([&](auto nz) { launch_masked_v1<typename decltype(tt)::type, decltype(nz)::value>(p, inputs, out, mk, seeds_dev, l.chunks, l.bps_shift, s); }, noise);
    });
    return finish_launch();
  }

  MaskedGenArgs a;
  for (int k = 0; k < SKR_ROW_TERMS; ++k) {
    const bool live = k < p.n_terms;
    a.in[k] = live ? inputs[k] : nullptr;
    a.c0[k] = live ? p.coef0[k] : 0.0;
    a.c1[k] = live ? p.coef1[k] : 0.0;
  }
  a.mask = mk.mask; a.out = out; a.seeds = seeds_dev; a.zeta0 = p.zeta0; a.stream0 = p.stream0;
  a.numel = numel; a.sample_numel = p.sample_numel; a.mask_numel = mk.mask_numel; a.mask_stride = mk.batch_stride;
  a.n = p.n_terms; a.n_a = p.n_group_a; a.dt_a = p.dtype_a; a.dt_b = p.dtype_b; a.dt_out = p.out0_dtype; a.dt_mask = mk.dtype;
  a.noise = noise ? 1 : 0;
  const dim3 grid((unsigned)grid_blocks(numel, BLOCK, 256 * 64));
  with_bools([&](auto f64) { hipLaunchKernelGGL((masked_kernel_gen<std::conditional_t<decltype(f64)::value, double, float>>), grid, dim3(BLOCK), 0, s, a); }, p.acc_f64 != 0);
  return finish_launch();
}
