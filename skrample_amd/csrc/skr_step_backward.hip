// The two transposed step launches (include/skrample_hip.h): skr_step_backward_launch, the backward of skr_step_launch, and
// skr_step_masked_backward_launch, the backward of skr_step_launch_masked.  Each writes one gradient per operand that needs one in one
// pass over HBM.  No saved tensors: the forwards are linear in their operands, their coefficients are host numbers and the mask is data.
//
//   plain    grad_k = a_k * g0 + b_k * g1                        o = a*g0  (one gradient)  or  o = fma(b, g1, a*g0)
//   masked   grad_k = (c0[k]*m + c1[k]*(1 - m)) * g              t = 1 - m;  w = fma(a, m, b * t);  o = w * g    (a = c0[k], b = c1[k])
//
// in the accumulate type (fp32, fp64 if acc_f64), o rounded once to the gradient's dtype (store8 / store_any).  Where m == 1 a masked
// gradient is a*g as the plain launch computes it, and where m == 0 it is b*g; there is no gradient for the noise or the mask.
//   * one-trip kernels (step_bwd_k1, masked_bwd_k1): whole 2048-element chunks, every gradient, incoming gradient and the mask of one
//     16- or 32-bit dtype, fp32 arithmetic, <= 16 gradients (kernarg slots of 4 / 8 / 16).  Lane ownership, XCD chunk map, loads and
//     stores are those of step_kernel_k1 (skr_step_fast.hip), so a DPM-2 backward moves the same kind of traffic as a forward step: one
//     or two reads, K writes.  The masked kernel also needs samples made of whole chunks and mask_numel % 8 == 0; its mask indexing is
//     that of masked_kernel_v1 (skr_step_masked.hip), and both of its loads are issued before the first scalar of the arithmetic is fetched.
//   * general kernels (step_bwd_general, masked_bwd_general): grid-stride, one element per lane and trip, any size, any dtype
//     combination, fp32 or fp64 arithmetic; up to SKR_MAX_TERMS gradients (masked: SKR_ROW_TERMS).
// The two kernels of a launch evaluate the same operations on every element, so they agree bit for bit where both apply.
#include "skr_step_masked.h"
#include "skr_device.h"

namespace skr {

// ---- plain step ------------------------------------------------------------------------------------------------------------
template <int KMAX>
struct BwdOneTripArgs {
  void* grad[KMAX];
  const void* g0;
  const void* g1;
  int32_t xmap_lr;
  int32_t n;  // gradients written (<= KMAX)
  float a[KMAX];
  float b[KMAX];
};

template <typename T, int KMAX, bool HAS1>
__global__ __launch_bounds__(BLOCK) void step_bwd_k1(const BwdOneTripArgs<KMAX> p) {
  constexpr bool TILE = sizeof(T) == 4;  // whole chunks are whole tiles: 32-bit tensors take the whole-line layout, as in launch_k1
  const uint32_t c = chunk_of(blockIdx.x, p.xmap_lr);
  const int64_t v = (int64_t)c * BLOCK + threadIdx.x;
  Raw<T> r0 = load_raw<T, TILE>(p.g0, v), r1;
  if constexpr (HAS1) r1 = load_raw<T, TILE>(p.g1, v);
  float x0[VEC], x1[VEC];
  widen<T, float>(r0, x0);
  if constexpr (HAS1) widen<T, float>(r1, x1);
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    if (j < p.n) {  // (uniform: the count is a kernarg scalar)
      const float aj = p.a[j];
      float o[VEC];
      if constexpr (HAS1) {
        const float bj = p.b[j];
#pragma unroll
        for (int i = 0; i < VEC; ++i) o[i] = fma_(bj, x1[i], mul_(aj, x0[i]));
      } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) o[i] = mul_(aj, x0[i]);
      }
      store8<T, float, TILE>(p.grad[j], v, o);
    }
  }
}

struct BwdArgs {
  void* grad[MAXK];
  double a[MAXK];
  double b[MAXK];
  const void* g0;
  const void* g1;
  int64_t numel;
  int32_t n, n_a, dt_a, dt_b, dt_g0, dt_g1;
};

template <typename Acc, bool HAS1>
__global__ __launch_bounds__(BLOCK) void step_bwd_general(const BwdArgs p) {
  for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < p.numel; e += (int64_t)gridDim.x * BLOCK) {
    const Acc x0 = load_elem<Acc, true>(p.g0, e, p.dt_g0);
    Acc x1 = 0;
    if constexpr (HAS1) x1 = load_elem<Acc, true>(p.g1, e, p.dt_g1);
    for (int j = 0; j < p.n; ++j) {
      const Acc aj = (Acc)p.a[j];
      const Acc o = HAS1 ? fma_((Acc)p.b[j], x1, mul_(aj, x0)) : mul_(aj, x0);
      store_any<Acc>(p.grad[j], e, j < p.n_a ? p.dt_a : p.dt_b, o);
    }
  }
}

// ---- masked step -----------------------------------------------------------------------------------------------------------
// Kernarg of the one-trip masked kernel: what the first instructions need (the two source pointers, chunk map, mask layout) leads.
template <int KMAX>
struct MaskedBwdArgs {
  const void* g;
  const void* mask;
  int32_t xmap_lr;
  int32_t bps_shift;     // chunks per sample, as sample_of takes them
  uint32_t mask_numel;   // elements of one sample's mask (a multiple of 8, below 2^31)
  uint32_t mask_stride;  // elements between the masks of two samples: mask_numel or 0
  int32_t n;             // gradients written (<= KMAX)
  void* grad[KMAX];
  float a[KMAX];
  float b[KMAX];
};

template <typename T, int KMAX>
__global__ __launch_bounds__(BLOCK) void masked_bwd_k1(const MaskedBwdArgs<KMAX> p) {
  constexpr bool TILE = sizeof(T) == 4;  // whole chunks are whole tiles: 32-bit tensors take the whole-line layout, as in step_bwd_k1
  const uint32_t c = chunk_of(blockIdx.x, p.xmap_lr);
  const int64_t v = (int64_t)c * BLOCK + threadIdx.x;
  Raw<T> rg = load_raw<T, TILE>(p.g, v);
  // the lane-vector's mask elements, looked up as masked_kernel_v1 does: per group of 4 under the tile layout, never across a wrap
  uint32_t smp, within;
  sample_of(c, p.bps_shift, smp, within);
  const uint32_t vs = within * BLOCK + threadIdx.x;  // lane-vector within the sample (sample_numel < 2^31)
  const uint32_t m0 = (4u * (uint32_t)group0<TILE>((int64_t)vs)) % p.mask_numel;
  uint32_t m1 = m0 + 4u;
  if constexpr (TILE) m1 = (4u * (uint32_t)group1<TILE>((int64_t)vs)) % p.mask_numel;
  const int64_t mbase = (int64_t)smp * p.mask_stride;
  Raw<T> rm = load_mask8<T>(p.mask, mbase + m0, mbase + m1);
  __builtin_amdgcn_sched_barrier(0);  // both loads are out before the first scalar of the arithmetic is fetched
  float x[VEC], m[VEC], t[VEC];
  widen<T, float>(rg, x);
  widen<T, float>(rm, m);
#pragma unroll
  for (int i = 0; i < VEC; ++i) t[i] = sub_(1.f, m[i]);
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    if (j < p.n) {  // (uniform: the count is a kernarg scalar)
      const float aj = p.a[j], bj = p.b[j];
      float o[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) o[i] = mul_(fma_(aj, m[i], mul_(bj, t[i])), x[i]);
      store8<T, float, TILE>(p.grad[j], v, o);
    }
  }
}

// ---- general kernel: per-element accesses, run-time dtypes -----------------------------------------------------------------
struct MaskedBwdGenArgs {
  void* grad[SKR_ROW_TERMS];
  double a[SKR_ROW_TERMS];
  double b[SKR_ROW_TERMS];
  const void* g;
  const void* mask;
  int64_t numel, sample_numel, mask_numel, mask_stride;
  int32_t n, n_a, dt_a, dt_b, dt_g, dt_mask;
};

template <typename Acc>
__global__ __launch_bounds__(BLOCK) void masked_bwd_general(const MaskedBwdGenArgs p) {
  for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < p.numel; e += (int64_t)gridDim.x * BLOCK) {
    const int64_t smp = e / p.sample_numel, r = e - smp * p.sample_numel;
    const Acc x = load_elem<Acc, true>(p.g, e, p.dt_g);
    const Acc m = load_elem<Acc, true>(p.mask, smp * p.mask_stride + r % p.mask_numel, p.dt_mask);
    const Acc t = sub_((Acc)1, m);
    for (int j = 0; j < p.n; ++j) {
      const Acc w = fma_((Acc)p.a[j], m, mul_((Acc)p.b[j], t));
      store_any<Acc>(p.grad[j], e, j < p.n_a ? p.dt_a : p.dt_b, mul_(w, x));
    }
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// The plan's gradient pointers and coefficients into a kernarg's KMAX slots; the slots beyond n_grads hold nullptr / 0.
// Coef = float: the one-trip kernels.  Coef = double: the general kernels, whose fp32 arithmetic uses the coefficients rounded to
// fp32, as the one-trip kernels do.
template <typename Coef, int KMAX>
static void fill_grads(const skr_step_grad_plan& pl, void* const* grads, void* (&grad)[KMAX], Coef (&a)[KMAX], Coef (&b)[KMAX]) {
  for (int k = 0; k < KMAX; ++k) {
    const bool live = k < pl.n_grads;
    grad[k] = live ? grads[k] : nullptr;
    a[k] = live ? (pl.acc_f64 ? (Coef)pl.a[k] : (Coef)(float)pl.a[k]) : (Coef)0;
    b[k] = live ? (pl.acc_f64 ? (Coef)pl.b[k] : (Coef)(float)pl.b[k]) : (Coef)0;
  }
}

// f(type_tag<T>{}, std::integral_constant<int, KMAX>{}) for the element type and the kernarg slots (4, 8 or 16) of a one-trip launch
template <typename F>
static void with_bwd_k1(const skr_step_grad_plan& p, F&& f) {
  with_step_type<false>(p.dtype_a, [&](auto tt) {
    if (p.n_grads <= 4) f(tt, std::integral_constant<int, 4>{});
    else if (p.n_grads <= 8) f(tt, std::integral_constant<int, 8>{});
    else f(tt, std::integral_constant<int, 16>{});
  });
}

// What both one-trip kernels ask of a launch: fp32 arithmetic, every gradient and incoming gradient of the one 16- or 32-bit dtype
// dtype_a, at most 16 gradients, whole chunks.
static bool bwd_one_trip(const skr_step_grad_plan& p, int64_t numel) {
  constexpr int64_t CHUNK = (int64_t)BLOCK * VEC;
  const int32_t t = p.dtype_a;
  const bool one_dtype = (p.n_group_a == p.n_grads || p.dtype_b == t) && p.g0_dtype == t && (p.g1_dtype == SKR_NONE || p.g1_dtype == t);
  return g_tune.one_trip && !p.acc_f64 && one_dtype && t != SKR_F64 && p.n_grads <= 16 && numel % CHUNK == 0 && numel / CHUNK <= 0x7fffffffll;
}

}  // namespace skr

extern "C" int skr_step_backward_launch(const skr_step_grad_plan* plan, const void* g0, const void* g1, void* const* grads, int64_t numel,
                                        void* stream) {
  using namespace skr;
  if (!plan) return SKR_ERR_NULL;
  const skr_step_grad_plan& p = *plan;
  if (p.n_grads < 1 || p.n_grads > SKR_MAX_TERMS || p.n_group_a < 0 || p.n_group_a > p.n_grads) return SKR_ERR_TERMS;
  if (numel < 0) return SKR_ERR_SHAPE;
  if (!grads) return SKR_ERR_NULL;
  DeviceGuard device_guard(grads[0]);
  const bool has1 = p.g1_dtype != SKR_NONE;
  if (!tensor_dtype(p.g0_dtype) || (has1 && !tensor_dtype(p.g1_dtype)) || !tensor_dtype(p.dtype_a) || (p.n_group_a < p.n_grads && !tensor_dtype(p.dtype_b)))
    return SKR_ERR_DTYPE;
  if (numel == 0) return SKR_OK;
  if (!g0 || (has1 != (g1 != nullptr))) return SKR_ERR_NULL;
  if (!aligned16(g0) || (has1 && !aligned16(g1))) return SKR_ERR_ALIGN;
  if (const int rc = check_ptrs(grads, p.n_grads)) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (bwd_one_trip(p, numel)) {
    const int64_t chunks = numel / ((int64_t)BLOCK * VEC);
    with_bwd_k1(p, [&](auto tt, auto kmax) {
      BwdOneTripArgs<decltype(kmax)::value> a;
      fill_grads(p, grads, a.grad, a.a, a.b);
      a.g0 = g0; a.g1 = g1; a.n = p.n_grads; a.xmap_lr = xmap_lr_for(chunks);
      with_bools([&](auto h1) {
        hipLaunchKernelGGL((step_bwd_k1<typename decltype(tt)::type, decltype(kmax)::value, decltype(h1)::value>), dim3((unsigned)chunks), dim3(BLOCK), 0, s, a);
      }, has1);
    });
    return finish_launch();
  }
  BwdArgs a;
  fill_grads(p, grads, a.grad, a.a, a.b);
  a.g0 = g0; a.g1 = g1; a.numel = numel; a.n = p.n_grads; a.n_a = p.n_group_a;
  a.dt_a = p.dtype_a; a.dt_b = p.dtype_b; a.dt_g0 = p.g0_dtype; a.dt_g1 = p.g1_dtype;
  const dim3 grid((unsigned)grid_blocks(numel, BLOCK, 256 * 64));
  with_bools([&](auto f64, auto h1) {
    hipLaunchKernelGGL((step_bwd_general<std::conditional_t<decltype(f64)::value, double, float>, decltype(h1)::value>), grid, dim3(BLOCK), 0, s, a);
  }, p.acc_f64 != 0, has1);
  return finish_launch();
}

extern "C" int skr_step_masked_backward_launch(const skr_step_grad_plan* plan, const void* g, const skr_step_mask* mask, void* const* grads,
                                               int64_t numel, int64_t sample_numel, void* stream) {
  using namespace skr;
  if (!plan || !mask) return SKR_ERR_NULL;
  const skr_step_grad_plan& p = *plan;
  const skr_step_mask& mk = *mask;
  if (p.n_grads < 1 || p.n_grads > SKR_ROW_TERMS || p.n_group_a < 0 || p.n_group_a > p.n_grads) return SKR_ERR_TERMS;
  if (numel < 0) return SKR_ERR_SHAPE;
  if (!grads) return SKR_ERR_NULL;
  if (!tensor_dtype(p.g0_dtype) || !tensor_dtype(p.dtype_a) || (p.n_group_a < p.n_grads && !tensor_dtype(p.dtype_b)) || !tensor_dtype(mk.dtype))
    return SKR_ERR_DTYPE;
  if (p.g1_dtype != SKR_NONE || mk.reserved != 0 || (mk.dtype == SKR_F64 && !p.acc_f64)) return SKR_ERR_UNSUPPORTED;
  if (sample_numel <= 0 || numel % sample_numel != 0) return SKR_ERR_SHAPE;
  if (mk.mask_numel < 1 || sample_numel % mk.mask_numel != 0 || (mk.batch_stride != 0 && mk.batch_stride != mk.mask_numel)) return SKR_ERR_SHAPE;
  if (numel == 0) return SKR_OK;
  if (!g || !mk.mask) return SKR_ERR_NULL;
  if (!aligned16(g) || !aligned16(mk.mask)) return SKR_ERR_ALIGN;
  if (const int rc = check_ptrs(grads, p.n_grads)) return rc;
  DeviceGuard device_guard(grads[0]);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  constexpr int64_t CHUNK = (int64_t)BLOCK * VEC;
  // (the mask too of the one dtype, samples of whole chunks, no group of 4 mask elements across a wrap)
  if (bwd_one_trip(p, numel) && mk.dtype == p.dtype_a && sample_numel % CHUNK == 0 && sample_numel < (1ll << 31) && mk.mask_numel % 8 == 0) {
    const int64_t chunks = numel / CHUNK;
    with_bwd_k1(p, [&](auto tt, auto kmax) {
      MaskedBwdArgs<decltype(kmax)::value> a;
      fill_grads(p, grads, a.grad, a.a, a.b);
      a.g = g; a.mask = mk.mask; a.n = p.n_grads;
      a.xmap_lr = xmap_lr_for(chunks); a.bps_shift = bps_shift_of(sample_numel / CHUNK);
      a.mask_numel = (uint32_t)mk.mask_numel; a.mask_stride = (uint32_t)mk.batch_stride;
      hipLaunchKernelGGL((masked_bwd_k1<typename decltype(tt)::type, decltype(kmax)::value>), dim3((unsigned)chunks), dim3(BLOCK), 0, s, a);
    });
    return finish_launch();
  }
  MaskedBwdGenArgs a;
  fill_grads(p, grads, a.grad, a.a, a.b);
  a.g = g; a.mask = mk.mask; a.numel = numel; a.sample_numel = sample_numel; a.mask_numel = mk.mask_numel; a.mask_stride = mk.batch_stride;
  a.n = p.n_grads; a.n_a = p.n_group_a; a.dt_a = p.dtype_a; a.dt_b = p.dtype_b; a.dt_g = p.g0_dtype; a.dt_mask = mk.dtype;
  const dim3 grid((unsigned)grid_blocks(numel, BLOCK, 256 * 64));
  with_bools([&](auto f64) { hipLaunchKernelGGL((masked_bwd_general<std::conditional_t<decltype(f64)::value, double, float>>), grid, dim3(BLOCK), 0, s, a); }, p.acc_f64 != 0);
  return finish_launch();
}
