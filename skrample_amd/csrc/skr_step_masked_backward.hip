// The transposed masked step (include/skrample_hip.h, skr_step_masked_backward_launch): the backward of skr_step_launch_masked.
//
//   forward   out = m * (sum_k c0[k]*in_k + zeta0*N) + (1 - m) * (sum_k c1[k]*in_k)      linear in its operands; the mask is data
//   backward  grad_k = (c0[k]*m + c1[k]*(1 - m)) * g                                      no saved operand, no gradient for N or m
//
// Arithmetic, in the accumulate type (fp32, fp64 if acc_f64), with a = c0[k], b = c1[k]:
//
//   t = 1 - m;   w = fma(a, m, b * t);   grad = w * g          rounded once to the gradient's dtype (store8 / store_any)
//
// so where m == 1 a gradient is a*g as skr_step_backward_launch computes it, and where m == 0 it is b*g.  One pass over HBM: g and the
// mask read once, one gradient written per operand that wants one.
//   * one-trip kernel (masked_bwd_k1): whole 2048-element chunks, samples made of whole chunks, g / mask / every gradient of one 16- or
//     32-bit dtype, fp32 arithmetic, mask_numel % 8 == 0, kernarg slots of 4 / 8 / 16 gradients.  Lane ownership, XCD chunk map, tile
//     layout and stores are those of step_bwd_k1 (skr_step_backward.hip), the mask indexing that of masked_kernel_v1
//     (skr_step_masked.hip); both loads are issued before the first scalar of the arithmetic is fetched.
//   * general kernel (masked_bwd_general): grid-stride, one element per lane and trip, any size, any dtype combination, fp32 or fp64.
// Both evaluate the same operations on every element, so they agree bit for bit where both apply.
#include "skr_step_masked.h"
#include "skr_device.h"

namespace skr {

// Kernarg of the one-trip kernel: what the first instructions need (the two source pointers, chunk map, mask layout) leads.
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

template <typename T, int KMAX>
static void launch_masked_bwd_k1(const skr_step_grad_plan& pl, const void* g, const skr_step_mask& mk, void* const* grads, int64_t chunks,
                                 int bps_shift, hipStream_t s) {
  MaskedBwdArgs<KMAX> p;
  for (int k = 0; k < KMAX; ++k) {
    const bool live = k < pl.n_grads;
    p.grad[k] = live ? grads[k] : nullptr;
    p.a[k] = live ? (float)pl.a[k] : 0.f;
    p.b[k] = live ? (float)pl.b[k] : 0.f;
  }
  p.g = g; p.mask = mk.mask; p.n = pl.n_grads;
  p.xmap_lr = xmap_lr_for(chunks); p.bps_shift = bps_shift;
  p.mask_numel = (uint32_t)mk.mask_numel; p.mask_stride = (uint32_t)mk.batch_stride;
  hipLaunchKernelGGL((masked_bwd_k1<T, KMAX>), dim3((unsigned)chunks), dim3(BLOCK), 0, s, p);
}

// kernarg slots of the one-trip kernel: 4, 8 or 16 (those of step_bwd_k1)
template <typename F>
static void with_masked_bwd_slots(int n, F&& f) {
  if (n <= 4) f(std::integral_constant<int, 4>{});
  else if (n <= 8) f(std::integral_constant<int, 8>{});
  else f(std::integral_constant<int, 16>{});
}

static bool tensor_dtype(int32_t d) { return d == SKR_BF16 || d == SKR_F16 || d == SKR_F32 || d == SKR_F64; }

}  // namespace skr

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
  const int32_t t = p.dtype_a;
  const bool one_dtype = (p.n_group_a == p.n_grads || p.dtype_b == t) && p.g0_dtype == t && mk.dtype == t && t != SKR_F64;
  if (g_tune.one_trip && !p.acc_f64 && one_dtype && numel % CHUNK == 0 && numel / CHUNK <= 0x7fffffffll && sample_numel % CHUNK == 0 &&
      sample_numel < (1ll << 31) && mk.mask_numel % 8 == 0) {
    const int64_t chunks = numel / CHUNK;
    const int bps_shift = bps_shift_of(sample_numel / CHUNK);
    with_step_type<false>(t, [&](auto tt) {
      with_masked_bwd_slots(p.n_grads, [&](auto kmax) { launch_masked_bwd_k1<typename decltype(tt)::type, decltype(kmax)::value>(p, g, mk, grads, chunks, bps_shift, s); });
    });
    return finish_launch();
  }

  MaskedBwdGenArgs a;
  for (int k = 0; k < SKR_ROW_TERMS; ++k) {
    const bool live = k < p.n_grads;
    a.grad[k] = live ? grads[k] : nullptr;
    // fp32 arithmetic uses the coefficients rounded to fp32, as the one-trip kernel does
    a.a[k] = live ? (p.acc_f64 ? p.a[k] : (double)(float)p.a[k]) : 0.0;
    a.b[k] = live ? (p.acc_f64 ? p.b[k] : (double)(float)p.b[k]) : 0.0;
  }
  a.g = g; a.mask = mk.mask; a.numel = numel; a.sample_numel = sample_numel; a.mask_numel = mk.mask_numel; a.mask_stride = mk.batch_stride;
  a.n = p.n_grads; a.n_a = p.n_group_a; a.dt_a = p.dtype_a; a.dt_b = p.dtype_b; a.dt_g = p.g0_dtype; a.dt_mask = mk.dtype;
  const dim3 grid((unsigned)grid_blocks(numel, BLOCK, 256 * 64));
  with_bools([&](auto f64) { hipLaunchKernelGGL((masked_bwd_general<std::conditional_t<decltype(f64)::value, double, float>>), grid, dim3(BLOCK), 0, s, a); }, p.acc_f64 != 0);
  return finish_launch();
}
