// The transposed solver step (include/skrample_hip.h, skr_step_backward_launch): grad_k = a_k * g0 + b_k * g1 for every operand
// that needs a gradient, in one pass over HBM.  No saved tensors: the forward is linear in its operands and its coefficients are
// host numbers.
//   * one-trip kernel: whole 2048-element chunks, every gradient and incoming gradient of one 16- or 32-bit dtype, fp32 arithmetic,
//     <= 16 gradients (kernarg slots of 4 / 8 / 16).  Lane ownership, XCD chunk map, loads and stores are those of step_kernel_k1
//     (skr_step_fast.hip), so a DPM-2 backward moves the same kind of traffic as a forward step: one or two reads, K writes.
//   * general kernel: grid-stride, any size, any dtype combination, up to SKR_MAX_TERMS gradients, fp32 or fp64 arithmetic.
// Both evaluate  o = a*g0  (one gradient)  or  o = fma(b, g1, a*g0)  and round o once, so they agree bit for bit where both apply.
#include "skr_step_common.h"
#include "skr_device.h"

namespace skr {

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

template <typename T, int KMAX, bool HAS1>
static void launch_bwd_k1(const skr_step_grad_plan& pl, const void* g0, const void* g1, void* const* grads, int64_t chunks, hipStream_t s) {
  BwdOneTripArgs<KMAX> p;
  for (int k = 0; k < KMAX; ++k) {
    const bool live = k < pl.n_grads;
    p.grad[k] = live ? grads[k] : nullptr;
    p.a[k] = live ? (float)pl.a[k] : 0.f;
    p.b[k] = live ? (float)pl.b[k] : 0.f;
  }
  p.g0 = g0; p.g1 = g1; p.n = pl.n_grads; p.xmap_lr = xmap_lr_for(chunks);
  hipLaunchKernelGGL((step_bwd_k1<T, KMAX, HAS1>), dim3((unsigned)chunks), dim3(BLOCK), 0, s, p);
}

// kernarg slots of the one-trip kernel: 4, 8 or 16
template <typename F>
static void with_bwd_slots(int n, F&& f) {
  if (n <= 4) f(std::integral_constant<int, 4>{});
  else if (n <= 8) f(std::integral_constant<int, 8>{});
  else f(std::integral_constant<int, 16>{});
}

static bool valid_dtype(int32_t d) { return d == SKR_BF16 || d == SKR_F16 || d == SKR_F32 || d == SKR_F64; }

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
  if (!valid_dtype(p.g0_dtype) || (has1 && !valid_dtype(p.g1_dtype)) || !valid_dtype(p.dtype_a) || (p.n_group_a < p.n_grads && !valid_dtype(p.dtype_b)))
    return SKR_ERR_DTYPE;
  if (numel == 0) return SKR_OK;
  if (!g0 || (has1 != (g1 != nullptr))) return SKR_ERR_NULL;
  if (!aligned16(g0) || (has1 && !aligned16(g1))) return SKR_ERR_ALIGN;
  if (const int rc = check_ptrs(grads, p.n_grads)) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  constexpr int64_t CHUNK = (int64_t)BLOCK * VEC;
  const int32_t t = p.dtype_a;
  const bool one_dtype = (p.n_group_a == p.n_grads || p.dtype_b == t) && p.g0_dtype == t && (!has1 || p.g1_dtype == t);
  if (g_tune.one_trip && !p.acc_f64 && one_dtype && t != SKR_F64 && p.n_grads <= 16 && numel % CHUNK == 0 && numel / CHUNK <= 0x7fffffffll) {
    const int64_t chunks = numel / CHUNK;
    with_step_type<false>(t, [&](auto tt) {
      with_bwd_slots(p.n_grads, [&](auto kmax) {
        with_bools([&](auto h1) { launch_bwd_k1<typename decltype(tt)::type, decltype(kmax)::value, decltype(h1)::value>(p, g0, g1, grads, chunks, s); }, has1);
      });
    });
    return finish_launch();
  }
  BwdArgs a;
  for (int k = 0; k < MAXK; ++k) {
    const bool live = k < p.n_grads;
    a.grad[k] = live ? grads[k] : nullptr;
    // fp32 arithmetic uses the coefficients rounded to fp32, as the one-trip kernel does
    a.a[k] = live ? (p.acc_f64 ? p.a[k] : (double)(float)p.a[k]) : 0.0;
    a.b[k] = live ? (p.acc_f64 ? p.b[k] : (double)(float)p.b[k]) : 0.0;
  }
  a.g0 = g0; a.g1 = g1; a.numel = numel; a.n = p.n_grads; a.n_a = p.n_group_a;
  a.dt_a = p.dtype_a; a.dt_b = p.dtype_b; a.dt_g0 = p.g0_dtype; a.dt_g1 = p.g1_dtype;
  const dim3 grid((unsigned)grid_blocks(numel, BLOCK, 256 * 64));
  with_bools([&](auto f64, auto h1) {
    hipLaunchKernelGGL((step_bwd_general<std::conditional_t<decltype(f64)::value, double, float>, decltype(h1)::value>), grid, dim3(BLOCK), 0, s, a);
  }, p.acc_f64 != 0, has1);
  return finish_launch();
}
