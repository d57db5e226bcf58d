// Error norms for adaptive step control (reference skrample/sampling/functional.py:197-214: FunctionalAdaptive.mae /
// .mse = mean(|a - b|^p)).  Two-stage, fixed-order reduction in double: bit-reproducible, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skr_device.h"
#include "skr_launch.h"

namespace {

constexpr int RED_BLOCKS = 1024;

template <typename T> __device__ __forceinline__ double ld(const void* p, int64_t i) { return (double)reinterpret_cast<const T*>(p)[i]; }
template <> __device__ __forceinline__ double ld<__bf16>(const void* p, int64_t i) { return (double)(float)reinterpret_cast<const __bf16*>(p)[i]; }
template <> __device__ __forceinline__ double ld<_Float16>(const void* p, int64_t i) { return (double)(float)reinterpret_cast<const _Float16*>(p)[i]; }

template <typename T>
__global__ __launch_bounds__(256) void norm_partials(const void* a, const void* b, int64_t numel, int power, double* partials) {
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < numel; i += (int64_t)gridDim.x * 256) {
    const double d = fabs((a ? ld<T>(a, i) : 0.0) - ld<T>(b, i));
    s += power == 2 ? d * d : d;
  }
  __shared__ double red[4];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ void norm_final(const double* partials, int n, int64_t numel, double* out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += partials[i];
    out[0] = s / (double)numel;
  }
}

}  // namespace

extern "C" int skr_error_mean(const void* a_or_null, const void* b, int32_t dtype, int64_t numel, int32_t power,
                              double* out_dev, double* partials_dev /* [1024] */, void* stream) {
  skr::DeviceGuard device_guard(b);
  if (!b || !out_dev || !partials_dev) return SKR_ERR_NULL;
  if (numel <= 0) return SKR_ERR_SHAPE;
  if (power != 1 && power != 2) return SKR_ERR_UNSUPPORTED;
  const int64_t blocks = skr::grid_blocks(numel, 256, RED_BLOCKS);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rc = skr::with_out_type(dtype, [&](auto t) {
    hipLaunchKernelGGL(norm_partials<typename decltype(t)::type>, dim3((unsigned)blocks), dim3(256), 0, s, a_or_null, b, numel, power, partials_dev);
  });
  if (rc != SKR_OK) return rc;
  hipLaunchKernelGGL(norm_final, dim3(1), dim3(64), 0, s, partials_dev, (int)blocks, numel, out_dev);
  return skr::launch_status();
}

// ---- signed-power blend (SPC with power != 1; reference structured.py:568-572, common.py:187-190) --------------
// out = spowf(p * spowf(a, P) + c * spowf(b, P), 1/P),  spowf(x, f) = |x|^f * sign(x)   (sign(0) = +1 as in the reference)
// fp32 results: |x|^f on the raw log2/exp2 units (|x| = 0 gives 0 for f > 0); fp64 results (compute_scale = float64):
// double-precision pow.  Elementwise, any numel.
namespace skr {
template <typename T, typename M> __device__ __forceinline__ M blend_load(const void* p, int64_t i) {
  if constexpr (__is_same(T, __bf16)) return (M)__uint_as_float((uint32_t) reinterpret_cast<const uint16_t*>(p)[i] << 16);
  else return (M) reinterpret_cast<const T*>(p)[i];
}

__device__ __forceinline__ float spow_dev(float x, float f) {
  const float m = __builtin_amdgcn_exp2f(f * __builtin_amdgcn_logf(__builtin_fabsf(x)));
  return x < 0.f ? -m : m;
}
__device__ __forceinline__ double spow_dev(double x, double f) {
  const double m = pow(fabs(x), f);
  return x < 0.0 ? -m : m;
}

template <typename TA, typename TB, typename M>
__global__ __launch_bounds__(256) void power_blend_kernel(M* out, const void* a, const void* b, M p, M c, M power, M inv_power, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const M mix = spow_dev(blend_load<TA, M>(a, i), power) * p + spow_dev(blend_load<TB, M>(b, i), power) * c;
    out[i] = spow_dev(mix, inv_power);
  }
}

template <typename M>
static int power_blend_a(M* out, const void* a, int32_t a_dtype, const void* b, int32_t b_dtype, double p, double c, double power, int64_t n, hipStream_t s) {
  const dim3 grid((unsigned)grid_blocks(n, 256, 256 * 32));
  const M mp = (M)p, mc = (M)c, mw = (M)power, ip = (M)(1.0 / power);
  const int rc = with_out_type(a_dtype, [&](auto ta) {
    return with_out_type(b_dtype, [&](auto tb) {
      hipLaunchKernelGGL((power_blend_kernel<typename decltype(ta)::type, typename decltype(tb)::type, M>), grid, dim3(256), 0, s, out, a, b, mp, mc, mw, ip, n);
    });
  });
  return rc != SKR_OK ? rc : launch_status();
}
}  // namespace skr

extern "C" int skr_power_blend(void* out, int32_t out_dtype, const void* a, int32_t a_dtype, const void* b, int32_t b_dtype, double p, double c,
                               double power, int64_t numel, void* stream) {
  skr::DeviceGuard device_guard(out);
  if (numel < 0) return SKR_ERR_SHAPE;
  if (numel == 0) return SKR_OK;
  if (!out || !a || !b) return SKR_ERR_NULL;
  if (power == 0.0) return SKR_ERR_UNSUPPORTED;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (out_dtype == SKR_F32) return skr::power_blend_a<float>((float*)out, a, a_dtype, b, b_dtype, p, c, power, numel, s);
  if (out_dtype == SKR_F64) return skr::power_blend_a<double>((double*)out, a, a_dtype, b, b_dtype, p, c, power, numel, s);
  return SKR_ERR_DTYPE;
}

// ---- backward of the signed-power blend (include/skrample_hip.h, skr_power_blend_backward) ---------------------------------------
// torch autograd of the host expression spowf(x, f) = |x|^f * sign(x) gives, per spowf, d/dx = sgn(x) * f |x|^(f-1) * sgn(x) with
// sgn(0) = 0: the products below are that chain in that order, so exact zeros give what autograd gives (0, or 0 * inf = NaN where
// a zero meets a negative exponent).  |x|^f: pow in fp64; in fp32 the raw log2 / exp2 units, as the forward, with x^0 = 1.
namespace skr {
template <typename M> __device__ __forceinline__ M sgn_dev(M x) { return x > (M)0 ? (M)1 : (x < (M)0 ? (M)-1 : (M)0); }
__device__ __forceinline__ float apow_dev(float x, float f) {
  return f == 0.f ? 1.f : __builtin_amdgcn_exp2f(f * __builtin_amdgcn_logf(__builtin_fabsf(x)));
}
__device__ __forceinline__ double apow_dev(double x, double f) { return pow(fabs(x), f); }

// fp32 stepping stone of a 16-bit store, rounded to odd: where v is no fp32 value the last bit is set instead of rounding to nearest,
// so the RNE conversion that follows sees on which side of a 16-bit tie v lies and the store rounds v once (a nearest-rounded fp32
// in between moves a value from just beside a tie onto it: half a 16-bit ULP plus 2^-25 off).  Exact for fp32 arithmetic.
__device__ __forceinline__ float to_f32_odd(double v) {
  float f = (float)v;
  if ((double)f != v && v == v) {
    uint32_t u = __float_as_uint(f);
    if (fabs((double)f) > fabs(v)) u -= 1;  // towards zero (from inf: the largest finite value)
    f = __uint_as_float(u | 1u);
  }
  return f;
}

template <typename T> __device__ __forceinline__ void blend_store(void* p, int64_t i, double v) {
  if constexpr (__is_same(T, __bf16)) {
    float f = to_f32_odd(v);
    asm("" : "+v"(f));
    reinterpret_cast<__bf16*>(p)[i] = (__bf16)f;  // RNE
  } else if constexpr (__is_same(T, _Float16)) {
    float f = to_f32_odd(v);
    asm("" : "+v"(f));
    reinterpret_cast<_Float16*>(p)[i] = (_Float16)f;
  } else {
    reinterpret_cast<T*>(p)[i] = (T)v;
  }
}

template <typename TA, typename TB, typename M>
__global__ __launch_bounds__(256) void power_blend_bwd_kernel(void* ga, void* gb, const M* g, const void* a, const void* b, M p, M c, M power, M inv_power,
                                                              int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const M av = blend_load<TA, M>(a, i), bv = blend_load<TB, M>(b, i);
    const M u = spow_dev(av, power) * p + spow_dev(bv, power) * c;
    const M su = sgn_dev(u);
    const M gu = ((g[i] * su) * (inv_power * apow_dev(u, inv_power - (M)1))) * su;
    if (ga) {
      const M sa = sgn_dev(av);
      blend_store<TA>(ga, i, (double)((((gu * p) * sa) * (power * apow_dev(av, power - (M)1))) * sa));
    }
    if (gb) {
      const M sb = sgn_dev(bv);
      blend_store<TB>(gb, i, (double)((((gu * c) * sb) * (power * apow_dev(bv, power - (M)1))) * sb));
    }
  }
}

template <typename M>
static int power_blend_bwd_a(void* ga, void* gb, const M* g, const void* a, int32_t a_dtype, const void* b, int32_t b_dtype, double p, double c, double power,
                             int64_t n, hipStream_t s) {
  const dim3 grid((unsigned)grid_blocks(n, 256, 256 * 32));
  const M mp = (M)p, mc = (M)c, mw = (M)power, ip = (M)(1.0 / power);
  const int rc = with_out_type(a_dtype, [&](auto ta) {
    return with_out_type(b_dtype, [&](auto tb) {
      hipLaunchKernelGGL((power_blend_bwd_kernel<typename decltype(ta)::type, typename decltype(tb)::type, M>), grid, dim3(256), 0, s, ga, gb, g, a, b, mp, mc, mw, ip, n);
    });
  });
  return rc != SKR_OK ? rc : launch_status();
}
}  // namespace skr

extern "C" int skr_power_blend_backward(void* grad_a, void* grad_b, const void* g, int32_t g_dtype, const void* a, int32_t a_dtype, const void* b,
                                        int32_t b_dtype, double p, double c, double power, int64_t numel, void* stream) {
  skr::DeviceGuard device_guard(g);
  if (numel < 0) return SKR_ERR_SHAPE;
  if (numel == 0 || (!grad_a && !grad_b)) return SKR_OK;
  if (!g || !a || !b) return SKR_ERR_NULL;
  if (power == 0.0) return SKR_ERR_UNSUPPORTED;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (g_dtype == SKR_F32) return skr::power_blend_bwd_a<float>(grad_a, grad_b, (const float*)g, a, a_dtype, b, b_dtype, p, c, power, numel, s);
  if (g_dtype == SKR_F64) return skr::power_blend_bwd_a<double>(grad_a, grad_b, (const double*)g, a, a_dtype, b, b_dtype, p, c, power, numel, s);
  return SKR_ERR_DTYPE;
}
