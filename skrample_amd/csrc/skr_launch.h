// Host-side launch helpers shared by the launchers: run-time values to compile-time tags, the operand checks of the entry points, and the one
// way to launch a kernel whose dynamic LDS may exceed the default limit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/skrample_hip.h"

namespace skr {
template <typename T> struct type_tag { using type = T; };
template <bool B> using bool_c = std::integral_constant<bool, B>;

static inline int launch_status() { return hipGetLastError() == hipSuccess ? SKR_OK : SKR_ERR_LAUNCH; }

// Launches kernel<<<grid, block, lds_bytes, stream>>>(args...).  A kernel that needs more than the default 48 KiB of dynamic LDS
// must opt in first: SKR_ERR_UNSUPPORTED if the runtime refuses that, SKR_ERR_LAUNCH if the launch fails, else SKR_OK.
template <typename... Params, typename... Args>
static inline int launch_lds(void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, const Args&... args) {
  const void* fn = reinterpret_cast<const void*>(kernel);
  if (lds_bytes > 48 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess) return SKR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, static_cast<Params>(args)...);
  return launch_status();
}

// ---- dtype codes to element types: THE ladder ---------------------------------------------------------------
// Kernel symbols are named after their element types, and two families of them exist: the noise and reduce kernels take the compiler's
// own 16-bit types, the step kernels the two structs of skr_step_common.h (StepTypes).
struct NoiseTypes { using bf16 = __bf16; using f16 = _Float16; };

// Returns f(type_tag<T>{}) for the element type T of a dtype code in Family: its bf16, its f16, float and, where WITH_F64, double.
// SKR_ERR_DTYPE, and no call, for every other code.  An f that returns nothing counts as SKR_OK.
template <typename Family, bool WITH_F64 = true, typename F>
static inline int with_dtype(int32_t dtype, F&& f) {
  auto call = [&](auto t) -> int {
    if constexpr (std::is_void<decltype(f(t))>::value) { f(t); return SKR_OK; }
    else return f(t);
  };
  if (dtype == SKR_BF16) return call(type_tag<typename Family::bf16>{});
  if (dtype == SKR_F16) return call(type_tag<typename Family::f16>{});
  if (dtype == SKR_F32) return call(type_tag<float>{});
  if constexpr (WITH_F64) if (dtype == SKR_F64) return call(type_tag<double>{});
  return SKR_ERR_DTYPE;
}
template <bool WITH_F64 = true, typename F>
static inline int with_out_type(int32_t out_dtype, F&& f) { return with_dtype<NoiseTypes, WITH_F64>(out_dtype, f); }

// f(bool_c<B>{}...) for the run-time values b...: every combination is instantiated, so f rules the impossible ones out with `if constexpr`
template <typename F>
static inline auto with_bools(F&& f) { return f(); }
template <typename F, typename... Rest>
static inline auto with_bools(F&& f, bool b, Rest... rest) {
  return b ? with_bools([&](auto... t) { return f(bool_c<true>{}, t...); }, rest...)
           : with_bools([&](auto... t) { return f(bool_c<false>{}, t...); }, rest...);
}

// ---- what every entry point checks of its pointers, and the grid of a grid-stride launch --------------------------------------------
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the first fault among p[0 .. n), a pointer's absence ahead of its alignment: SKR_ERR_NULL, SKR_ERR_ALIGN (16 bytes), or SKR_OK
static inline int check_ptrs(const void* const* p, int n) {
  for (int k = 0; k < n; ++k) {
    if (!p[k]) return SKR_ERR_NULL;
    if (!aligned16(p[k])) return SKR_ERR_ALIGN;
  }
  return SKR_OK;
}

// workgroups of `per_block` items over n items, at most `cap` of them (the kernel strides over the rest)
static inline int64_t grid_blocks(int64_t n, int64_t per_block, int64_t cap) {
  const int64_t blocks = (n + per_block - 1) / per_block;
  return blocks > cap ? cap : blocks;
}
}  // namespace skr
