// Host-side launch helpers shared by the launchers: run-time values to compile-time tags, and the one way to launch a kernel
// whose dynamic LDS may exceed the default limit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/skrample_hip.h"

namespace skr {
template <typename T> struct type_tag { using type = T; };

// Launches kernel<<<grid, block, lds_bytes, stream>>>(args...).  A kernel that needs more than the default 48 KiB of dynamic LDS
// must opt in first: SKR_ERR_UNSUPPORTED if the runtime refuses that, SKR_ERR_LAUNCH if the launch fails, else SKR_OK.
template <typename... Params, typename... Args>
static inline int launch_lds(void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, const Args&... args) {
  const void* fn = reinterpret_cast<const void*>(kernel);
  if (lds_bytes > 48 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess) return SKR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, static_cast<Params>(args)...);
  return hipGetLastError() == hipSuccess ? SKR_OK : SKR_ERR_LAUNCH;
}

// Returns f(type_tag<T>{}) for the element type T of an output dtype code: __bf16, _Float16, float and, where WITH_F64, double.
// SKR_ERR_DTYPE for every other code.
template <bool WITH_F64 = true, typename F>
static inline int with_out_type(int32_t out_dtype, F&& f) {
  if (out_dtype == SKR_BF16) return f(type_tag<__bf16>{});
  if (out_dtype == SKR_F16) return f(type_tag<_Float16>{});
  if (out_dtype == SKR_F32) return f(type_tag<float>{});
  if constexpr (WITH_F64) if (out_dtype == SKR_F64) return f(type_tag<double>{});
  return SKR_ERR_DTYPE;
}
}  // namespace skr
