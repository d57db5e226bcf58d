// Host-side launch helpers shared by the launchers: run-time values to compile-time tags, the operand checks of the entry points, and the one
// way to launch a kernel whose dynamic LDS may exceed the default limit, how a launcher reads an environment switch, and the route decision of
// the Pyramid generator (host arithmetic only, so that a stand-alone program can check it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <type_traits>
#include "../../include/skrample_hip.h"

namespace skr {
template <typename T> struct type_tag { using type = T; };
template <bool B> using bool_c = std::integral_constant<bool, B>;

static inline int launch_status() { return hipGetLastError() == hipSuccess ? SKR_OK : SKR_ERR_LAUNCH; }

// environment switches of the launchers (measurement and test switches: production sets none).  A launcher that reads one once keeps it in a
// function-local static
static inline bool env_flag(const char* name) { return getenv(name) != nullptr; }
static inline int64_t env_int(const char* name, int64_t unset) { const char* e = getenv(name); return e ? (int64_t)atoll(e) : unset; }

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

// ---- routes of skr_noise_pyramid: which pass-1 form a (h, w) plane gets (the table is in DESIGN.md section 4.3) ---------------------------------
constexpr int PYR_MAX_LEVELS = 8;
constexpr int PYR_LDS_FLOATS = 38 * 1024;  // up to 152 KiB of level storage per block (dynamic LDS, 160 KiB per CU)
constexpr int PYR_UNROLLED = 5;  // levels 1..4 are unrolled (and cached per column strip); deeper levels are rare and tiny
constexpr int PYR_THREADS = 512;  // 8 waves per block (the strip kernel's 165 registers allow one such block per CU; 128 registers with spills were no faster)

// the five pass-1 forms: pyramid_pass1<false, 512>, <true, 256>, <true, 512>, <true, 1024> and <true, 1024, true>
enum class PyramidForm { Generic, Strip256, Strip512, Strip1024, Uni };
struct PyramidRoute {
  int status = SKR_ERR_UNSUPPORTED;  // the LDS level stage does not take the shape: the caller goes to skr_noise_pyramid_any
  PyramidForm form = PyramidForm::Generic;
  int threads = 0;
  size_t lds_bytes = 0;   // the level planes, and behind them the vertical tap table wherever the shape allows UNI
  int32_t ytab_off = -1;  // float offset of that table, -1 without
};
// h x w (w a multiple of 4, both at most 32767; h = 1 without resize_h).  The two tuning switches: no_uni (SKR_PYR_NO_UNI), and forced
// (SKR_PYR_MODE): 0 by shape, 1 generic, 2 strip/512, 3 strip/256, 4 strip/1024
static inline PyramidRoute choose_pyramid_route(int64_t h, int64_t w, bool resize_h, bool no_uni, int forced) {
  PyramidRoute r;
  // LDS stage for levels >= 1: every level is at most half the previous size per resized axis (r >= 2, and
  // level i >= 2 shrinks by r^i >= 4), so sum_{l>=1} h_l*w_l <= h*w/4 * (1 + 1/16 + ...) (1-D: w/2 * (1 + 1/4 + ...))
  const int64_t bound = resize_h ? (h / 2) * (w / 2) + (h / 8) * (w / 8) + (h / 32) * (w / 32) + 64 : w / 2 + w / 8 + w / 32 + 64;
  if (bound > PYR_LDS_FLOATS) return r;
  r.status = SKR_OK;
  r.lds_bytes = sizeof(float) * (size_t)bound;  // (the level geometry is worked out inside pass 1)
  const int64_t w4 = w / 4;  // a thread owns four columns
  auto strip = [&](int threads) { return threads % w4 == 0 && h / (threads / w4) >= 12; };  // strips pay off when a thread visits enough rows to amortise its tap table
  // rows a whole number of waves wide (w % 256 == 0) under 1024-lane strips: the vertical taps of the cached levels in a table behind the level planes
  const size_t ytab_bytes = sizeof(float2) * (size_t)(PYR_UNROLLED - 1) * (size_t)h;
  const bool uni = !no_uni && resize_h && w4 % 64 == 0 && strip(1024) && r.lds_bytes + ytab_bytes <= 156 * 1024;
  if (uni) {  // (the table is laid out whatever form SKR_PYR_MODE forces afterwards: a forced generic or 512-lane launch carries its bytes too)
    r.ytab_off = (int32_t)((bound + 1) & ~(int64_t)1);  // (8-byte entries)
    r.lds_bytes = sizeof(float) * (size_t)r.ytab_off + ytab_bytes;
  }
  // the strip kernel holds 165 registers, so a CU runs ONE 512-lane block (2 waves per SIMD) whatever the LDS would allow: where the
  // runs stay long enough, 1024 lanes (4 waves per SIMD at 128 registers, 19 of them spilled) hide more of the Philox / Box-Muller
  // dependency chains -- 72.9 against 75.9 us per draw at 64 x (4, 256, 256); small planes get long runs with 256-lane blocks
  const bool strip256 = r.lds_bytes <= 48 * 1024 && strip(256);
  const int mode = forced ? forced : (strip(1024) ? 4 : (strip(PYR_THREADS) ? 2 : (strip256 ? 3 : 1)));
  // A forced mode whose precondition fails, or that names no form, falls to the generic form.  (The enlarged byte count never decides
  // strip256, forced or not: uni asks for 12 rows per 1024-lane strip, h * w >= 49152, and the levels of such a plane alone pass 48 KiB.
  // The order -- the table's bytes first, strip256 after -- is kept as it was all the same.)
  if (mode == 4 && strip(1024)) r.form = uni ? PyramidForm::Uni : PyramidForm::Strip1024;
  else if (mode == 2 && strip(PYR_THREADS)) r.form = PyramidForm::Strip512;
  else if (mode == 3 && strip256) r.form = PyramidForm::Strip256;
  r.threads = r.form == PyramidForm::Strip256 ? 256 : (r.form == PyramidForm::Strip1024 || r.form == PyramidForm::Uni ? 1024 : PYR_THREADS);
  return r;
}
}  // namespace skr
