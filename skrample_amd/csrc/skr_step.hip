// Fused solver-step kernel for MI355X (gfx950): one coalesced HBM round trip per step.
//
//   out0 = sum_k c0[k]*in_k + zeta0*N(stream0)            (fp32 / fp64 registers)
//   out1 = chain*out0 + sum_k c1[k]*in_k + zeta1*N(stream1)
//
// Memory-bound by construction (<= ~1.5 flop/byte without noise): no LDS, no MFMA.  Each lane owns
// 8 consecutive elements per trip (16 B of bf16, 32 B of fp32), inputs are issued in batches of four
// independent 16-byte loads before any FMA so every wave keeps >= 4 KiB in flight, coefficients
// live in SGPRs (kernarg), 16-bit outputs and whole-line 32-bit outputs are written through (`sc0 sc1` stores:
// they are next read by the model, not by us).  The reference equivalent is ~16 separate aten passes + 17 copies per step
// (SURVEY.md section 8a, rows S2-S12).


#include "skr_device.h"
#include "skr_step_common.h"
#include <new>

namespace skr {

Tuning g_tune;

// ---- accumulate one dtype group: N terms x UV vectors of independent 16-byte loads, then FMAs --------
template <typename T, typename Acc, bool HAS1, int N, int UV, bool TILE>
__device__ __forceinline__ void acc_batch(const StepArgs<Acc>& a, int k, int64_t v0, int64_t vhi, Acc s0[UV][VEC], Acc s1[UV][VEC]) {
  Raw<T> raw[UV][N];
#pragma unroll
  for (int u = 0; u < UV; ++u) {
    const int64_t v = v0 + u * BLOCK;
    if (v < vhi) {
#pragma unroll
      for (int j = 0; j < N; ++j) raw[u][j] = load_raw<T, TILE>(a.in[k + j], v);
    }
  }
#pragma unroll
  for (int u = 0; u < UV; ++u) {
    if (v0 + u * BLOCK >= vhi) continue;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      Acc v[VEC];
      widen<T, Acc>(raw[u][j], v);
      const Acc w0 = a.c0[k + j];
#pragma unroll
      for (int i = 0; i < VEC; ++i) s0[u][i] = fma_(w0, v[i], s0[u][i]);
      if constexpr (HAS1) {
        const Acc w1 = a.c1[k + j];
#pragma unroll
        for (int i = 0; i < VEC; ++i) s1[u][i] = fma_(w1, v[i], s1[u][i]);
      }
    }
  }
}

template <typename T, typename Acc, bool HAS1, int UV, bool TILE>
__device__ __forceinline__ void acc_group(const StepArgs<Acc>& a, int k, int kend, int64_t v0, int64_t vhi, Acc s0[UV][VEC], Acc s1[UV][VEC]) {
  for (; k + 4 <= kend; k += 4) acc_batch<T, Acc, HAS1, 4, UV, TILE>(a, k, v0, vhi, s0, s1);
  if (k + 2 <= kend) { acc_batch<T, Acc, HAS1, 2, UV, TILE>(a, k, v0, vhi, s0, s1); k += 2; }
  if (k < kend) acc_batch<T, Acc, HAS1, 1, UV, TILE>(a, k, v0, vhi, s0, s1);
}

// generic placement: any sample_numel.  `smp`/`r` locate element e0 (first of the 8).
template <typename Acc>
__device__ __forceinline__ void locate(const StepArgs<Acc>& a, int64_t e0, int64_t& smp, int64_t& r) {
  smp = (int64_t)((double)e0 * a.inv_sample_numel);  // fp64 reciprocal, exact after one fix-up below 2^52
  r = e0 - smp * a.sample_numel;
  if (r < 0) { --smp; r += a.sample_numel; }
  else if (r >= a.sample_numel) { ++smp; r -= a.sample_numel; }
}

template <typename TA, typename TB, typename TO0, typename TO1, typename Acc, bool ST0, bool HAS1, bool NOISE, bool CONV, bool TILE>
__global__ __launch_bounds__(BLOCK) void step_kernel(const StepArgs<Acc> a) {
  constexpr int UV = uv_for(NOISE, HAS1);
  // Geometry.  mode 1 (per-sample grid): blockIdx.y/z pick the sample, so the seed is one scalar
  // load per block and no division is needed.  mode 0: flat grid over all vectors.
  int64_t vlo = 0, vhi = a.numel / VEC;
  uint64_t seed_u = 0;
  if constexpr (NOISE) {
    if (a.grid_mode == 1) {
      const int64_t smp = (int64_t)blockIdx.z * gridDim.y + blockIdx.y;
      vlo = smp * a.vps;
      vhi = vlo + a.vps;
      seed_u = a.seeds[smp];
    }
  }
  const int64_t stride = (int64_t)gridDim.x * (BLOCK * UV);
  for (int64_t v0 = vlo + (int64_t)blockIdx.x * (BLOCK * UV) + threadIdx.x; v0 < vhi; v0 += stride) {
    // flat-grid noise needs a per-lane seed: fetch it BEFORE the data loads so that waiting for it
    // (vmcnt counts in order) does not drain the whole load batch ahead of the Philox rounds.
    uint64_t seed_l[UV];
    int64_t r_l[UV];
    if constexpr (NOISE) {
      if (a.grid_mode == 0) {
#pragma unroll
        for (int u = 0; u < UV; ++u) {
          const int64_t v = v0 + u * BLOCK;
          seed_l[u] = 0; r_l[u] = 0;
          if (v < vhi) { int64_t smp; locate(a, v * VEC, smp, r_l[u]); seed_l[u] = a.seeds[smp]; }
        }
      }
    }
    Acc s0[UV][VEC], s1[UV][VEC];
#pragma unroll
    for (int u = 0; u < UV; ++u)
#pragma unroll
      for (int i = 0; i < VEC; ++i) { s0[u][i] = 0; s1[u][i] = 0; }

    // first load batch of group A is issued here; Philox (pure VALU) runs while it is in flight
    float z0[UV][VEC], z1[UV][VEC];
    if constexpr (NOISE) {
#pragma unroll
      for (int u = 0; u < UV; ++u) {
        const int64_t v = v0 + u * BLOCK;
        if (v >= vhi) continue;
        const uint64_t seed = a.grid_mode == 1 ? seed_u : seed_l[u];
        // Philox blocks of this slot's two 4-element groups (TILE launches always use the per-sample grid)
        const uint64_t blk = a.grid_mode == 1 ? (uint64_t)group0<TILE>(v - vlo) : (uint64_t)r_l[u] >> 2;
        const uint64_t blk_hi = a.grid_mode == 1 ? (uint64_t)group1<TILE>(v - vlo) : blk + 1;
        if (a.zeta0 != (Acc)0) { normal4(seed, a.stream0, blk, z0[u]); normal4(seed, a.stream0, blk_hi, z0[u] + 4); }
        if constexpr (HAS1) {
          if (a.zeta1 != (Acc)0) { normal4(seed, a.stream1, blk, z1[u]); normal4(seed, a.stream1, blk_hi, z1[u] + 4); }
        }
      }
    }

    acc_group<TA, Acc, HAS1, UV, TILE>(a, 0, a.n_a, v0, vhi, s0, s1);
    if constexpr (!std::is_same<TA, TB>::value) acc_group<TB, Acc, HAS1, UV, TILE>(a, a.n_a, a.n_terms, v0, vhi, s0, s1);
    if constexpr (CONV) {
      // out0 = rounded conversion of (in[0], in[1]); the host zeroes coef0 so s0 is still 0 here
      using M = typename OpMath<TA>::type;
      const M k[4] = {(M)a.ck[0], (M)a.ck[1], (M)a.ck[2], (M)a.ck[3]};
#pragma unroll
      for (int u = 0; u < UV; ++u) {
        const int64_t v = v0 + u * BLOCK;
        if (v >= vhi) continue;
        M sv[VEC], ov[VEC];
        widen<TA, M>(load_raw<TA, TILE>(a.in[0], v), sv);
        widen<TA, M>(load_raw<TA, TILE>(a.in[1], v), ov);
#pragma unroll
        for (int i = 0; i < VEC; ++i) s0[u][i] = (Acc)convert_rounded<TA, M>(sv[i], ov[i], a.conv_to, a.conv_from, k);
      }
    }

#pragma unroll
    for (int u = 0; u < UV; ++u) {
      const int64_t v = v0 + u * BLOCK;
      if (v >= vhi) continue;
      if constexpr (NOISE) { if (a.zeta0 != (Acc)0) fma_noise8<Acc>(a.zeta0, z0[u], s0[u]); }
      if constexpr (HAS1) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) s1[u][i] = fma_(a.chain, s0[u][i], s1[u][i]);
        if constexpr (NOISE) { if (a.zeta1 != (Acc)0) fma_noise8<Acc>(a.zeta1, z1[u], s1[u]); }
        store8<TO1, Acc, TILE>(a.out1, v, s1[u]);
      }
      if constexpr (ST0) store8<TO0, Acc, TILE>(a.out0, v, s0[u]);
    }
  }

  // ragged tail (< 8 elements at the very end of the tensor): one lane, scalar.  In-kernel noise
  // requires sample_numel % 8 == 0 (checked on the host), so a noisy launch never has a tail.
  const int64_t tail0 = (a.numel / VEC) * VEC;
  if (!NOISE && tail0 < a.numel && blockIdx.x == 0 && threadIdx.x == 0) {
    for (int i = 0; tail0 + i < a.numel; ++i) {
      const int64_t e = tail0 + i;
      Acc t0 = 0, t1 = 0;
      for (int k = 0; k < a.n_terms; ++k) {
        Acc v;
        if (k < a.n_a) v = std::is_same<Acc, double>::value ? (Acc)load_scalar_d<TA>(a.in[k], e) : (Acc)load_scalar<TA>(a.in[k], e);
        else v = std::is_same<Acc, double>::value ? (Acc)load_scalar_d<TB>(a.in[k], e) : (Acc)load_scalar<TB>(a.in[k], e);
        t0 = fma_(a.c0[k], v, t0);
        if constexpr (HAS1) t1 = fma_(a.c1[k], v, t1);
      }
      if constexpr (CONV) {
        using M = typename OpMath<TA>::type;
        const M k[4] = {(M)a.ck[0], (M)a.ck[1], (M)a.ck[2], (M)a.ck[3]};
        M sv, ov;
        if constexpr (std::is_same<M, double>::value) { sv = load_scalar_d<TA>(a.in[0], e); ov = load_scalar_d<TA>(a.in[1], e); }
        else { sv = load_scalar<TA>(a.in[0], e); ov = load_scalar<TA>(a.in[1], e); }
        t0 = (Acc)convert_rounded<TA, M>(sv, ov, a.conv_to, a.conv_from, k);
      }
      if constexpr (HAS1) {
        t1 = fma_(a.chain, t0, t1);
        store_scalar<TO1, Acc>(a.out1, e, t1);
      }
      if constexpr (ST0) store_scalar<TO0, Acc>(a.out0, e, t0);
    }
  }
}

// ---- host-side dispatch ------------------------------------------------------------------------------
thread_local int g_last_hip_error = 0;

// ---- compile-time-K fast path: uniform dtype, one output, no tail -------------------------------------
// The generic kernel walks a runtime term list (pointer/coefficient fetched from kernarg at a loop-dependent
// offset, loads in batches of 4).  For the common plans (<= 8 same-dtype operands, out dtype = in dtype) the
// term count is a template constant: every pointer and coefficient sits in SGPRs before the first load, all K
// loads are issued back to back, the Philox rounds run while they are in flight, then the FMAs.
struct FastArgs {  // compact kernarg (2-3 cache lines instead of the general 1.4 KB block)
  const void* in[8];
  float c0[8];
  void* out0;
  const uint64_t* seeds;
  float zeta0;
  uint64_t stream0;
  int64_t numel, vps;
};

template <typename T, int K, bool NOISE, int UV, bool TILE>
__global__ __launch_bounds__(BLOCK) void step_kernel_k(const FastArgs a) {
  int64_t vlo = 0, vhi = a.numel / VEC;
  uint64_t seed_u = 0;
  if constexpr (NOISE) {
    const int64_t smp = (int64_t)blockIdx.z * gridDim.y + blockIdx.y;
    vlo = smp * a.vps;
    vhi = vlo + a.vps;
    seed_u = a.seeds[smp];
  }
  const int64_t stride = (int64_t)gridDim.x * (BLOCK * UV);
  for (int64_t v0 = vlo + (int64_t)blockIdx.x * (BLOCK * UV) + threadIdx.x; v0 < vhi; v0 += stride) {
    Raw<T> raw[UV][K];
#pragma unroll
    for (int u = 0; u < UV; ++u) {
      if (v0 + u * BLOCK < vhi) {
#pragma unroll
        for (int j = 0; j < K; ++j) raw[u][j] = load_raw<T, TILE>(a.in[j], v0 + u * BLOCK);
      }
    }
    float z[UV][VEC];
    if constexpr (NOISE) {
#pragma unroll
      for (int u = 0; u < UV; ++u) {
        normal4(seed_u, a.stream0, (uint64_t)group0<TILE>(v0 + u * BLOCK - vlo), z[u]);
        normal4(seed_u, a.stream0, (uint64_t)group1<TILE>(v0 + u * BLOCK - vlo), z[u] + 4);
      }
    }
#pragma unroll
    for (int u = 0; u < UV; ++u) {
      const int64_t v = v0 + u * BLOCK;
      if (v >= vhi) continue;
      float s[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) s[i] = 0.f;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        float w[VEC];
        widen<T, float>(raw[u][j], w);
        const float c = a.c0[j];
#pragma unroll
        for (int i = 0; i < VEC; ++i) s[i] = fma_(c, w[i], s[i]);
      }
      if constexpr (NOISE) fma_noise8<float>(a.zeta0, z[u], s);
      store8<T, float, TILE>(a.out0, v, s);
    }
  }
}

// ---- compile-time-K Runge-Kutta stage: rounded pair conversion + chained second output ------------------
// out0 = convert_rounded(in[0], in[1])            (the stage's derivative, stored in T)
// out1 = chain*out0 + sum_k c1[k]*in[k]           (next stage input / step result, stored in T)
// Same arithmetic, in the same order, as step_kernel<..., CONV> -- but every operand is loaded exactly once
// (the generic kernel fetches the converted pair a second time), all K loads are issued back to back and the
// term list is a template constant.

template <typename T, int K, int UV, bool TILE>
__global__ __launch_bounds__(BLOCK) void step_kernel_rk(const RkArgs a) {
  const int64_t vhi = a.numel / VEC;
  const int64_t stride = (int64_t)gridDim.x * (BLOCK * UV);
  const float k[4] = {a.ck[0], a.ck[1], a.ck[2], a.ck[3]};
  for (int64_t v0 = (int64_t)blockIdx.x * (BLOCK * UV) + threadIdx.x; v0 < vhi; v0 += stride) {
    Raw<T> raw[UV][K];
#pragma unroll
    for (int u = 0; u < UV; ++u) {
      if (v0 + u * BLOCK < vhi) {
#pragma unroll
        for (int j = 0; j < K; ++j) raw[u][j] = load_raw<T, TILE>(a.in[j], v0 + u * BLOCK);
      }
    }
#pragma unroll
    for (int u = 0; u < UV; ++u) {
      const int64_t v = v0 + u * BLOCK;
      if (v >= vhi) continue;
      float sv[VEC], ov[VEC], d[VEC], s1[VEC];
      widen<T, float>(raw[u][0], sv);
      widen<T, float>(raw[u][1], ov);
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        d[i] = convert_rounded<T, float>(sv[i], ov[i], a.conv_to, a.conv_from, k);
        s1[i] = fma_(a.c1[1], ov[i], fma_(a.c1[0], sv[i], 0.f));
      }
#pragma unroll
      for (int j = 2; j < K; ++j) {
        float w[VEC];
        widen<T, float>(raw[u][j], w);
        const float c = a.c1[j];
#pragma unroll
        for (int i = 0; i < VEC; ++i) s1[i] = fma_(c, w[i], s1[i]);
      }
#pragma unroll
      for (int i = 0; i < VEC; ++i) s1[i] = fma_(a.chain, d[i], s1[i]);
      store8<T, float, TILE>(a.out1, v, s1);
      store8<T, float, TILE>(a.out0, v, d);
    }
  }
}


struct Geometry { dim3 grid; int mode; };

template <int UV, bool NOISE>
static Geometry geometry(int64_t numel, int64_t sample_numel) {
  const int64_t nvec = numel / VEC, per_block = BLOCK * UV;
  const bool aligned = (sample_numel % VEC) == 0;
  const int64_t vps = sample_numel / VEC, batch = numel / sample_numel;
  if (NOISE && aligned && vps >= per_block / 2 && batch <= 65535ll * 65535ll) {
    // per-sample grid: x covers one sample's vectors in ONE trip, (y,z) enumerate samples
    int64_t bx = (vps + per_block - 1) / per_block;
    if (bx > 65535) bx = 65535;  // grid-stride beyond (samples of > 134M elements)
    const int64_t gy = batch < 65535 ? batch : 65535;
    const int64_t gz = (batch + gy - 1) / gy;
    if (gy * gz == batch) return {dim3((unsigned)bx, (unsigned)gy, (unsigned)gz), 1};
  }
  int64_t blocks = grid_blocks(nvec, per_block, NOISE ? 256 * 32 : 256 * 4);  // grid-stride beyond: 4 blocks per CU (32 with Philox)
  if (blocks < 1) blocks = 1;  // (fewer than 8 elements: the block of the ragged tail)
  return {dim3((unsigned)blocks, 1, 1), 0};
}

// whole 512-element tiles everywhere (and, with in-kernel noise, samples made of whole tiles on the per-sample grid)
static bool tile_ok(int64_t numel, int64_t sample_numel, bool noise, int grid_mode) {
  return g_tune.tile && numel % 512 == 0 && (!noise || (grid_mode == 1 && sample_numel % 512 == 0));
}

// f(bool_c<TILE>{}): the whole-line tile layout when a 32-bit tensor takes part (WIDE) and the launch is made of whole tiles
template <bool WIDE, typename F>
static int with_tile(int64_t numel, int64_t sample_numel, bool noise, int grid_mode, F&& f) {
  if constexpr (WIDE) { if (tile_ok(numel, sample_numel, noise, grid_mode)) return f(bool_c<true>{}); }
  return f(bool_c<false>{});
}

int finish_launch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { g_last_hip_error = (int)e; return SKR_ERR_LAUNCH; }
  return SKR_OK;
}

template <typename T, bool NOISE, int UV>
static int launch_k_uv(StepArgs<float>& args, hipStream_t stream, bool& taken) {
  Geometry g = geometry<UV, NOISE>(args.numel, args.sample_numel);
  if (NOISE && g.mode != 1) return SKR_OK;  // flat-grid noise (tiny samples): generic kernel
  FastArgs fa;
  fill_operands(args.in, args.c0, args.n_terms, fa.in, fa.c0);
  fa.out0 = args.out0; fa.seeds = args.seeds; fa.zeta0 = args.zeta0; fa.stream0 = args.stream0;
  fa.numel = args.numel; fa.vps = args.sample_numel / VEC;
  taken = true;
  return with_tile<sizeof(T) == 4>(args.numel, args.sample_numel, NOISE, g.mode, [&](auto tile) {
    with_count<1, 8>(args.n_terms, [&](auto n) {
      hipLaunchKernelGGL((step_kernel_k<T, decltype(n)::value, NOISE, UV, decltype(tile)::value>), g.grid, dim3(BLOCK), 0, stream, fa);
    });
    return finish_launch();
  });
}

template <typename T, bool NOISE>
static int launch_k(StepArgs<float>& args, hipStream_t stream, bool& taken) {
  taken = false;
  if (args.n_terms < 1 || args.n_terms > 20 || args.numel % VEC != 0) return SKR_OK;
  {
    const int rc = launch_one_trip_k<T>(args, NOISE, stream, taken);  // whole chunks: one-trip kernel (skr_step_fast.hip), <= 20 operands
    if (taken) return rc;
  }
  if (has_table(args.form)) { taken = true; return SKR_ERR_UNSUPPORTED; }  // table launches: one-trip kernels only
  if (args.n_terms > 8) return SKR_OK;  // (the grid-stride compile-time kernels stop at 8: ragged launches of more operands take the general kernel)
  if constexpr (NOISE) {
    return launch_k_uv<T, true, 1>(args, stream, taken);
  } else {
    // 4 vectors per lane once that still leaves >= 4 blocks per CU (>= 8M elements), else 1 per lane
    if (args.numel / VEC >= 4ll * 256 * BLOCK * 4) return launch_k_uv<T, false, 4>(args, stream, taken);
    return launch_k_uv<T, false, 1>(args, stream, taken);
  }
}

template <typename T, int UV>
static int launch_rk_uv(const StepArgs<float>& args, hipStream_t stream) {
  Geometry g = geometry<UV, false>(args.numel, args.sample_numel);
  RkArgs ra;
  fill_operands(args.in, args.c1, args.n_terms, ra.in, ra.c1);
  ra.out0 = args.out0; ra.out1 = args.out1; ra.chain = args.chain;
  for (int i = 0; i < 4; ++i) ra.ck[i] = (float)args.ck[i];
  ra.conv_to = args.conv_to; ra.conv_from = args.conv_from; ra.numel = args.numel;
  return with_tile<sizeof(T) == 4>(args.numel, args.sample_numel, false, g.mode, [&](auto tile) {
    with_count<2, 8>(args.n_terms, [&](auto n) {
      hipLaunchKernelGGL((step_kernel_rk<T, decltype(n)::value, UV, decltype(tile)::value>), g.grid, dim3(BLOCK), 0, stream, ra);
    });
    return finish_launch();
  });
}

template <typename T>
static int launch_rk(const StepArgs<float>& args, hipStream_t stream) {
  {
    bool taken = false;
    const int rc = launch_one_trip_rk<T>(args, false, stream, taken);
    if (taken) return rc;
  }
  if (has_table(args.form)) return SKR_ERR_UNSUPPORTED;
  const int uv = g_tune.rk_uv ? g_tune.rk_uv : 1;  // measured on the cfg5 shard: 1, 2 and 4 vectors per lane are within 2 %
  if (uv == 4) return launch_rk_uv<T, 4>(args, stream);
  if (uv == 2) return launch_rk_uv<T, 2>(args, stream);
  return launch_rk_uv<T, 1>(args, stream);
}

template <typename TA, typename TB, typename TO0, typename TO1, typename Acc, bool ST0, bool HAS1, bool NOISE, bool CONV>
static int launch(StepArgs<Acc>& args, hipStream_t stream) {
  // fast path: uniform 16/32-bit dtype, single output of the same dtype, fp32 accumulate
  if constexpr (std::is_same<Acc, float>::value && std::is_same<TA, TB>::value && std::is_same<TO0, TA>::value && ST0 && !HAS1 && !CONV) {
    if (args.n_a == args.n_terms && (!NOISE || args.zeta0 != 0.f || has_table(args.form))) {
      bool taken = false;
      const int rc = launch_k<TA, NOISE>(args, stream, taken);
      if (taken) return rc;
    }
  }
  // Runge-Kutta stage fast path: uniform dtype in and out, conversion + chained result; with in-kernel noise (the last
  // stage of a stochastic step) only the one-trip kernel has a variant
  if constexpr (std::is_same<Acc, float>::value && std::is_same<TA, TB>::value && std::is_same<TO0, TA>::value && std::is_same<TO1, TA>::value && ST0 && HAS1 && CONV) {
    if (args.n_terms >= 2 && args.n_terms <= 8 && args.numel % VEC == 0) {
      if constexpr (!NOISE) return launch_rk<TA>(args, stream);
      else {
        bool taken = false;
        const int rc = launch_one_trip_rk<TA>(args, true, stream, taken);
        if (taken) return rc;
      }
    }
  }
  // two-output fast path (UniPC / SPC): 16-bit operands (+ at most one fp32 state), fp32 out0 + 16-bit out1
  if constexpr (std::is_same<Acc, float>::value && sizeof(TA) == 2 && (std::is_same<TB, TA>::value || std::is_same<TB, float>::value) &&
                std::is_same<TO0, float>::value && std::is_same<TO1, TA>::value && ST0 && HAS1 && !CONV) {
    bool taken = false;
    const int rc = launch_one_trip_two<TA>(args, NOISE, std::is_same<TB, float>::value, stream, taken);
    if (taken) return rc;
  }
  if (has_table(args.form)) return SKR_ERR_UNSUPPORTED;  // device-resident rows are read by the one-trip kernels only
  constexpr int UV = uv_for(NOISE, HAS1);
  Geometry g = geometry<UV, NOISE>(args.numel, args.sample_numel);
  args.grid_mode = g.mode;
  args.vps = args.sample_numel / VEC;
  constexpr bool HAS32 = std::is_same<Acc, float>::value && (std::is_same<TA, float>::value || std::is_same<TB, float>::value ||
                                                               (ST0 && std::is_same<TO0, float>::value) || (HAS1 && std::is_same<TO1, float>::value));
  return with_tile<HAS32>(args.numel, args.sample_numel, NOISE, g.mode, [&](auto tile) {
    hipLaunchKernelGGL((step_kernel<TA, TB, TO0, TO1, Acc, ST0, HAS1, NOISE, CONV, decltype(tile)::value>), g.grid, dim3(BLOCK), 0, stream, args);
    return finish_launch();
  });
}

// no kernel exists without an output, or with a conversion and no out1: asked at run time for the status and at compile time for the instantiations
constexpr bool no_kernel(bool st0, bool has1, bool conv) { return !has1 && (!st0 || conv); }

template <typename TA, typename TB, typename TO0, typename TO1, typename Acc>
static int pick_flags(StepArgs<Acc>& a, bool st0, bool has1, bool noise, bool conv, hipStream_t s) {
  if (no_kernel(st0, has1, conv)) return conv ? SKR_ERR_UNSUPPORTED : SKR_ERR_NULL;
  return with_bools([&](auto c_st0, auto c_has1, auto c_noise, auto c_conv) -> int {
    if constexpr (no_kernel(c_st0, c_has1, c_conv)) return SKR_ERR_UNSUPPORTED;  // (returned above)
    else return launch<TA, TB, TO0, TO1, Acc, c_st0, c_has1, c_noise, c_conv>(a, s);
  }, st0, has1, noise, conv);
}

// The one place that maps a plan's dtypes to the element types of a general kernel.  What the rule of
// skr_step_common.h admits becomes (TA, TB): group b's own type is that of fp32 operands beside 16-bit ones, and every fp64-arithmetic
// kernel reads group b as fp64 (16-bit latents under compute_scale=float64, skrample/diffusers.py:575-579, are widened exactly, summed in
// double and rounded once).  Each output is TA or the wide type Acc; one that is not stored counts as TA.
template <typename Acc>
static int pick(StepArgs<Acc>& a, const skr_step_plan& p, hipStream_t s) {
  constexpr bool F64 = std::is_same<Acc, double>::value;
  const bool noise = p.noise_mode == 1 && (has_table(a.form) || plan_draws(p));
  const int da = p.dtype_a, db = (p.n_group_a == p.n_terms) ? p.dtype_a : p.dtype_b;
  const bool conv = p.convert_to != 0 || p.convert_from != 0;
  const bool st0 = p.out0_dtype != SKR_NONE, has1 = p.out1_dtype != SKR_NONE;
  if (!step_inputs_ok(da, db, F64)) return SKR_ERR_DTYPE;
  if ((st0 && !step_output_ok(p.out0_dtype, da, F64)) || (has1 && !step_output_ok(p.out1_dtype, da, F64))) return SKR_ERR_DTYPE;
  return with_step_type<F64>(da, [&](auto ta) {
    using TA = typename decltype(ta)::type;
    return with_bools([&](auto b_wide, auto wide0, auto wide1) -> int {
      using TB = std::conditional_t<F64 || b_wide, Acc, TA>;
      using TO0 = std::conditional_t<wide0, Acc, TA>;
      using TO1 = std::conditional_t<wide1, Acc, TA>;
      return pick_flags<TA, TB, TO0, TO1, Acc>(a, st0, has1, noise, conv, s);
    }, !F64 && db != da, st0 && p.out0_dtype != da, has1 && p.out1_dtype != da);
  });
}

template <typename Acc>
static int run(const skr_step_plan& p, const void* const* inputs, void* out0, void* out1, const uint64_t* seeds, int64_t numel, hipStream_t s,
               RowForm form = RowForm::Kernarg, const skr_step_row* rows = nullptr, const int32_t* index = nullptr, int32_t row_offset = 0) {
  StepArgs<Acc> a;
  a.form = form; a.rows = rows; a.index = index; a.row_offset = row_offset;
  for (int k = 0; k < p.n_terms; ++k) {
    a.in[k] = inputs[k];
    a.c0[k] = (Acc)p.coef0[k];
    a.c1[k] = (Acc)p.coef1[k];
  }
  for (int k = p.n_terms; k < MAXK; ++k) { a.in[k] = nullptr; a.c0[k] = 0; a.c1[k] = 0; }
  a.out0 = out0; a.out1 = out1; a.seeds = seeds;
  a.chain = (Acc)p.chain; a.zeta0 = (Acc)p.zeta0; a.zeta1 = (Acc)p.zeta1;
  a.stream0 = p.stream0; a.stream1 = p.stream1;
  a.numel = numel;
  a.sample_numel = p.sample_numel > 0 ? p.sample_numel : (numel > 0 ? numel : 1);
  a.inv_sample_numel = 1.0 / (double)a.sample_numel;
  a.n_a = p.n_group_a; a.n_terms = p.n_terms;
  a.conv_to = p.convert_to; a.conv_from = p.convert_from;
  for (int i = 0; i < 4; ++i) a.ck[i] = p.convert_k[i];
  if (a.conv_to != 0 || a.conv_from != 0) {
    for (int k = 0; k < p.n_terms; ++k) a.c0[k] = 0;  // out0 is the conversion alone
  }
  return pick<Acc>(a, p, s);
}

}  // namespace skr

using skr::aligned16;

// a sample size that divides the launch into samples made of whole `multiple`s of elements
static int samples_ok(const skr_step_plan& p, int64_t numel, int64_t multiple) {
  if (p.sample_numel <= 0 || numel % p.sample_numel != 0) return SKR_ERR_SHAPE;
  return p.sample_numel % multiple == 0 ? SKR_OK : SKR_ERR_UNSUPPORTED;
}

// every check that depends on the plan and the element count alone (skr_program_create makes them once, a launch every time)
static int validate_plan(const skr_step_plan& p, int64_t numel) {
  if (p.n_terms < 0 || p.n_terms > SKR_MAX_TERMS || p.n_group_a < 0 || p.n_group_a > p.n_terms) return SKR_ERR_TERMS;
  if (numel < 0) return SKR_ERR_SHAPE;
  if (p.out0_dtype == SKR_NONE && p.out1_dtype == SKR_NONE) return SKR_ERR_NULL;
  if (p.noise_mode != 0 && p.noise_mode != 1) return SKR_ERR_UNSUPPORTED;
  if (p.convert_to < 0 || p.convert_to > 3 || p.convert_from < 0 || p.convert_from > 3) return SKR_ERR_UNSUPPORTED;
  if ((p.convert_to || p.convert_from) && (p.n_group_a < 2 || p.out1_dtype == SKR_NONE)) return SKR_ERR_TERMS;
  // fused Philox needs every 8-element lane group inside one sample; other shapes draw the noise
  // with skr_noise_random (any shape) and pass it as an ordinary input term.
  if (skr::plan_draws(p) && numel > 0) return samples_ok(p, numel, 8);
  return SKR_OK;
}

// the checks every step launch makes before anything form-specific, in their order; `empty`: numel == 0, SKR_OK and nothing to launch
int skr::step_launch_checks(const skr_step_plan* plan, const void* const* inputs, void* out0, void* out1, const uint64_t* seeds_dev, int64_t numel,
                            skr::RowForm form, const skr_step_row* rows, const int32_t* index, bool& empty) {
  empty = false;
  if (!plan || (has_table(form) && (!rows || (per_sample_rows(form) && !index)))) return SKR_ERR_NULL;  // (from here on: rows != nullptr exactly when has_table(form))
  const skr_step_plan& p = *plan;
  // (ahead of the plan's own checks: a launch that draws without seeds is told so whatever else is wrong with its sample size)
  if (p.noise_mode == 1 && (has_table(form) || skr::plan_draws(p)) && numel > 0 && !seeds_dev) return SKR_ERR_NULL;
  if (const int rc = validate_plan(p, numel)) return rc;
  if (numel == 0) { empty = true; return SKR_OK; }  // empty batch: nothing to do (the reference returns empty tensors)
  const bool st0 = p.out0_dtype != SKR_NONE, has1 = p.out1_dtype != SKR_NONE;
  if ((p.n_terms > 0 && !inputs) || (st0 && !out0) || (has1 && !out1)) return SKR_ERR_NULL;
  if (const int rc = skr::check_ptrs(inputs, p.n_terms)) return rc;
  if ((st0 && !aligned16(out0)) || (has1 && !aligned16(out1))) return SKR_ERR_ALIGN;
  return SKR_OK;
}

static int step_launch_impl(const skr_step_plan* plan, const void* const* inputs, void* out0, void* out1, const uint64_t* seeds_dev, int64_t numel,
                            void* stream, skr::RowForm form, const skr_step_row* rows, const int32_t* index, int32_t row_offset) {
  skr::DeviceGuard device_guard(out0 ? out0 : out1);
  bool empty = false;
  if (const int rc = skr::step_launch_checks(plan, inputs, out0, out1, seeds_dev, numel, form, rows, index, empty)) return rc;
  if (empty) return SKR_OK;
  const skr_step_plan& p = *plan;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (has_table(form)) {
    // one row per sample: the batch is numel / sample_numel, and a workgroup (2048 elements) must lie inside one sample
    // (or, for a single-output plan, ragged samples: at least one chunk each and a multiple of 8 elements -- skr_step_ragged.hip)
    const bool ragged = skr::ragged_launch(p, numel, form);
    if (per_sample_rows(form) || p.noise_mode == 1) {
      const int rc = samples_ok(p, numel, per_sample_rows(form) ? 2048 : 8);
      if (rc != SKR_OK && !(ragged && rc == SKR_ERR_UNSUPPORTED)) return rc;
    }
    if (p.acc_f64 || p.n_terms > SKR_ROW_TERMS || row_offset < 0) return SKR_ERR_UNSUPPORTED;
    if (ragged) return skr::launch_ragged(p, inputs, out0, seeds_dev, numel, s, form, rows, index, row_offset);
    return skr::run<float>(p, inputs, out0, out1, seeds_dev, numel, s, form, rows, index, row_offset);
  }
  return p.acc_f64 ? skr::run<double>(p, inputs, out0, out1, seeds_dev, numel, s)
                   : skr::run<float>(p, inputs, out0, out1, seeds_dev, numel, s);
}

extern "C" int skr_step_launch(const skr_step_plan* plan, const void* const* inputs, void* out0, void* out1,
                               const uint64_t* seeds_dev, int64_t numel, void* stream) {
  return step_launch_impl(plan, inputs, out0, out1, seeds_dev, numel, stream, skr::RowForm::Kernarg, nullptr, nullptr, 0);
}

extern "C" int skr_step_launch_indexed(const skr_step_plan* plan, const void* const* inputs, void* out0, void* out1,
                                       const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev,
                                       const int32_t* index_dev, int32_t row_offset, void* stream) {
  return step_launch_impl(plan, inputs, out0, out1, seeds_dev, numel, stream, skr::RowForm::WholeBatch, rows_dev, index_dev, row_offset);
}

extern "C" int skr_step_launch_indexed_per_sample(const skr_step_plan* plan, const void* const* inputs, void* out0, void* out1,
                                                  const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev,
                                                  const int32_t* sample_index_dev, int32_t row_offset, void* stream) {
  return step_launch_impl(plan, inputs, out0, out1, seeds_dev, numel, stream, skr::RowForm::PerSample, rows_dev, sample_index_dev, row_offset);
}

extern "C" int skr_step_launch_rolling(const skr_step_plan* plan, const void* const* inputs, void* out0, void* out1,
                                       const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev,
                                       const int32_t* sample_index_dev, int32_t row_offset, void* stream) {
  return step_launch_impl(plan, inputs, out0, out1, seeds_dev, numel, stream, skr::RowForm::Rolling, rows_dev, sample_index_dev, row_offset);
}

// ---- step programs: a plan kept by the library, launched by handle ------------------------------------------------------------------
// What is per launch stays per launch (operand / output / seed pointers, the two Philox stream ids); everything that depends on
// the plan alone -- term counts, dtype combination, conversion kinds, shape consistency -- is checked once, when the program is made.
struct skr_program {
  skr_step_plan plan;
  int64_t numel;
  skr_step_layout layout;  // channels == 0: none (skr_program_create)
};

extern "C" int skr_program_create(const skr_step_plan* plan, int64_t numel, skr_program** out) {
  if (!plan || !out) return SKR_ERR_NULL;
  *out = nullptr;
  if (const int rc = validate_plan(*plan, numel)) return rc;
  *out = new (std::nothrow) skr_program{*plan, numel, skr_step_layout{0, 0}};
  return *out ? SKR_OK : SKR_ERR_LAUNCH;
}

extern "C" int skr_program_create_channels_last(const skr_step_plan* plan, int64_t numel, const skr_step_layout* layout, skr_program** out) {
  if (!plan || !out) return SKR_ERR_NULL;
  *out = nullptr;
  if (const int rc = validate_plan(*plan, numel)) return rc;
  if (const int rc = skr::channels_last_checks(*plan, layout)) return rc;
  *out = new (std::nothrow) skr_program{*plan, numel, *layout};
  return *out ? SKR_OK : SKR_ERR_LAUNCH;
}

extern "C" int skr_program_launch(const skr_program* prog, const void* const* inputs, void* out0, void* out1, const uint64_t* seeds_dev,
                                  uint64_t stream0, uint64_t stream1, void* stream) {
  if (!prog) return SKR_ERR_NULL;
  skr_step_plan p = prog->plan;  // (a private copy: one program may be launched from several threads at once)
  p.stream0 = stream0;
  p.stream1 = stream1;
  if (prog->layout.channels != 0) return skr_step_launch_channels_last(&p, inputs, out0, out1, seeds_dev, &prog->layout, prog->numel, stream);
  return step_launch_impl(&p, inputs, out0, out1, seeds_dev, prog->numel, stream, skr::RowForm::Kernarg, nullptr, nullptr, 0);
}

extern "C" void skr_program_destroy(skr_program* prog) { delete prog; }

extern "C" int skr_last_hip_error(void) { return skr::g_last_hip_error; }

namespace skr { extern int g_fft_rank, g_use_hipfft; }  // skr_colored_any.hip: trailing axes given to the FFT (0 = up to three); hipFFT instead of skr_fft_own.hip

extern "C" int skr_set_tuning(const char* key, int32_t value) {
  if (!key) return SKR_ERR_NULL;
  if (!strcmp(key, "reset")) { skr::g_tune = skr::Tuning(); skr::g_fft_rank = 0; skr::g_use_hipfft = -1; }
  else if (!strcmp(key, "fft_rank")) skr::g_fft_rank = value;
  else if (!strcmp(key, "hipfft")) skr::g_use_hipfft = value;
  else if (!strcmp(key, "one_trip")) skr::g_tune.one_trip = value;
  else if (!strcmp(key, "xmap")) skr::g_tune.xmap = value;
  else if (!strcmp(key, "tile")) skr::g_tune.tile = value;
  else if (!strcmp(key, "rk_uv")) skr::g_tune.rk_uv = value;
  else if (!strcmp(key, "two_out")) skr::g_tune.two_out = value;
  else if (!strcmp(key, "pace")) skr::g_tune.pace = value;
  else if (!strcmp(key, "two_nt")) skr::g_tune.two_nt = value;
  else if (!strcmp(key, "tape_words")) skr::g_tune.tape_words = (value == 1 || value == 2) ? value : 0;
  else if (!strcmp(key, "rk_blk")) skr::g_tune.rk_blk = (value == 128 || value == 256) ? value : 0;
  else return SKR_ERR_UNSUPPORTED;
  return SKR_OK;
}
