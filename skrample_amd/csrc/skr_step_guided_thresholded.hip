// The guided thresholded solver step (include/skrample_hip.h, skr_guided_thresholded_step_launch): classifier-free guidance and dynamic
// thresholding fused into the step launch -- skr_thresholded_step_launch with the network output formed in registers from uncond and cond.
//
//   pg  = rn_T( u + rn_T( g * rn_T(c - u) ) )            u = inputs[slot], c = guide->cond; guided_value, torch's bits
//   x0  = rn32( rn32(a x) + rn32(b pg) )                 x = inputs[xslot]; x0_value
//   p   = rn_T( min(max(x0, -s), s) / s )                s = scale_dev[sample], what skr_guided_threshold_scale wrote (1 without one)
//   out = sum_k c0[k] * v_k + zeta0 * N(stream0)         v_slot = p, v_k = in_k otherwise: accumulated exactly as skr_step_launch does
//   x0_out = p                                           (when asked for)
// pg is never stored: out and x0_out have the bits skr_thresholded_step_launch writes over the tensor of the guidance-only launch.
//
//   * one-trip kernel (guided_thresholded_kernel_v1<T, K, NOISE>): whole 2048-element chunks, thr->sample_numel a multiple of 2048, one
//     16- or 32-bit dtype, 2..16 operands.  Lane ownership, XCD chunk map, Philox numbering, fp32 tile layout and stores are
//     thresholded_kernel_v1's.  A launch holds K + 1 operand images: the K operand loads and the cond load are issued in front of the
//     scheduling barrier, s is one scalar load through the constant address space behind them.  16-bit launches of more than 11 operands
//     keep 12 images in flight (11 operands and cond; the sample whatever its number, because the operand at `slot` needs it): operand
//     j + 11 is loaded where operand j has been summed, into the registers that frees (GT_AHEAD; profiles/guided_thresholded_isa.txt has
//     the register counts that decided it).  `slot` and `xslot` are kernarg scalars compared against the unrolled operand's number, so
//     the register arrays are never indexed at run time; whether out and x0_out are stored are uniform branches on the pointers, so the
//     thresholding-only form takes this kernel too.  Whole chunks are whole blocks of torch's kernel: no fp16 tail here.
//   * general kernel (guided_thresholded_kernel_gen): grid-stride, one element per lane and trip: ragged sizes, small samples, two dtype
//     groups; the fp16 tail rule by the element's index in the whole launch.
// Both evaluate the same operations in the same order on every element, so they agree bit for bit where both apply.
#include "skr_threshold.h"
#include "skr_step_guided_kernel.h"

namespace skr {

template <int KMAX>
struct GuidedThresholdedArgs {  // what the first instructions need leads, as in ThresholdedArgs
  const void* in[KMAX];
  const void* cond;
  void* out;            // nullptr: the thresholding-only form
  void* x0_out;         // nullptr: p is not stored
  int32_t xmap_lr;
  int32_t bps_shift;    // chunks per sample of the statistic (and of the draw)
  const uint64_t* seeds;
  const float* scale;   // nullptr: s = 1
  uint64_t stream0;
  float zeta0;
  float g;              // the guidance scale, narrowed once
  float a, b;
  int32_t slot, xslot;
  float c0[KMAX];
};

// operand images in flight beside cond: 16-bit launches of more than 11 operands stage the rest
template <typename T, int K>
constexpr int gt_ahead() { return (sizeof(T) == 2 && K > 11) ? 11 : K; }

template <typename T, int K, bool NOISE>
__global__ __launch_bounds__(BLOCK) void guided_thresholded_kernel_v1(const GuidedThresholdedArgs<guided_kmax(K)> a) {
  constexpr bool TILE = sizeof(T) == 4;
  constexpr int AHEAD = gt_ahead<T, K>();
  const uint32_t c = chunk_of(blockIdx.x, a.xmap_lr);
  const int64_t v = (int64_t)c * BLOCK + threadIdx.x;
  const int32_t slot = a.slot, xslot = a.xslot;
  Raw<T> raw[K];
#pragma unroll
  for (int j = 0; j < K; ++j) if (j < AHEAD || j == xslot) raw[j] = load_raw<T, TILE>(a.in[j], v);  // (uniform beyond AHEAD: the sample is needed at `slot`)
  const Raw<T> rc = load_raw<T, TILE>(a.cond, v);
  __builtin_amdgcn_sched_barrier(0);  // every load is out before the sample's scale is asked for
  uint32_t smp, within;
  sample_of(c, a.bps_shift, smp, within);
  smp = __builtin_amdgcn_readfirstlane(smp);
  const float s = a.scale != nullptr ? uniform(a.scale)[smp] : 1.f;  // (read-only for the launch: a scalar load)
  float z[VEC];
  if constexpr (NOISE) {
    const uint32_t vs = within * BLOCK + threadIdx.x;  // lane-vector within the sample (sample_numel < 2^31)
    const uint64_t seed = a.seeds[smp];
    normal4(seed, a.stream0, (uint64_t)group0<TILE>((int64_t)vs), z);
    normal4(seed, a.stream0, (uint64_t)group1<TILE>((int64_t)vs), z + 4);
  }
  float x[VEC];
#pragma unroll
  for (int j = 0; j < K; ++j) if (j == xslot) widen<T, float>(raw[j], x);  // (uniform: a kernarg scalar against the unrolled operand's number)
  float acc[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
  const bool step_out = a.out != nullptr;
  const float g = a.g;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    float w[VEC];
    widen<T, float>(raw[j], w);
    if (j == slot) {  // (uniform) uncond stands here: the guided value, then the thresholded prediction, takes its place
      float cf[VEC];
      widen<T, float>(rc, cf);
#pragma unroll
      for (int i = 0; i < VEC; ++i) w[i] = thresholded_value<T>(x0_value(a.a, x[i], a.b, guided_value<T>(w[i], cf[i], g)), s);
      if (a.x0_out != nullptr) store8<T, float, TILE>(a.x0_out, v, w);  // (p is a value of T: the store's rounding is exact)
    }
    if (step_out) {
      const float w0 = a.c0[j];
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = fma_(w0, w[i], acc[i]);
    }
    if constexpr (AHEAD < K) {  // operand j + AHEAD is loaded where operand j has been summed, into the registers that frees
      if (j + AHEAD < K) { if (j + AHEAD != xslot) raw[j + AHEAD] = load_raw<T, TILE>(a.in[j + AHEAD], v); }
    }
  }
  if (!step_out) return;
  if constexpr (NOISE) fma_noise8<float>(a.zeta0, z, acc);
  store8<T, float, TILE>(a.out, v, acc);
}

// ---- general kernel: per-element accesses, run-time dtypes, fp32 arithmetic -----------------------------------------------------------
struct GuidedThresholdedGenArgs {
  const void* in[SKR_ROW_TERMS];
  double c0[SKR_ROW_TERMS];
  const void* cond;
  void* out;      // nullptr: the thresholding-only form
  void* x0_out;   // nullptr: p is not stored
  const uint64_t* seeds;
  const float* scale;
  double zeta0;
  uint64_t stream0;
  int64_t numel, sample_numel, stat_numel;  // the draw's sample and the statistic's (equal when the launch draws)
  float g, a, b;
  int32_t n, n_a, dt_a, dt_b, dt_out, dt_g, dt_x, slot, xslot, noise;
};

__global__ __launch_bounds__(BLOCK) void guided_thresholded_kernel_gen(const GuidedThresholdedGenArgs a) {
  const int64_t tail_from = a.numel - a.numel % TORCH_TAIL;  // fp16: torch rounds g * d once from here on (mul_once_f16)
  for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < a.numel; e += (int64_t)gridDim.x * BLOCK) {
    const float s = a.scale != nullptr ? a.scale[e / a.stat_numel] : 1.f;
    const float x = load_elem<float, false>(a.in[a.xslot], e, a.dt_x);
    const float u = load_elem<float, false>(a.in[a.slot], e, a.dt_g), cv = load_elem<float, false>(a.cond, e, a.dt_g);
    float p;
    if (a.dt_g == SKR_BF16) p = thresholded_value<bf16_t>(x0_value(a.a, x, a.b, guided_value<bf16_t>(u, cv, a.g)), s);
    else if (a.dt_g == SKR_F16) p = thresholded_value<f16_t>(x0_value(a.a, x, a.b, e >= tail_from ? guided_value_f16_tail(u, cv, a.g) : guided_value<f16_t>(u, cv, a.g)), s);
    else p = thresholded_value<float>(x0_value(a.a, x, a.b, guided_value<float>(u, cv, a.g)), s);
    if (a.x0_out != nullptr) store_any<float>(a.x0_out, e, a.dt_g, p);  // (p is a value of that dtype: exact)
    if (a.out == nullptr) continue;
    float acc = 0.f;
    for (int j = 0; j < a.n; ++j) {
      float w = load_elem<float, false>(a.in[j], e, j < a.n_a ? a.dt_a : a.dt_b);
      if (j == a.slot) w = p;
      acc = fma_((float)a.c0[j], w, acc);
    }
    if (a.noise) {  // element r of the sample: Philox block r >> 2, lane r & 3 (sample_numel % 8 == 0, checked on the host)
      const int64_t smp = e / a.sample_numel, r = e - smp * a.sample_numel;
      float z[4];
      normal4(a.seeds[smp], a.stream0, (uint64_t)r >> 2, z);
      const int lane = (int)(r & 3);
      const float zz = lane == 0 ? z[0] : (lane == 1 ? z[1] : (lane == 2 ? z[2] : z[3]));
      acc = fma_((float)a.zeta0, zz, acc);
    }
    store_any<float>(a.out, e, a.dt_out, acc);
  }
}

}  // namespace skr

extern "C" int skr_guided_thresholded_step_launch(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                                  const skr_step_threshold* thr, const uint64_t* seeds_dev, int64_t numel, void* stream) {
  using namespace skr;
  if (!plan || !guide || !thr) return SKR_ERR_NULL;
  const skr_step_plan& p = *plan;
  const bool step_out = p.out0_dtype != SKR_NONE;
  const bool noise = step_out && p.noise_mode == 1 && p.zeta0 != 0.0;
  if (noise && numel > 0 && !seeds_dev) return SKR_ERR_NULL;
  if (p.n_terms < 0 || p.n_terms > SKR_ROW_TERMS || p.n_group_a < 0 || p.n_group_a > p.n_terms) return SKR_ERR_TERMS;
  if (thr->slot < 0 || thr->slot >= p.n_terms || thr->xslot < 0 || thr->xslot >= p.n_terms || thr->slot == thr->xslot) return SKR_ERR_TERMS;
  if (guide->slot != thr->slot) return SKR_ERR_TERMS;
  if (numel < 0) return SKR_ERR_SHAPE;
  if (!step_out && !thr->x0_out) return SKR_ERR_NULL;  // no output at all
  if (p.noise_mode != 0 && p.noise_mode != 1) return SKR_ERR_UNSUPPORTED;
  if (p.out1_dtype != SKR_NONE || p.chain != 0.0 || p.zeta1 != 0.0 || p.convert_to != 0 || p.convert_from != 0 || thr->reserved != 0 || guide->reserved != 0)
    return SKR_ERR_UNSUPPORTED;
  if (guide->guided_out != nullptr) return SKR_ERR_UNSUPPORTED;  // the guided prediction is never stored
  if (p.acc_f64 != 0) return SKR_ERR_UNSUPPORTED;
  if (!step_out && (out != nullptr || p.n_terms != 2)) return SKR_ERR_UNSUPPORTED;  // the thresholding-only form: the two operands, p alone
  if (noise && numel > 0) {  // fused Philox needs every 8-element group inside one sample, as in skr_step_launch
    if (p.sample_numel <= 0 || numel % p.sample_numel != 0) return SKR_ERR_SHAPE;
    if (p.sample_numel % 8 != 0) return SKR_ERR_UNSUPPORTED;
  }
  if (thr->sample_numel < 1 || numel % thr->sample_numel != 0) return SKR_ERR_SHAPE;
  if (noise && numel > 0 && p.sample_numel != thr->sample_numel) return SKR_ERR_SHAPE;
  if (numel == 0) return SKR_OK;
  if (!inputs || (step_out && !out) || !guide->cond) return SKR_ERR_NULL;
  if (const int rc = check_ptrs(inputs, p.n_terms)) return rc;
  if ((step_out && !aligned16(out)) || !aligned16(guide->cond) || !aligned16(thr->x0_out) || (reinterpret_cast<uintptr_t>(thr->scale_dev) & 3u) != 0)
    return SKR_ERR_ALIGN;
  const int32_t db = p.n_group_a == p.n_terms ? p.dtype_a : p.dtype_b;
  if (p.dtype_a == SKR_F64 || db == SKR_F64 || p.out0_dtype == SKR_F64) return SKR_ERR_UNSUPPORTED;
  if (!step_inputs_ok(p.dtype_a, db, false) || (step_out && !step_output_ok(p.out0_dtype, p.dtype_a, false))) return SKR_ERR_DTYPE;

  constexpr int64_t CHUNK = (int64_t)BLOCK * VEC;
  const int t = p.dtype_a;
  const bool one_dtype = db == t && (!step_out || p.out0_dtype == t);
  const bool one_trip = g_tune.one_trip && one_dtype && (t != SKR_F32 || g_tune.tile) && numel % CHUNK == 0 && numel / CHUNK <= 0x7fffffffll &&
                        thr->sample_numel % CHUNK == 0 && thr->sample_numel < (1ll << 31);
  DeviceGuard device_guard(step_out ? out : thr->x0_out);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (one_trip) {
    const int64_t chunks = numel / CHUNK;
    with_step_type<false>(t, [&](auto tt) {
      with_bools([&](auto nz) {
        with_count<2, SKR_ROW_TERMS>(p.n_terms, [&](auto n) {
          using T = typename decltype(tt)::type;
          constexpr int N = decltype(n)::value, KMAX = guided_kmax(N);
          GuidedThresholdedArgs<KMAX> a;
          for (int k = 0; k < KMAX; ++k) { a.in[k] = k < N ? inputs[k] : nullptr; a.c0[k] = k < N ? (float)p.coef0[k] : 0.f; }
          a.cond = guide->cond; a.out = step_out ? out : nullptr; a.x0_out = thr->x0_out; a.seeds = seeds_dev; a.scale = thr->scale_dev;
          a.xmap_lr = xmap_lr_for(chunks); a.bps_shift = bps_shift_of(thr->sample_numel / CHUNK);
          a.stream0 = p.stream0; a.zeta0 = (float)p.zeta0; a.g = (float)guide->scale; a.a = (float)thr->a; a.b = (float)thr->b;
          a.slot = thr->slot; a.xslot = thr->xslot;
          hipLaunchKernelGGL((guided_thresholded_kernel_v1<T, N, decltype(nz)::value>), dim3((unsigned)chunks), dim3(BLOCK), 0, s, a);
        });
      }, noise);
    });
  } else {
    GuidedThresholdedGenArgs a;
    for (int k = 0; k < SKR_ROW_TERMS; ++k) {
      const bool live = k < p.n_terms;
      a.in[k] = live ? inputs[k] : nullptr;
      a.c0[k] = live ? p.coef0[k] : 0.0;
    }
    a.cond = guide->cond; a.out = step_out ? out : nullptr; a.x0_out = thr->x0_out; a.seeds = seeds_dev; a.scale = thr->scale_dev;
    a.zeta0 = p.zeta0; a.stream0 = p.stream0;
    a.numel = numel; a.sample_numel = noise ? p.sample_numel : numel; a.stat_numel = thr->sample_numel;
    a.g = (float)guide->scale; a.a = (float)thr->a; a.b = (float)thr->b;
    a.n = p.n_terms; a.n_a = p.n_group_a; a.dt_a = p.dtype_a; a.dt_b = db; a.dt_out = p.out0_dtype;
    a.dt_g = thr->slot < p.n_group_a ? p.dtype_a : db; a.dt_x = thr->xslot < p.n_group_a ? p.dtype_a : db;
    a.slot = thr->slot; a.xslot = thr->xslot; a.noise = noise ? 1 : 0;
    hipLaunchKernelGGL(guided_thresholded_kernel_gen, dim3((unsigned)grid_blocks(numel, BLOCK, 256 * 64)), dim3(BLOCK), 0, s, a);
  }
  return finish_launch();
}
