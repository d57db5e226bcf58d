// Guided in-painting (include/skrample_hip.h, skr_guided_masked_step_launch): classifier-free guidance, the solver step and the keep-region
// blend in one launch.  A guided step under a mask otherwise takes the guidance-only form of skr_step_launch_guided[_rescaled], which
// writes the prediction p to HBM, and then skr_step_launch_masked, which reads it straight back: for DPM-2 on bf16 latents 9 tensor
// passes plus the mask in two launches, against 8 here (sample, uncond, cond, one history prediction, original, noise in; prev_sample
// and p out).
//
//   p   = rn_T( u + rn_T( g * rn_T(c - u) ) )                u = inputs[slot], c = cond: torch's three tensor ops (guided_value, skr_step_guided.h)
//   p'  = rn_T( rn_T(phi * rn_T(p * r)) + rn_T(psi * p) )    rescale != NULL: r = factor_dev[sample] (rescaled_value); p' = p otherwise
//   s   = sum_k c0[k]*v_k + zeta0*N(stream0)                 v_slot = p', v_k = in_k otherwise: from zero, slot order, one fma each, noise last
//   kn  = sum_k c1[k]*in_k                                   over the operands whose c1 is not exactly zero (never the slot: refused on the host)
//   out = fma(m, s, (1 - m) * kn)                            one store, one rounding (store8's)
//   guided_out = p'                                          (when given)
//
// `out` has the bits skr_step_launch_masked writes with a tensor holding p' in `slot` -- p' is a value of T, so the store and the load
// between the two launches change nothing, and the accumulation here is that kernel's, operation for operation --, and guided_out the
// bits of the guidance-only launch.
//
// One kernel, guided_masked_kernel_v1<T, K, NOISE, RESCALE>, Kernarg form only: 3 dtypes x 16 operand counts x 2 x 2 = 192 instantiations.
// It covers exactly what a one-trip kernel can take -- whole 2048-element chunks, samples made of whole chunks, one 16- or 32-bit dtype
// for operands, cond, mask and both outputs, fp32 arithmetic, 1..16 operands, mask_numel % 8 == 0 -- and there is no grid-stride kernel
// and no row form behind it: everything else is SKR_ERR_UNSUPPORTED with nothing written.  numel is always whole chunks, so the fp16
// exception of the guided step (torch rounds g * d once in the partial last block of its kernel) cannot arise
// here: TORCH_TAIL is the chunk size, and a tensor of whole chunks has no tail.
//
// Lane ownership, XCD chunk map, loads, stores and Philox block numbering are those of masked_kernel_v1 (skr_step_masked.hip); the mask
// index belongs to the lane-vector within the sample, as there.  Every load of the workgroup -- K operands, cond, the mask vector -- is
// issued before the first scalar of the arithmetic is fetched; the kernarg scalars, the per-sample factor (one uniform load), the seed
// and the Philox rounds run while the loads are in flight.
#include "skr_step_guided.h"
#include "skr_step_masked.h"
#include "skr_device.h"

namespace skr {

constexpr int guided_masked_kmax(int k) { return k <= 4 ? 4 : (k <= 8 ? 8 : (k <= 12 ? 12 : 16)); }

// Kernarg: what the first instructions need (operand pointers, cond, mask, chunk map, the mask's geometry) leads, as in MaskedArgs; the
// scalars of the arithmetic follow, the two coefficient arrays last.  One layout for both RESCALE values: an unrescaled launch leaves
// factor NULL and phi / psi zero, and never reads them.
template <int KMAX>
struct GuidedMaskedArgs {
  const void* in[KMAX];
  const void* cond;
  const void* mask;
  void* out;
  void* guided;         // nullptr: p' is not stored
  int32_t xmap_lr;      // log2(run length) of the XCD chunk map
  int32_t bps_shift;    // chunks per sample: log2 when >= 0, minus the count otherwise (see sample_of)
  uint32_t mask_numel;  // elements of one sample's mask (a multiple of 8, below 2^31)
  uint32_t mask_stride; // elements between the masks of two samples: mask_numel or 0
  const uint64_t* seeds;
  const void* factor;   // T[samples] (RESCALE)
  uint64_t stream0;
  float zeta0;
  float scale;          // g in the op-math type
  float phi, psi;       // guidance_rescale and 1 - guidance_rescale, each narrowed once (RESCALE)
  int32_t slot;         // the operand that p' replaces in the step form
  float c0[KMAX];
  float c1[KMAX];
};

template <typename T, int K, bool NOISE, bool RESCALE>
__global__ __launch_bounds__(BLOCK) void guided_masked_kernel_v1(const GuidedMaskedArgs<guided_masked_kmax(K)> a) {
  constexpr bool TILE = sizeof(T) == 4;  // whole chunks are whole tiles: 32-bit tensors take the whole-line layout, as in launch_k1
  const uint32_t c = chunk_of(blockIdx.x, a.xmap_lr);
  const int64_t v = (int64_t)c * BLOCK + threadIdx.x;
  // 1. every load: the K operands and cond non-temporal (read once), the mask vector plain (every channel of the sample re-reads it)
  Raw<T> raw[K];
#pragma unroll
  for (int j = 0; j < K; ++j) raw[j] = load_raw<T, TILE>(a.in[j], v);
  const Raw<T> rc = load_raw<T, TILE>(a.cond, v);
  uint32_t smp, within;
  sample_of(c, a.bps_shift, smp, within);
  const uint32_t vs = within * BLOCK + threadIdx.x;  // lane-vector within the sample (sample_numel < 2^31)
  // The mask index belongs to the lane-vector, not to the workgroup: a chunk may hold several wraps of the mask, or one in its middle.
  // With mask_numel % 8 == 0 a group of 4 consecutive elements never straddles a wrap, and the tile layout's two groups are looked
  // up separately.
  const uint32_t e0 = 4u * (uint32_t)group0<TILE>((int64_t)vs);
  const uint32_t m0 = e0 % a.mask_numel;
  uint32_t m1 = m0 + 4u;
  if constexpr (TILE) m1 = (4u * (uint32_t)group1<TILE>((int64_t)vs)) % a.mask_numel;
  const int64_t mbase = (int64_t)smp * a.mask_stride;
  const Raw<T> rm = load_mask8<T>(a.mask, mbase + m0, mbase + m1);
  // 2. nothing below moves above this line
  __builtin_amdgcn_sched_barrier(0);
  // 3. the scalars of the arithmetic, the factor, the seed and the Philox rounds, all while the loads are in flight
  float c0[K], c1[K];
#pragma unroll
  for (int j = 0; j < K; ++j) { c0[j] = a.c0[j]; c1[j] = a.c1[j]; }
  const float zeta0 = a.zeta0, g = a.scale;
  const int32_t slot = a.slot;
  [[maybe_unused]] float r = 0.f, phi = 0.f, psi = 0.f;
  if constexpr (RESCALE) {
    r = load_scalar<T>(a.factor, (int64_t)smp);  // (uniform: one sample per workgroup)
    phi = a.phi; psi = a.psi;
  }
  float z[VEC];
  if constexpr (NOISE) {  // (the host chose the instantiation by the plan's zeta0: the draw is unconditional)
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
    if (j == slot) {  // (uniform: a kernarg scalar against the unrolled operand's number) the guided value takes this operand's place
      float cf[VEC];
      widen<T, float>(rc, cf);
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        w[i] = guided_value<T>(w[i], cf[i], g);
        if constexpr (RESCALE) w[i] = rescaled_value<T>(w[i], r, phi, psi);
      }
      if (a.guided != nullptr) store8<T, float, TILE>(a.guided, v, w);  // (p' is a value of T: the store's rounding is exact)
    }
    const float w0 = c0[j], w1 = c1[j];
#pragma unroll
    for (int i = 0; i < VEC; ++i) s[i] = fma_(w0, w[i], s[i]);
    if (w1 != 0.f) {  // (uniform: a kernarg scalar) an operand absent from the known form adds nothing to it, not even 0 * x; never the slot
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

// ---- host side ---------------------------------------------------------------------------------------------------------------
// dtype x noise x rescale x operand count to the instantiation, and its kernarg
static void launch_guided_masked_v1(const skr_step_plan& p, const void* const* inputs, void* out, const skr_step_guidance& gd, const skr_step_rescale* rs,
                                    const skr_step_mask& mk, const uint64_t* seeds, const MaskedLaunch& l, hipStream_t s) {
  with_step_type<false>(p.dtype_a, [&](auto tt) {
    with_bools([&](auto nz, auto re) {
      with_count<1, SKR_ROW_TERMS>(p.n_terms, [&](auto n) {
        using T = typename decltype(tt)::type;
        constexpr int N = decltype(n)::value, KMAX = guided_masked_kmax(N);
        constexpr bool RESCALE = decltype(re)::value;
        GuidedMaskedArgs<KMAX> a;
        for (int k = 0; k < KMAX; ++k) {
          a.in[k] = k < N ? inputs[k] : nullptr;
          a.c0[k] = k < N ? (float)p.coef0[k] : 0.f;
          a.c1[k] = k < N ? (float)p.coef1[k] : 0.f;
        }
        a.cond = gd.cond; a.mask = mk.mask; a.out = out; a.guided = gd.guided_out; a.seeds = seeds;
        a.xmap_lr = xmap_lr_for(l.chunks); a.bps_shift = l.bps_shift;
        a.mask_numel = (uint32_t)mk.mask_numel; a.mask_stride = (uint32_t)mk.batch_stride;
        a.stream0 = p.stream0; a.zeta0 = (float)p.zeta0; a.scale = (float)gd.scale; a.slot = gd.slot;
        a.factor = nullptr; a.phi = a.psi = 0.f;
        if constexpr (RESCALE) { a.factor = rs->factor_dev; a.phi = (float)rs->phi; a.psi = (float)(1.0 - rs->phi); }
        hipLaunchKernelGGL((guided_masked_kernel_v1<T, N, decltype(nz)::value, RESCALE>), dim3((unsigned)l.chunks), dim3(BLOCK), 0, s, a);
      });
    }, l.noise, rs != nullptr);
  });
}

// The checks of skr_step_launch_guided[_rescaled] behind its NULL tests, in its order and with its codes, for a launch that always has a
// step output and whose workgroups always lie inside one sample; numel == 0 skips the pointers, as there.
static int guided_masked_guidance_checks(const skr_step_plan& p, const skr_step_guidance& gd, const skr_step_rescale* rescale, const void* const* inputs,
                                         void* out, const uint64_t* seeds_dev, int64_t numel) {
  const bool step_out = p.out0_dtype != SKR_NONE;
  const bool noise = step_out && p.noise_mode == 1 && p.zeta0 != 0.0;
  if (noise && numel > 0 && !seeds_dev) return SKR_ERR_NULL;
  if (p.n_terms < 0 || p.n_terms > SKR_ROW_TERMS || p.n_group_a < 0 || p.n_group_a > p.n_terms) return SKR_ERR_TERMS;
  if (gd.slot < 0 || gd.slot >= p.n_terms) return SKR_ERR_TERMS;
  if (numel < 0) return SKR_ERR_SHAPE;
  if (!step_out && !gd.guided_out) return SKR_ERR_NULL;  // no output at all
  if (p.noise_mode != 0 && p.noise_mode != 1) return SKR_ERR_UNSUPPORTED;
  if (p.out1_dtype != SKR_NONE || p.chain != 0.0 || p.zeta1 != 0.0 || p.convert_to != 0 || p.convert_from != 0 || gd.reserved != 0) return SKR_ERR_UNSUPPORTED;
  if (rescale && rescale->reserved != 0) return SKR_ERR_UNSUPPORTED;
  if (!step_out) return SKR_ERR_UNSUPPORTED;  // there is no guidance-only form
  if (noise && numel > 0) {  // fused Philox needs every 8-element group inside one sample, as in skr_step_launch
    if (p.sample_numel <= 0 || numel % p.sample_numel != 0) return SKR_ERR_SHAPE;
    if (p.sample_numel % 8 != 0) return SKR_ERR_UNSUPPORTED;
  }
  if (rescale) {  // the statistic's sample: at least two elements, and the one the mask and the draw go by
    if (rescale->sample_numel < 2 || numel % rescale->sample_numel != 0) return SKR_ERR_SHAPE;
    if (numel > 0 && p.sample_numel != rescale->sample_numel) return SKR_ERR_SHAPE;
  }
  if (numel == 0) return SKR_OK;
  if (!inputs || !out || !gd.cond || (rescale && !rescale->factor_dev)) return SKR_ERR_NULL;
  if (const int rc = check_ptrs(inputs, p.n_terms)) return rc;
  if (!aligned16(out) || !aligned16(gd.cond) || !aligned16(gd.guided_out)) return SKR_ERR_ALIGN;
  const int32_t db = p.n_group_a == p.n_terms ? p.dtype_a : p.dtype_b;
  if (!step_inputs_ok(p.dtype_a, db, p.acc_f64) || !step_output_ok(p.out0_dtype, p.dtype_a, p.acc_f64)) return SKR_ERR_DTYPE;
  return SKR_OK;
}

}  // namespace skr

extern "C" int skr_guided_masked_step_launch(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                             const skr_step_rescale* rescale, const skr_step_mask* mask, const uint64_t* seeds_dev, int64_t numel,
                                             void* stream) {
  using namespace skr;
  if (!plan || !guide || !mask) return SKR_ERR_NULL;
  const skr_step_plan& p = *plan;
  if (const int rc = guided_masked_guidance_checks(p, *guide, rescale, inputs, out, seeds_dev, numel)) return rc;
  // the mask checks, and whether the one-trip geometry of the masked step -- this kernel's -- takes the launch
  MaskedLaunch l;
  if (const int rc = masked_prepare(p, *mask, inputs, out, seeds_dev, numel, false, &l)) return rc;
  if (numel == 0) return SKR_OK;
  if (!l.one_trip || p.coef1[guide->slot] != 0.0) return SKR_ERR_UNSUPPORTED;  // (the known form never contains the prediction)
  DeviceGuard device_guard(out);
  launch_guided_masked_v1(p, inputs, out, *guide, rescale, *mask, seeds_dev, l, reinterpret_cast<hipStream_t>(stream));
  return finish_launch();
}
