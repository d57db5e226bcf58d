// The guided solver step (include/skrample_hip.h, skr_step_launch_guided and its seven siblings): classifier-free guidance, and diffusers'
// rescale_noise_cfg of it where asked for, fused into the step launch.
//
//   p   = rn_T( u + rn_T( g * rn_T(c - u) ) )                u = inputs[slot], c = cond: torch's three tensor ops, one rounded op at a time in
//                                                            the op-math type of T (fp32; fp64 for fp64 tensors), g converted to it once
//   p'  = rn_T( rn_T(phi * rn_T(p * r)) + rn_T(psi * p) )    a rescaled launch: r = factor_dev[sample], what the statistics launch wrote
//                                                            (skr_guidance_stats.hip, skr_guidance_stats_rows.hip); psi = 1 - phi, formed in
//                                                            double and narrowed once.  p' = p in an unrescaled one
//   out = sum_k c0[k]*v_k + zeta0*N(stream0)                 v_slot = p', v_k = in_k otherwise: accumulated exactly as skr_step_launch does
//   guided_out = p'                                          (when asked for: the tensor the unfused loop hands to the step and keeps as history)
//
//   * one-trip kernel (guided_kernel_v1<T, K, NOISE, RowForm, RESCALE>): whole 2048-element chunks, samples made of whole chunks when it
//     draws, rescales or has per-sample rows, operands / cond / both outputs of one 16- or 32-bit dtype, fp32 arithmetic, <= 16 operands.
//     Lane ownership, XCD chunk map, loads, stores and Philox block numbering are those of masked_kernel_v1 (skr_step_masked.hip).  `slot`
//     is a kernarg scalar: each unrolled operand compares its own number with it (a uniform branch), so the register arrays are never
//     indexed at run time.  Whether p' is stored is a uniform branch on the pointer, not a template flag:
//     3 dtypes x 16 operand counts x 2 (noise) x 4 forms x 2 (rescale) = 768 instantiations, the template in skr_step_guided_kernel.h, the
//     RESCALE half compiled in skr_step_guided_rescaled.hip.
//   * general kernel (guided_kernel_gen<Acc, RESCALE>), Kernarg form only: grid-stride, one element per lane and trip, any size, any dtype
//     combination skr_step_launch takes, fp32 or fp64 arithmetic, ragged and small samples, and the guidance-only form (no step output).
// Both evaluate the same operations in the same order on every element, so they agree bit for bit where both apply.  One exception follows
// torch's own device op: for fp16 the elements past the last whole 2048 of the tensor have their tensor-times-number products (g * d,
// phi * resc, psi * p) rounded once (mul_once_f16, skr_step_guided.h).  Only the general kernel meets such elements.
//
// Eight entries, one template.  RowForm (skr_step_common.h) says where a launch's scalars come from, as for the plain and the masked step:
//   Kernarg     skr_step_launch_guided[_rescaled]                      coef0 / zeta0 / stream0 from the plan, g from guide->scale, phi from rescale->phi,
//                                                                      narrowed on the host.  The rescale is unconditional.
//   WholeBatch  skr_step_launch_guided[_rescaled]_indexed              from rows[index[0] + row_offset], read by the kernel behind its loads, so that a
//   PerSample   skr_step_launch_guided[_rescaled]_indexed_per_sample   captured loop serves any schedule, any guidance scale (convert_k[0]) and any
//                                                                      guidance_rescale (convert_k[1]); per sample: rows[index[sample] + row_offset]
//   Rolling     skr_step_launch_guided[_rescaled]_rolling              per-sample rows for the slots of a rolling.RollingBatch, the row fetch IN FRONT
//                                                                      of the loads (rolling_row), with the three rolling semantics:
//       inactive sample   a negative index entry (tested before row_offset is added) ends the workgroup before its first vector-memory
//                         instruction: no operand, cond, seed, factor or row is read, `out` and `guided_out` keep their bytes;
//       absent operand    an operand other than `slot` whose coef0 is exactly zero (either sign) in the row is neither loaded nor summed
//                         (history a request in its ramp-up does not have yet).  Its bytes may be NaN or inf, and its pointer is fetched from
//                         the kernarg inside its branch.  inputs[slot] and cond are always loaded, and p' takes its one fma whatever
//                         coef0[slot] is.  (The other forms give every operand its fma, zero coefficients included.)
//       operand order     the present operands are summed in slot order, one fma each, p' in the slot's place, noise last: the bits of the
//                         narrower Kernarg launch that holds exactly these operands.
// A row launch is bit for bit the Kernarg launch with the row's values in its plan, guide and rescale.  A row is uniform over the workgroup
// (the sample id goes through readfirstlane, the index entry and the row are scalar loads), so every decision taken from it is a scalar
// branch with exec never masked: a NOISE instantiation skips the draw for a row whose zeta0 narrows to zero, and a RESCALE one rescales
// only where the row's phi is not +-0 -- a real branch, not arithmetic (0 * inf would leak through), with the factor's load inside it:
// an unrescaled row never touches the factor, which may hold NaN.  A rescaling launch keeps a workgroup inside one sample of the
// statistic in every form.  The row forms have no grid-stride kernel: what the one-trip kernel does not cover is SKR_ERR_UNSUPPORTED.
#include "skr_step_guided_kernel.h"

namespace skr {

// ---- general kernel: per-element accesses, run-time dtypes -----------------------------------------------------------------
struct GuidedGenArgs {
  const void* in[SKR_ROW_TERMS];
  double c0[SKR_ROW_TERMS];
  const void* cond;
  void* out;      // nullptr: the guidance-only form
  void* guided;   // nullptr: p' is not stored
  const uint64_t* seeds;
  double zeta0, scale;
  uint64_t stream0;
  int64_t numel, sample_numel;
  int32_t n, n_a, dt_a, dt_b, dt_out, dt_g, slot, noise;
};
struct GuidedRescaledGenArgs {
  const void* in[SKR_ROW_TERMS];
  double c0[SKR_ROW_TERMS];
  const void* cond;
  void* out;
  void* guided;
  const uint64_t* seeds;
  const void* factor;
  double zeta0, scale, phi, psi;
  uint64_t stream0;
  int64_t numel, sample_numel, stat_numel;  // the draw's sample and the statistic's (equal when the launch draws)
  int32_t n, n_a, dt_a, dt_b, dt_out, dt_g, slot, noise;
};

// p' of one element in fp32 op-math; TAIL: an fp16 element of torch's partial last block
template <typename T, bool RESCALE, bool TAIL = false>
__device__ __forceinline__ float guided_gen_value(float u, float c, float g, float r, float phi, float psi) {
  if constexpr (TAIL) {
    const float p = guided_value_f16_tail(u, c, g);
    if constexpr (RESCALE) return rescaled_value_f16_tail(p, r, phi, psi);
    else return p;
  } else {
    const float p = guided_value<T>(u, c, g);
    if constexpr (RESCALE) return rescaled_value<T>(p, r, phi, psi);
    else return p;
  }
}

template <typename Acc, bool RESCALE>
__global__ __launch_bounds__(BLOCK) void guided_kernel_gen(const std::conditional_t<RESCALE, GuidedRescaledGenArgs, GuidedGenArgs> a) {
  constexpr bool F64 = std::is_same<Acc, double>::value;  // (an fp64 tensor takes part in fp64 arithmetic only)
  const int64_t tail_from = a.numel - a.numel % TORCH_TAIL;  // fp16: torch rounds a tensor-times-number product once from here on (mul_once_f16)
  for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < a.numel; e += (int64_t)gridDim.x * BLOCK) {
    [[maybe_unused]] int64_t stat_smp = 0;
    if constexpr (RESCALE) stat_smp = e / a.stat_numel;
    // p', in the op-math type of the slot's dtype whatever the accumulate type is; then widened exactly
    Acc p;
    bool wide_p = false;
    if constexpr (F64) wide_p = a.dt_g == SKR_F64;
    if (wide_p) {
      const double* up = reinterpret_cast<const double*>(a.in[a.slot]);
      const double* cp = reinterpret_cast<const double*>(a.cond);
      if constexpr (RESCALE) p = (Acc)rescaled_d(guide_d(up[e], cp[e], a.scale), reinterpret_cast<const double*>(a.factor)[stat_smp], a.phi, a.psi);
      else p = (Acc)guide_d(up[e], cp[e], a.scale);
    } else {
      const float u = load_elem<float, false>(a.in[a.slot], e, a.dt_g), cv = load_elem<float, false>(a.cond, e, a.dt_g);
      float r = 0.f, phi = 0.f, psi = 0.f;
      if constexpr (RESCALE) r = load_elem<float, false>(a.factor, stat_smp, a.dt_g);
      const float g = (float)a.scale;
      if constexpr (RESCALE) { phi = (float)a.phi; psi = (float)a.psi; }
      float pf;
      if (a.dt_g == SKR_BF16) pf = guided_gen_value<bf16_t, RESCALE>(u, cv, g, r, phi, psi);
      else if (a.dt_g == SKR_F16) pf = e >= tail_from ? guided_gen_value<f16_t, RESCALE, true>(u, cv, g, r, phi, psi) : guided_gen_value<f16_t, RESCALE>(u, cv, g, r, phi, psi);
      else pf = guided_gen_value<float, RESCALE>(u, cv, g, r, phi, psi);
      p = (Acc)pf;
    }
    if (a.guided != nullptr) store_any<Acc>(a.guided, e, a.dt_g, p);  // (p' is a value of that dtype: exact)
    if (a.out == nullptr) continue;
    Acc s = 0;
    for (int j = 0; j < a.n; ++j) {
      Acc x = load_elem<Acc, F64>(a.in[j], e, j < a.n_a ? a.dt_a : a.dt_b);
      if (j == a.slot) x = p;
      s = fma_((Acc)a.c0[j], x, s);
    }
    if (a.noise) {  // element r of the sample: Philox block r >> 2, lane r & 3 (sample_numel % 8 == 0, checked on the host)
      const int64_t smp = e / a.sample_numel, r = e - smp * a.sample_numel;
      float z[4];
      normal4(a.seeds[smp], a.stream0, (uint64_t)r >> 2, z);
      const int lane = (int)(r & 3);
      const float zz = lane == 0 ? z[0] : (lane == 1 ? z[1] : (lane == 2 ? z[2] : z[3]));
      s = fma_((Acc)a.zeta0, (Acc)zz, s);
    }
    store_any<Acc>(a.out, e, a.dt_out, s);
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// the general launch (Kernarg form): accumulate type x rescale, and its kernarg
static void launch_guided_gen(const skr_step_plan& p, const void* const* inputs, void* out, const skr_step_guidance& gd, const skr_step_rescale* rs,
                              const uint64_t* seeds, const GuidedLaunch& l, int64_t numel, hipStream_t s) {
  with_bools([&](auto f64, auto re) {
    constexpr bool RESCALE = decltype(re)::value;
    std::conditional_t<RESCALE, GuidedRescaledGenArgs, GuidedGenArgs> a;
    for (int k = 0; k < SKR_ROW_TERMS; ++k) {
      const bool live = k < p.n_terms;
      a.in[k] = live ? inputs[k] : nullptr;
      a.c0[k] = live ? p.coef0[k] : 0.0;
    }
    a.cond = gd.cond; a.out = l.step_out ? out : nullptr; a.guided = gd.guided_out; a.seeds = seeds;
    a.zeta0 = p.zeta0; a.scale = gd.scale; a.stream0 = p.stream0;
    a.numel = numel; a.sample_numel = l.noise ? p.sample_numel : numel;
    if constexpr (RESCALE) { a.factor = rs->factor_dev; a.phi = rs->phi; a.psi = 1.0 - rs->phi; a.stat_numel = rs->sample_numel; }
    a.n = p.n_terms; a.n_a = p.n_group_a; a.dt_a = p.dtype_a; a.dt_b = l.dtype_b; a.dt_out = p.out0_dtype; a.dt_g = l.dtype_g; a.slot = gd.slot;
    a.noise = l.noise ? 1 : 0;
    const dim3 grid((unsigned)grid_blocks(numel, BLOCK, 256 * 64));
    hipLaunchKernelGGL((guided_kernel_gen<std::conditional_t<decltype(f64)::value, double, float>, RESCALE>), grid, dim3(BLOCK), 0, s, a);
  }, p.acc_f64 != 0, rs != nullptr);
}

// Every check of a guided launch behind its NULL tests: those of skr_step_launch in its order, with what the guidance adds where the like
// of it stands there.  `rows`: for a row form, whose plan scalars are ignored.  SKR_OK with numel == 0 means "nothing to do".
// `rescale` (nullptr: an unrescaled entry): what it adds is checked where the like of it stands -- `reserved` beside the guide's, the
// sample size behind that of a launch that draws, factor_dev beside the operands.
static int guided_prepare(const skr_step_plan& p, const skr_step_guidance& gd, const void* const* inputs, void* out, const uint64_t* seeds_dev, int64_t numel,
                          bool rows, GuidedLaunch* launch, const skr_step_rescale* rescale) {
  launch->step_out = launch->noise = launch->one_trip = false;
  const bool step_out = p.out0_dtype != SKR_NONE;
  const bool noise = step_out && p.noise_mode == 1 && (rows || p.zeta0 != 0.0);
  if (noise && numel > 0 && !seeds_dev) return SKR_ERR_NULL;
  if (p.n_terms < 0 || p.n_terms > SKR_ROW_TERMS || p.n_group_a < 0 || p.n_group_a > p.n_terms) return SKR_ERR_TERMS;
  if (gd.slot < 0 || gd.slot >= p.n_terms) return SKR_ERR_TERMS;
  if (numel < 0) return SKR_ERR_SHAPE;
  if (!step_out && !gd.guided_out) return SKR_ERR_NULL;  // no output at all
  if (p.noise_mode != 0 && p.noise_mode != 1) return SKR_ERR_UNSUPPORTED;
  if (p.out1_dtype != SKR_NONE || p.chain != 0.0 || p.zeta1 != 0.0 || p.convert_to != 0 || p.convert_from != 0 || gd.reserved != 0) return SKR_ERR_UNSUPPORTED;
  if (rescale && rescale->reserved != 0) return SKR_ERR_UNSUPPORTED;
  if (!step_out && (out != nullptr || p.n_terms != 1)) return SKR_ERR_UNSUPPORTED;  // the guidance-only form: one operand, p alone
  if (noise && numel > 0) {  // fused Philox needs every 8-element group inside one sample, as in skr_step_launch
    if (p.sample_numel <= 0 || numel % p.sample_numel != 0) return SKR_ERR_SHAPE;
    if (p.sample_numel % 8 != 0) return SKR_ERR_UNSUPPORTED;
  }
  if (rescale) {  // the statistic's sample: at least two elements (an unbiased std), and the one the noise is drawn by
    if (rescale->sample_numel < 2 || numel % rescale->sample_numel != 0) return SKR_ERR_SHAPE;
    if (noise && numel > 0 && p.sample_numel != rescale->sample_numel) return SKR_ERR_SHAPE;
  }
  if (numel == 0) return SKR_OK;
  if (!inputs || (step_out && !out) || !gd.cond || (rescale && !rescale->factor_dev)) return SKR_ERR_NULL;
  if (const int rc = check_ptrs(inputs, p.n_terms)) return rc;
  if ((step_out && !aligned16(out)) || !aligned16(gd.cond) || !aligned16(gd.guided_out)) return SKR_ERR_ALIGN;
  // the dtype combinations of skr_step_launch, with one output; an fp64 group (the slot's or not) needs fp64 arithmetic
  const int32_t db = p.n_group_a == p.n_terms ? p.dtype_a : p.dtype_b;
  if (!step_inputs_ok(p.dtype_a, db, p.acc_f64) || (step_out && !step_output_ok(p.out0_dtype, p.dtype_a, p.acc_f64))) return SKR_ERR_DTYPE;
  launch->step_out = step_out; launch->noise = noise;
  launch->dtype_b = db; launch->dtype_g = gd.slot < p.n_group_a ? p.dtype_a : db;

  constexpr int64_t CHUNK = (int64_t)BLOCK * VEC;
  const int t = p.dtype_a;
  const bool one_dtype = db == t && p.out0_dtype == t && t != SKR_F64;
  if (g_tune.one_trip && step_out && !p.acc_f64 && one_dtype && (t != SKR_F32 || g_tune.tile) && numel % CHUNK == 0 && numel / CHUNK <= 0x7fffffffll &&
      (!noise || (p.sample_numel % CHUNK == 0 && p.sample_numel < (1ll << 31)))) {
    launch->one_trip = true; launch->chunks = numel / CHUNK; launch->bps_shift = noise ? bps_shift_of(p.sample_numel / CHUNK) : 0;
  }
  return SKR_OK;
}

// The eight entries (from the table test on: rows != nullptr exactly when has_table(form); `rescaled`: the entry has a rescale argument).
static int guided_launch_impl(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide, bool rescaled,
                              const skr_step_rescale* rescale, const uint64_t* seeds_dev, int64_t numel, RowForm form, const skr_step_row* rows,
                              const int32_t* index, int32_t row_offset, void* stream) {
  const bool table = has_table(form);
  if (!plan || !guide || (rescaled && !rescale) || (table && (!rows || (per_sample_rows(form) && !index)))) return SKR_ERR_NULL;
  const skr_step_plan& p = *plan;
  GuidedLaunch l;
  if (const int rc = guided_prepare(p, *guide, inputs, out, seeds_dev, numel, table, &l, rescale)) return rc;
  if (numel == 0) return SKR_OK;
  constexpr int64_t CHUNK = (int64_t)BLOCK * VEC;
  if (table) {
    if (!l.one_trip || row_offset < 0) return SKR_ERR_UNSUPPORTED;
    if (per_sample_rows(form) || rescale) {  // a workgroup lies inside one sample, with or without noise, and a rescaled one inside the statistic's
      if (p.sample_numel <= 0 || numel % p.sample_numel != 0 || (rescale && rescale->sample_numel != p.sample_numel)) return SKR_ERR_SHAPE;
      if (p.sample_numel % CHUNK != 0 || p.sample_numel >= (1ll << 31)) return SKR_ERR_UNSUPPORTED;
      l.bps_shift = bps_shift_of(p.sample_numel / CHUNK);
    }
  } else if (rescale && l.one_trip) {  // a workgroup inside one sample of the statistic, or the general kernel
    l.one_trip = rescale->sample_numel % CHUNK == 0 && rescale->sample_numel < (1ll << 31);
    if (l.one_trip) l.bps_shift = bps_shift_of(rescale->sample_numel / CHUNK);
  }
  DeviceGuard device_guard(l.step_out ? out : guide->guided_out);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (l.one_trip && rescale) launch_guided_rescaled_v1(p, inputs, out, *guide, rescale, seeds_dev, l, form, RowRef{rows, index, row_offset}, s);
  else if (l.one_trip) launch_guided_v1<false>(p, inputs, out, *guide, nullptr, seeds_dev, l, form, RowRef{rows, index, row_offset}, s);
  else launch_guided_gen(p, inputs, out, *guide, rescale, seeds_dev, l, numel, s);
  return finish_launch();
}

}  // namespace skr

using skr::RowForm;

extern "C" int skr_step_launch_guided(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                      const uint64_t* seeds_dev, int64_t numel, void* stream) {
  return skr::guided_launch_impl(plan, inputs, out, guide, false, nullptr, seeds_dev, numel, RowForm::Kernarg, nullptr, nullptr, 0, stream);
}

extern "C" int skr_step_launch_guided_indexed(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                              const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev, const int32_t* index_dev,
                                              int32_t row_offset, void* stream) {
  return skr::guided_launch_impl(plan, inputs, out, guide, false, nullptr, seeds_dev, numel, RowForm::WholeBatch, rows_dev, index_dev, row_offset, stream);
}

extern "C" int skr_step_launch_guided_indexed_per_sample(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                                         const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev,
                                                         const int32_t* sample_index_dev, int32_t row_offset, void* stream) {
  return skr::guided_launch_impl(plan, inputs, out, guide, false, nullptr, seeds_dev, numel, RowForm::PerSample, rows_dev, sample_index_dev, row_offset, stream);
}

extern "C" int skr_step_launch_guided_rolling(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                              const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev,
                                              const int32_t* sample_index_dev, int32_t row_offset, void* stream) {
  return skr::guided_launch_impl(plan, inputs, out, guide, false, nullptr, seeds_dev, numel, RowForm::Rolling, rows_dev, sample_index_dev, row_offset, stream);
}

extern "C" int skr_step_launch_guided_rescaled(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                               const skr_step_rescale* rescale, const uint64_t* seeds_dev, int64_t numel, void* stream) {
  return skr::guided_launch_impl(plan, inputs, out, guide, true, rescale, seeds_dev, numel, RowForm::Kernarg, nullptr, nullptr, 0, stream);
}

extern "C" int skr_step_launch_guided_rescaled_indexed(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                                       const skr_step_rescale* rescale, const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev,
                                                       const int32_t* index_dev, int32_t row_offset, void* stream) {
  return skr::guided_launch_impl(plan, inputs, out, guide, true, rescale, seeds_dev, numel, RowForm::WholeBatch, rows_dev, index_dev, row_offset, stream);
}

extern "C" int skr_step_launch_guided_rescaled_indexed_per_sample(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                                                  const skr_step_rescale* rescale, const uint64_t* seeds_dev, int64_t numel,
                                                                  const skr_step_row* rows_dev, const int32_t* sample_index_dev, int32_t row_offset, void* stream) {
  return skr::guided_launch_impl(plan, inputs, out, guide, true, rescale, seeds_dev, numel, RowForm::PerSample, rows_dev, sample_index_dev, row_offset, stream);
}

extern "C" int skr_step_launch_guided_rescaled_rolling(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                                       const skr_step_rescale* rescale, const uint64_t* seeds_dev, int64_t numel,
                                                       const skr_step_row* rows_dev, const int32_t* sample_index_dev, int32_t row_offset, void* stream) {
  return skr::guided_launch_impl(plan, inputs, out, guide, true, rescale, seeds_dev, numel, RowForm::Rolling, rows_dev, sample_index_dev, row_offset, stream);
}
