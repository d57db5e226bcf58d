// The step of adaptive projected guidance with device-resident scalars (include/skrample_hip.h,
// skr_projected_guided_step_launch_indexed[_per_sample]): skr_projected_guided_step_launch's one-trip kernel (skr_step_projected.hip) with
// everything a schedule or a projected setting changes taken from the row  rows[(index ? index[0] : 0) + row_offset]  (WholeBatch)  or
// rows[index[sample] + row_offset]  (PerSample):
//   coef0[K], zeta0, stream0   as skr_step_launch_indexed reads them; a row whose zeta0 narrows to zero skips the draw (a uniform branch)
//   convert_k[3]               beta, the momentum: what projected_kernel_v1 splits at compile time (DIFF) is a workgroup-uniform run-time
//                              choice here.  A momentum row's d is the loop's buffer, as the statistic left it; a zero-momentum row's d is
//                              rn_T(c - u), formed in registers from uncond, because the statistic stored nothing for that sample.
// convert_k[0..2] (g, eta, r) are the statistic's alone: A_s and B_s carry them.  Lane ownership, XCD chunk map, loads, stores and Philox
// numbering are projected_kernel_v1's, and so is every arithmetic operation: a sample has the bits the direct launch gives it alone with
// the row's values and diff given exactly when beta != 0.  There is no grid-stride form and no guidance-only form: whole 2048-element
// chunks, proj->sample_numel a multiple of 2048 -- a workgroup lies inside one sample --, one 16- or 32-bit dtype, 1 .. 16 operands.
//   one image at `slot`        the choice selects the BASE ADDRESS of the operand at `slot` -- proj->diff or inputs[slot] -- before that load
//                              is issued: one of the two is loaded, never both.  For that the index entry and the row's convert_k[3] are
//                              two scalar loads in front of the operand loads; the cond load, which needs neither, is issued ahead of them.
//   the row behind the loads   all K operand loads and the cond load stand in front of the scheduling barrier; the rest of the row, the
//                              seed and A_s, B_s are scalar loads through the constant address space behind it, while the loads are in
//                              flight.  Branches follow (the choice, the draw), and the barrier holds inside its basic block only: an empty
//                              statement that may write memory keeps the loads in front (thresholded_rows_kernel_v1's).
//   the row's doubles          stay in SGPRs and are narrowed where they are used, as in thresholded_rows_kernel_v1.
//   wide launches              16-bit launches of more than 12 operands keep 12 images in flight (11 operands and cond), as
//                              projected_kernel_v1 does; a staged operand at `slot` takes the chosen base like any other.
//   slot                       a kernarg scalar compared against the unrolled operand's number: no register array is indexed at run time.
#include "skr_projected.h"
#include "skr_step_guided_kernel.h"

namespace skr {

template <int KMAX>
struct ProjectedRowArgs {  // ProjectedArgs without the scalars a row carries, with both images the operand at `slot` may be
  const void* in[KMAX];  // in[slot]: uncond, loaded by the workgroups of a zero-momentum row
  const void* cond;
  const void* diff;      // the loop's buffer, loaded by the workgroups of a momentum row
  void* out;
  void* guided;          // nullptr: p is not stored
  int32_t xmap_lr;
  int32_t bps_shift;     // chunks per sample of the statistic (and of the draw)
  const uint64_t* seeds;
  const float* coef;     // [2 * samples]: A_s, B_s
  RowRef tab;
  int32_t slot;
};

template <typename T, int K>
constexpr int projected_rows_ahead() { return (sizeof(T) == 2 && K > 12) ? 11 : K; }  // (projected_ahead of skr_step_projected.hip)

template <typename T, int K, bool NOISE, RowForm F>
__global__ __launch_bounds__(BLOCK) void projected_rows_kernel_v1(const ProjectedRowArgs<guided_kmax(K)> a) {
  static_assert(row_behind_loads(F), "the two captured-loop forms");
  constexpr bool TILE = sizeof(T) == 4;
  constexpr int AHEAD = projected_rows_ahead<T, K>();
  const uint32_t c = chunk_of(blockIdx.x, a.xmap_lr);
  const int64_t v = (int64_t)c * BLOCK + threadIdx.x;
  const int32_t slot = a.slot;
  const Raw<T> rc = load_raw<T, TILE>(a.cond, v);
  uint32_t smp, within;
  sample_of(c, a.bps_shift, smp, within);
  smp = __builtin_amdgcn_readfirstlane(smp);  // (uniform over the workgroup) the index entry, the row, the seed and the coefficients are scalar loads
  int32_t at = 0;
  if constexpr (F == RowForm::PerSample) at = uniform(a.tab.index)[smp];
  else if (a.tab.index != nullptr) at = uniform(a.tab.index)[0];
  const auto row = uniform(a.tab.rows + (at + a.tab.row_offset));
  const bool stored = rescaling(row->convert_k[3]);  // (uniform) beta != +-0: d is the buffer's; otherwise it is formed from uncond
  Raw<T> raw[K];
#pragma unroll
  for (int j = 0; j < AHEAD; ++j) raw[j] = load_raw<T, TILE>((j == slot && stored) ? a.diff : a.in[j], v);
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);  // every load is out before the rest of the row and the sample's coefficients are asked for
  double c0[K];
#pragma unroll
  for (int j = 0; j < K; ++j) c0[j] = row->coef0[j];
  const float zeta0 = (float)row->zeta0;
  const float A = uniform(a.coef)[2 * smp], B = uniform(a.coef)[2 * smp + 1];  // (read-only for the launch: two scalar loads)
  float z[VEC];
  [[maybe_unused]] bool n0 = false;
  if constexpr (NOISE) {
    n0 = zeta0 != 0.f;
    if (n0) {  // (uniform: the row's)
      const uint64_t stream0 = row->stream0;
      const uint32_t vs = within * BLOCK + threadIdx.x;  // lane-vector within the sample (sample_numel < 2^31)
      const uint64_t seed = uniform(a.seeds)[smp];
      normal4(seed, stream0, (uint64_t)group0<TILE>((int64_t)vs), z);
      normal4(seed, stream0, (uint64_t)group1<TILE>((int64_t)vs), z + 4);
    }
  }
  float acc[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    float w[VEC];
    widen<T, float>(raw[j], w);
    if (j == slot) {  // (uniform) the difference, or uncond, stands here: the projected prediction takes its place
      float cf[VEC];
      widen<T, float>(rc, cf);
      if (!stored) {  // (uniform: the row's)
#pragma unroll
        for (int i = 0; i < VEC; ++i) w[i] = projected_diff<T>(w[i], cf[i]);
      }
#pragma unroll
      for (int i = 0; i < VEC; ++i) w[i] = projected_value<T>(cf[i], w[i], A, B);
      if (a.guided != nullptr) store8<T, float, TILE>(a.guided, v, w);  // (p is a value of T: the store's rounding is exact)
    }
    const float w0 = (float)c0[j];
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = fma_(w0, w[i], acc[i]);
    if constexpr (AHEAD < K) {  // operand j + AHEAD is loaded where operand j has been summed, into the registers that frees
      if (j + AHEAD < K) raw[j + AHEAD] = load_raw<T, TILE>((j + AHEAD == slot && stored) ? a.diff : a.in[j + AHEAD], v);
    }
  }
  if constexpr (NOISE) { if (n0) fma_noise8<float>(zeta0, z, acc); }
  store8<T, float, TILE>(a.out, v, acc);
}

// The two entries: the checks of skr_projected_guided_step_launch in its order, the row arguments where the thresholded row entries put theirs.
static int projected_rows_impl(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide, const skr_step_projection* proj,
                               const uint64_t* seeds_dev, int64_t numel, RowForm form, const skr_step_row* rows, const int32_t* index, int32_t row_offset, void* stream) {
  if (!plan || !guide || !proj || !rows || (per_sample_rows(form) && !index)) return SKR_ERR_NULL;
  const skr_step_plan& p = *plan;
  const bool step_out = p.out0_dtype != SKR_NONE;
  const bool noise = step_out && p.noise_mode == 1;  // (whether a draw happens is the row's business)
  if (noise && numel > 0 && !seeds_dev) return SKR_ERR_NULL;
  if (p.n_terms < 0 || p.n_terms > SKR_ROW_TERMS || p.n_group_a < 0 || p.n_group_a > p.n_terms) return SKR_ERR_TERMS;
  if (guide->slot < 0 || guide->slot >= p.n_terms) return SKR_ERR_TERMS;
  if (numel < 0) return SKR_ERR_SHAPE;
  if (!step_out && !guide->guided_out) return SKR_ERR_NULL;  // no output at all
  if (p.noise_mode != 0 && p.noise_mode != 1) return SKR_ERR_UNSUPPORTED;
  if (p.out1_dtype != SKR_NONE || p.convert_to != 0 || p.convert_from != 0 || guide->reserved != 0) return SKR_ERR_UNSUPPORTED;  // (chain and zeta1 are row values nobody reads)
  if (proj->reserved != 0 || p.acc_f64 != 0) return SKR_ERR_UNSUPPORTED;
  if (!step_out) return SKR_ERR_UNSUPPORTED;  // the guidance-only form has no row form
  if (noise && numel > 0) {
    if (p.sample_numel <= 0 || numel % p.sample_numel != 0) return SKR_ERR_SHAPE;
    if (p.sample_numel % 8 != 0) return SKR_ERR_UNSUPPORTED;
  }
  if (proj->sample_numel < 2 || numel % proj->sample_numel != 0) return SKR_ERR_SHAPE;
  if (noise && numel > 0 && p.sample_numel != proj->sample_numel) return SKR_ERR_SHAPE;
  if (numel == 0) return SKR_OK;
  if (!inputs || !out || !guide->cond || !proj->coef_dev || !proj->diff) return SKR_ERR_NULL;  // (a row may carry momentum: the buffer is required)
  if (const int rc = check_ptrs(inputs, p.n_terms)) return rc;
  if (!aligned16(out) || !aligned16(guide->cond) || !aligned16(guide->guided_out) || !aligned16(proj->diff) || (reinterpret_cast<uintptr_t>(proj->coef_dev) & 3u) != 0)
    return SKR_ERR_ALIGN;
  const int32_t db = p.n_group_a == p.n_terms ? p.dtype_a : p.dtype_b;
  if (!step_inputs_ok(p.dtype_a, db, false) || !step_output_ok(p.out0_dtype, p.dtype_a, false)) return SKR_ERR_DTYPE;  // (an fp64 tensor among them)

  constexpr int64_t CHUNK = (int64_t)BLOCK * VEC;
  const int t = p.dtype_a;
  const bool one_dtype = db == t && p.out0_dtype == t;
  const bool one_trip = g_tune.one_trip && one_dtype && (t != SKR_F32 || g_tune.tile) && p.n_terms >= 1 && numel % CHUNK == 0 && numel / CHUNK <= 0x7fffffffll &&
                        proj->sample_numel % CHUNK == 0 && proj->sample_numel < (1ll << 31);
  if (!one_trip || row_offset < 0) return SKR_ERR_UNSUPPORTED;  // the row forms have no other kernel
  DeviceGuard device_guard(out);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t chunks = numel / CHUNK;
  with_step_type<false>(t, [&](auto tt) {
    with_bools([&](auto nz) {
      with_row_form(form, [&](auto fm) {
        with_count<1, SKR_ROW_TERMS>(p.n_terms, [&](auto n) {
          using T = typename decltype(tt)::type;
          constexpr int N = decltype(n)::value, KMAX = guided_kmax(N);
          constexpr RowForm F = decltype(fm)::value;
          if constexpr (row_behind_loads(F)) {  // (no entry passes another form)
            ProjectedRowArgs<KMAX> a;
            for (int k = 0; k < KMAX; ++k) a.in[k] = k < N ? inputs[k] : nullptr;
            a.cond = guide->cond; a.diff = proj->diff; a.out = out; a.guided = guide->guided_out; a.seeds = seeds_dev; a.coef = proj->coef_dev;
            a.xmap_lr = xmap_lr_for(chunks); a.bps_shift = bps_shift_of(proj->sample_numel / CHUNK);
            a.tab = RowRef{rows, index, row_offset}; a.slot = guide->slot;
            hipLaunchKernelGGL((projected_rows_kernel_v1<T, N, decltype(nz)::value, F>), dim3((unsigned)chunks), dim3(BLOCK), 0, s, a);
          }
        });
      });
    }, noise);
  });
  return finish_launch();
}

}  // namespace skr

extern "C" int skr_projected_guided_step_launch_indexed(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                                        const skr_step_projection* proj, const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev,
                                                        const int32_t* index_dev, int32_t row_offset, void* stream) {
  return skr::projected_rows_impl(plan, inputs, out, guide, proj, seeds_dev, numel, skr::RowForm::WholeBatch, rows_dev, index_dev, row_offset, stream);
}

extern "C" int skr_projected_guided_step_launch_indexed_per_sample(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                                                   const skr_step_projection* proj, const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev,
                                                                   const int32_t* sample_index_dev, int32_t row_offset, void* stream) {
  return skr::projected_rows_impl(plan, inputs, out, guide, proj, seeds_dev, numel, skr::RowForm::PerSample, rows_dev, sample_index_dev, row_offset, stream);
}
