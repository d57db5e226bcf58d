// The thresholded solver step with device-resident scalars (include/skrample_hip.h, skr_thresholded_step_launch_indexed[_per_sample]):
// skr_thresholded_step_launch's one-trip kernel (skr_step_thresholded.hip) with everything a schedule or a thresholding setting changes
// taken from the row  rows[(index ? index[0] : 0) + row_offset]  (WholeBatch)  or  rows[index[sample] + row_offset]  (PerSample):
//   coef0[K], zeta0, stream0     as skr_step_launch_indexed reads them; a row whose zeta0 narrows to zero skips the draw (a uniform branch)
//   convert_k[0], convert_k[1]   a, b: the to_x weights, each narrowed to fp32 once on the device (v_cvt_f32_f64, round to nearest even:
//                                the host's (float) cast)
//   convert_k[3]                 the maximum: <= 1 is the plain-clip row -- s = 1 by a uniform branch, scale[sample] is NOT read
// convert_k[2] (the ratio) is the statistic's alone.  Lane ownership, XCD chunk map, loads, stores and Philox numbering are
// thresholded_kernel_v1's, and so is every arithmetic operation behind the scalars: a sample has the bits the direct launch gives it alone
// with the row's values.  There is no grid-stride form: whole 2048-element chunks, thr->sample_numel a multiple of 2048 -- a workgroup lies
// inside one sample --, one 16- or 32-bit dtype, 2 .. 16 operands.
//   the row behind the loads   every operand load is issued first; the index entry, the row, the seed and the scale are scalar loads
//                              through the constant address space behind the scheduling barrier, while the loads are in flight.  Three
//                              branches follow (the plain-clip test, the draw, the stores), and the barrier holds inside its basic block
//                              only: an empty statement that may write memory keeps the loads in front (guided_kernel_v1's CLOBBER).
//   the row's doubles          stay in SGPRs and are narrowed where they are used: as floats they would be K VGPRs live across the Philox
//                              rounds.
#include "skr_threshold.h"
#include "skr_step_guided_kernel.h"

namespace skr {

template <int KMAX>
struct ThresholdedRowArgs {  // ThresholdedArgs without the scalars a row carries
  const void* in[KMAX];
  void* out;            // nullptr: the thresholding-only form
  void* x0_out;         // nullptr: p is not stored
  int32_t xmap_lr;
  int32_t bps_shift;    // chunks per sample of the statistic (and of the draw)
  const uint64_t* seeds;
  const float* scale;   // float[samples]: read for the rows that select
  RowRef tab;
  int32_t slot, xslot;
};

template <typename T, int K, bool NOISE, RowForm F>
__global__ __launch_bounds__(BLOCK) void thresholded_rows_kernel_v1(const ThresholdedRowArgs<guided_kmax(K)> a) {
  static_assert(row_behind_loads(F), "the two captured-loop forms");
  constexpr bool TILE = sizeof(T) == 4;
  const uint32_t c = chunk_of(blockIdx.x, a.xmap_lr);
  const int64_t v = (int64_t)c * BLOCK + threadIdx.x;
  Raw<T> raw[K];
#pragma unroll
  for (int j = 0; j < K; ++j) raw[j] = load_raw<T, TILE>(a.in[j], v);
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);  // every load is out before the first scalar of the arithmetic (the index entry, the row) is fetched
  uint32_t smp, within;
  sample_of(c, a.bps_shift, smp, within);
  smp = __builtin_amdgcn_readfirstlane(smp);  // (uniform over the workgroup) the index entry, the row, the seed and the scale are scalar loads
  int32_t at = 0;
  if constexpr (F == RowForm::PerSample) at = uniform(a.tab.index)[smp];
  else if (a.tab.index != nullptr) at = uniform(a.tab.index)[0];
  const auto row = uniform(a.tab.rows + (at + a.tab.row_offset));
  double c0[K];
#pragma unroll
  for (int j = 0; j < K; ++j) c0[j] = row->coef0[j];
  const float zeta0 = (float)row->zeta0, wa = (float)row->convert_k[0], wb = (float)row->convert_k[1];
  float s = 1.f;
  if (!(row->convert_k[3] <= 1.0)) s = uniform(a.scale)[smp];  // (uniform) a plain-clip row's scale is never touched: it may be NaN or uninitialised
  const int32_t slot = a.slot, xslot = a.xslot;
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
  float x[VEC];
#pragma unroll
  for (int j = 0; j < K; ++j) if (j == xslot) widen<T, float>(raw[j], x);  // (uniform: a kernarg scalar against the unrolled operand's number)
  float acc[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
  const bool step_out = a.out != nullptr;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    float w[VEC];
    widen<T, float>(raw[j], w);
    if (j == slot) {  // (uniform) the thresholded prediction takes this operand's place
#pragma unroll
      for (int i = 0; i < VEC; ++i) w[i] = thresholded_value<T>(x0_value(wa, x[i], wb, w[i]), s);
      if (a.x0_out != nullptr) store8<T, float, TILE>(a.x0_out, v, w);  // (p is a value of T: the store's rounding is exact)
    }
    if (step_out) {
      const float w0 = (float)c0[j];
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = fma_(w0, w[i], acc[i]);
    }
  }
  if (!step_out) return;
  if constexpr (NOISE) { if (n0) fma_noise8<float>(zeta0, z, acc); }
  store8<T, float, TILE>(a.out, v, acc);
}

// Rolling batches (skr_thresholded_step_launch_rolling): rows[index[slot] + row_offset] for the slots of a rolling.RollingBatch, a kernel
// of its own because its statement order is the opposite one -- the row stands IN FRONT of the loads, as in step_kernel_k1's and
// guided_kernel_v1's Rolling forms (skr_step_fast.hip, skr_step_guided_kernel.h):
//   inactive slot    a negative index entry: the workgroup ends before its first vector-memory instruction; both outputs keep their bytes
//   slot, xslot      the model output and the sample are read for every active slot: x0 needs them.  The output's place is summed with
//                    the row's coefficient; the sample is summed unless both of its coefficients are exactly zero -- a step whose form
//                    does not hold it (a last step onto sigma = 0) then has the bits of the launches that never sum it
//   other operands   present iff row_has: an absent one is neither loaded nor summed, so a request in its multistep ramp-up has the bits
//                    of the narrower direct launch that holds exactly its operands, whatever the history rings hold; present ones are
//                    summed from zero in slot order
//   s                scale[slot] by scalar load for a row that selects; a plain-clip row takes s = 1 by a uniform branch, scale unread
//   the draw         a row whose zeta0 narrows to zero skips it; the seed is seeds[slot], the block numbers are local to the sample
//   wide launches    16-bit launches of more than 12 operands keep 12 loads in flight (step_kernel_k1's AHEAD); the sample is loaded in
//                    front whatever its number, because the operand at `slot` needs it
//   32-bit launches  the sample has a load of its own, outside the row's branches, and is kept as loaded; the last operand of a
//                    4-operand launch and the last two from 5 operands on are loaded where the first ones have been summed, into the
//                    registers that frees.  With every image in flight ten instantiations sat 1 to 4 VGPRs over the occupancy bracket
//                    of their per-sample twins; staged, none of the 90 is below its twin (profiles/thresholding_rolling_isa.txt)
// Lane ownership, XCD chunk map, the fp32 tile layout and Philox numbering are thresholded_kernel_v1's.  There is no thresholding-only
// instantiation: a rolling batch refuses the samplers that need one.
template <typename T, int K, bool NOISE>
__global__ __launch_bounds__(BLOCK) void thresholded_rolling_kernel_v1(const ThresholdedRowArgs<guided_kmax(K)> a) {
  constexpr bool TILE = sizeof(T) == 4;
  constexpr bool XOWN = sizeof(T) == 4;
  constexpr int AHEAD = (sizeof(T) == 2 && K > 12) ? 12 : (XOWN && K > 4) ? K - 2 : (XOWN && K > 3) ? K - 1 : K;
  const uint32_t c = chunk_of(blockIdx.x, a.xmap_lr);
  const int64_t v = (int64_t)c * BLOCK + threadIdx.x;
  uint32_t smp, within;
  const skr_step_row* row = rolling_row(a.tab, c, a.bps_shift, smp, within);
  if (row == nullptr) return;  // inactive slot: nothing read, nothing written
  const int32_t slot = a.slot, xslot = a.xslot;
  bool on[K];
  double c0[K];  // (narrowed where they are used: the doubles sit in SGPRs, the floats would be K VGPRs live across the loads and the Philox rounds)
#pragma unroll
  for (int j = 0; j < K; ++j) { on[j] = j == slot || j == xslot || row_has(row, j); c0[j] = row->coef0[j]; }
  const float zeta0 = (float)row->zeta0;
  const double wa_d = row->convert_k[0], wb_d = row->convert_k[1];
  const bool selecting = !(row->convert_k[3] <= 1.0);
  const uint64_t stream0 = row->stream0;
  // (each operand's pointer is fetched from the kernarg inside its branch, as in step_kernel_k1)
  Raw<T> raw[K];
#pragma unroll
  for (int j = 0; j < K; ++j) if (on[j] && (XOWN ? j < AHEAD && j != xslot : j < AHEAD || j == xslot)) raw[j] = load_raw<T, TILE>(a.in[j], v);
  [[maybe_unused]] Raw<T> rx;
  if constexpr (XOWN) {
    const void* px = a.in[0];
#pragma unroll
    for (int j = 1; j < K; ++j) if (j == xslot) px = a.in[j];
    rx = load_raw<T, TILE>(px, v);
  }
  float s = 1.f;
  if (selecting) s = uniform(a.scale)[smp];  // (uniform) a plain-clip row's scale is never touched: it may be NaN or uninitialised
  float z[VEC];
  [[maybe_unused]] bool n0 = false;
  if constexpr (NOISE) {
    n0 = zeta0 != 0.f;
    if (n0) {  // (uniform: the row's)
      const uint32_t vs = within * BLOCK + threadIdx.x;  // lane-vector within the sample (sample_numel < 2^31)
      const uint64_t seed = uniform(a.seeds)[smp];
      normal4(seed, stream0, (uint64_t)group0<TILE>((int64_t)vs), z);
      normal4(seed, stream0, (uint64_t)group1<TILE>((int64_t)vs), z + 4);
    }
  }
  const float wa = (float)wa_d, wb = (float)wb_d;
  // the sample for x0 is kept as loaded and widened where `slot` uses it: held as eight floats from here on, a 16-bit one cost the 4- to
  // 6-operand forms an occupancy bracket against their per-sample twins
  constexpr bool XRAW = sizeof(T) == 2;
  float x[VEC];
  if constexpr (XRAW) {
#pragma unroll
    for (int j = 0; j < K; ++j) if (j == xslot) rx = raw[j];  // (uniform: a kernarg scalar against the unrolled operand's number)
  }
  float acc[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    if (on[j]) {  // (uniform: the row's) present operands in slot order: the bits of the narrower launch that holds exactly these
      float w[VEC];
      if (XOWN && j == xslot) widen<T, float>(rx, w);
      else widen<T, float>(raw[j], w);
      if (j == slot) {  // (uniform) the thresholded prediction takes this operand's place
        widen<T, float>(rx, x);
#pragma unroll
        for (int i = 0; i < VEC; ++i) w[i] = thresholded_value<T>(x0_value(wa, x[i], wb, w[i]), s);
        if (a.x0_out != nullptr) store8<T, float, TILE>(a.x0_out, v, w);  // (p is a value of T: the store's rounding is exact)
      }
      if (j != xslot || row_has(row, j)) {  // (uniform) a sample the step's form does not hold is read for x0 and not summed
        const float w0 = (float)c0[j];
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = fma_(w0, w[i], acc[i]);
      }
    }
    if constexpr (AHEAD < K) {  // operand j + 12 is loaded where operand j has been summed, into the registers that frees
      if (j + AHEAD < K) { if (on[j + AHEAD] && j + AHEAD != xslot) raw[j + AHEAD] = load_raw<T, TILE>(a.in[j + AHEAD], v); }
    }
  }
  if constexpr (NOISE) { if (n0) fma_noise8<float>(zeta0, z, acc); }
  store8<T, float, TILE>(a.out, v, acc);
}

// The three entries: the checks of skr_thresholded_step_launch in its order, the row arguments where the rescaled row entries put theirs.
static int thresholded_rows_impl(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_threshold* thr, const uint64_t* seeds_dev,
                                 int64_t numel, RowForm form, const skr_step_row* rows, const int32_t* index, int32_t row_offset, void* stream) {
  if (!plan || !thr || !rows || (per_sample_rows(form) && !index)) return SKR_ERR_NULL;
  const skr_step_plan& p = *plan;
  const bool step_out = p.out0_dtype != SKR_NONE;
  const bool noise = step_out && p.noise_mode == 1;  // (whether a draw happens is the row's business)
  if (noise && numel > 0 && !seeds_dev) return SKR_ERR_NULL;
  if (p.n_terms < 0 || p.n_terms > SKR_ROW_TERMS || p.n_group_a < 0 || p.n_group_a > p.n_terms) return SKR_ERR_TERMS;
  if (thr->slot < 0 || thr->slot >= p.n_terms || thr->xslot < 0 || thr->xslot >= p.n_terms || thr->slot == thr->xslot) return SKR_ERR_TERMS;
  if (numel < 0) return SKR_ERR_SHAPE;
  if (!step_out && !thr->x0_out) return SKR_ERR_NULL;  // no output at all
  if (p.noise_mode != 0 && p.noise_mode != 1) return SKR_ERR_UNSUPPORTED;
  if (p.out1_dtype != SKR_NONE || p.convert_to != 0 || p.convert_from != 0 || thr->reserved != 0) return SKR_ERR_UNSUPPORTED;  // (chain and zeta1 are row values nobody reads)
  if (p.acc_f64 != 0) return SKR_ERR_UNSUPPORTED;
  if (!step_out && (out != nullptr || p.n_terms != 2)) return SKR_ERR_UNSUPPORTED;  // the thresholding-only form: the two operands, p alone
  if (noise && numel > 0) {
    if (p.sample_numel <= 0 || numel % p.sample_numel != 0) return SKR_ERR_SHAPE;
    if (p.sample_numel % 8 != 0) return SKR_ERR_UNSUPPORTED;
  }
  if (thr->sample_numel < 1 || numel % thr->sample_numel != 0) return SKR_ERR_SHAPE;
  if (noise && numel > 0 && p.sample_numel != thr->sample_numel) return SKR_ERR_SHAPE;
  if (numel == 0) return SKR_OK;
  if (!inputs || (step_out && !out) || !thr->scale_dev) return SKR_ERR_NULL;  // (a row may select: the scale is required)
  if (const int rc = check_ptrs(inputs, p.n_terms)) return rc;
  if ((step_out && !aligned16(out)) || !aligned16(thr->x0_out) || (reinterpret_cast<uintptr_t>(thr->scale_dev) & 3u) != 0) return SKR_ERR_ALIGN;
  const int32_t db = p.n_group_a == p.n_terms ? p.dtype_a : p.dtype_b;
  if (p.dtype_a == SKR_F64 || db == SKR_F64 || p.out0_dtype == SKR_F64) return SKR_ERR_UNSUPPORTED;
  if (!step_inputs_ok(p.dtype_a, db, false) || (step_out && !step_output_ok(p.out0_dtype, p.dtype_a, false))) return SKR_ERR_DTYPE;

  constexpr int64_t CHUNK = (int64_t)BLOCK * VEC;
  const int t = p.dtype_a;
  const bool one_dtype = db == t && (!step_out || p.out0_dtype == t);
  const bool one_trip = g_tune.one_trip && one_dtype && (t != SKR_F32 || g_tune.tile) && numel % CHUNK == 0 && numel / CHUNK <= 0x7fffffffll &&
                        thr->sample_numel % CHUNK == 0 && thr->sample_numel < (1ll << 31) && p.n_terms >= 2;
  if (!one_trip || row_offset < 0) return SKR_ERR_UNSUPPORTED;  // the row forms have no other kernel
  if (form == RowForm::Rolling && !step_out) return SKR_ERR_UNSUPPORTED;  // (a rolling batch has no thresholding-only tick)
  DeviceGuard device_guard(step_out ? out : thr->x0_out);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t chunks = numel / CHUNK;
  with_step_type<false>(t, [&](auto tt) {
    with_bools([&](auto nz) {
      with_row_form(form, [&](auto fm) {
        with_count<2, SKR_ROW_TERMS>(p.n_terms, [&](auto n) {
          using T = typename decltype(tt)::type;
          constexpr int N = decltype(n)::value, KMAX = guided_kmax(N);
          constexpr RowForm F = decltype(fm)::value;
          if constexpr (has_table(F)) {  // (no entry passes the kernarg form)
            ThresholdedRowArgs<KMAX> a;
            for (int k = 0; k < KMAX; ++k) a.in[k] = k < N ? inputs[k] : nullptr;
            a.out = step_out ? out : nullptr; a.x0_out = thr->x0_out; a.seeds = seeds_dev; a.scale = thr->scale_dev;
            a.xmap_lr = xmap_lr_for(chunks); a.bps_shift = bps_shift_of(thr->sample_numel / CHUNK);
            a.tab = RowRef{rows, index, row_offset}; a.slot = thr->slot; a.xslot = thr->xslot;
            if constexpr (row_behind_loads(F)) hipLaunchKernelGGL((thresholded_rows_kernel_v1<T, N, decltype(nz)::value, F>), dim3((unsigned)chunks), dim3(BLOCK), 0, s, a);
            else hipLaunchKernelGGL((thresholded_rolling_kernel_v1<T, N, decltype(nz)::value>), dim3((unsigned)chunks), dim3(BLOCK), 0, s, a);
          }
        });
      });
    }, noise);
  });
  return finish_launch();
}

}  // namespace skr

extern "C" int skr_thresholded_step_launch_indexed(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_threshold* thr,
                                                   const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev, const int32_t* index_dev,
                                                   int32_t row_offset, void* stream) {
  return skr::thresholded_rows_impl(plan, inputs, out, thr, seeds_dev, numel, skr::RowForm::WholeBatch, rows_dev, index_dev, row_offset, stream);
}

extern "C" int skr_thresholded_step_launch_indexed_per_sample(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_threshold* thr,
                                                              const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev,
                                                              const int32_t* sample_index_dev, int32_t row_offset, void* stream) {
  return skr::thresholded_rows_impl(plan, inputs, out, thr, seeds_dev, numel, skr::RowForm::PerSample, rows_dev, sample_index_dev, row_offset, stream);
}

extern "C" int skr_thresholded_step_launch_rolling(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_threshold* thr,
                                                   const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev, const int32_t* sample_index_dev,
                                                   int32_t row_offset, void* stream) {
  return skr::thresholded_rows_impl(plan, inputs, out, thr, seeds_dev, numel, skr::RowForm::Rolling, rows_dev, sample_index_dev, row_offset, stream);
}
