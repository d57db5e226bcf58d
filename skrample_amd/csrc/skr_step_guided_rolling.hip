// The guided solver step for the slots of a rolling batch (include/skrample_hip.h, skr_step_launch_guided_rolling): the per-sample row form
// of guided_kernel_v1 (skr_step_guided_rows.hip) with the three semantics and the statement order of the rolling forms
// (masked_kernel_v1<..., RowForm::Rolling> of skr_step_masked.hip, step_kernel_k1's rolling form of skr_step_fast.hip).
//
//   p   = rn_T( u + rn_T( g * rn_T(c - u) ) )       u = inputs[slot], c = cond;  g = (float)row.convert_k[0]: each sample its own scale
//   out = sum_k c0[k]*v_k + zeta0*N(stream0)        v_slot = p, v_k = in_k otherwise, over the PRESENT operands;  c0 / zeta0 / stream0 from the row
//   guided_out = p                                  (when asked for)
//
// The row fetch stands IN FRONT of the loads (rolling_row, skr_step_common.h), two dependent scalar round trips per wave:
//   inactive sample   a negative index entry (tested before row_offset is added) ends the workgroup before its first vector-memory
//                     instruction: no operand, cond, seed or row is read, `out` and `guided_out` keep their bytes;
//   absent operand    an operand other than `slot` whose coef0 is exactly zero (either sign) in the row is neither loaded nor summed
//                     (history a request in its ramp-up does not have yet).  Its bytes may be NaN or inf, and its pointer is fetched from
//                     the kernarg inside its branch.  The row's coef1 is not read.  inputs[slot] and cond are always loaded, and p takes
//                     its one fma whatever coef0[slot] is, as in skr_step_launch_guided;
//   operand order     the present operands are summed in slot order, one fma each, p in the slot's place, noise last and only when the
//                     row's zeta0 narrows to non-zero: the bits of the narrower skr_step_launch_guided that holds exactly these operands.
// Lane ownership, XCD chunk map, 16-byte loads and stores, Philox block numbering and the fp32 tile layout are the twins'.  A row is uniform
// over the workgroup (the sample id goes through readfirstlane, the index entry and the row are scalar loads), so every decision taken
// from it, and the `slot` test of each unrolled operand, is a scalar branch.  There is no grid-stride form: what the one-trip kernel does
// not cover is SKR_ERR_UNSUPPORTED.
#include "skr_step_guided.h"
#include "skr_device.h"

namespace skr {

// Kernarg: GuidedRowArgs (skr_step_guided_rows.hip) member for member.  What the first instructions need (chunk map, row reference) is
// read first; an operand's pointer is read inside the branch that loads it.
template <int KMAX>
struct GuidedRollingArgs {
  const void* in[KMAX];
  const void* cond;
  void* out;
  void* guided;         // nullptr: p is not stored
  int32_t xmap_lr;      // log2(run length) of the XCD chunk map
  int32_t bps_shift;    // chunks per sample: log2 when >= 0, minus the count otherwise (see sample_of)
  const uint64_t* seeds;
  RowRef tab;
  int32_t slot;         // the operand that p replaces in the sum
};

template <typename T, int K, bool NOISE>
__global__ __launch_bounds__(BLOCK) void guided_rolling_kernel_v1(const GuidedRollingArgs<guided_kmax(K)> a) {
  constexpr bool TILE = sizeof(T) == 4;  // whole chunks are whole tiles: 32-bit tensors take the whole-line layout, as in guided_kernel_v1
  const uint32_t c = chunk_of(blockIdx.x, a.xmap_lr);
  const int64_t v = (int64_t)c * BLOCK + threadIdx.x;
  uint32_t smp, within;
  const skr_step_row* row = rolling_row(a.tab, c, a.bps_shift, smp, within);
  if (row == nullptr) return;  // inactive sample: nothing read, nothing written
  const int32_t slot = a.slot;
  // (a row's doubles stay in SGPRs and are narrowed where they are used, as in masked_kernel_v1's table forms)
  double c0[K];
  bool on[K];  // operand j is present
#pragma unroll
  for (int j = 0; j < K; ++j) { c0[j] = row->coef0[j]; on[j] = j == slot || guided_row_has(row, j); }
  const float zeta0 = (float)row->zeta0, g = (float)row->convert_k[0];
  [[maybe_unused]] const uint64_t stream0 = row->stream0;
  Raw<T> raw[K];
#pragma unroll
  for (int j = 0; j < K; ++j) if (on[j]) raw[j] = load_raw<T, TILE>(a.in[j], v);
  Raw<T> rc = load_raw<T, TILE>(a.cond, v);
  // A NOISE instantiation serves every row: one whose zeta0 narrows to zero skips the draw (a uniform branch), as a launch without noise does.
  float z[VEC];
  [[maybe_unused]] bool n0 = false;
  if constexpr (NOISE) {
    n0 = zeta0 != 0.f;
    if (n0) {
      const uint32_t vs = within * BLOCK + threadIdx.x;  // lane-vector within the sample (sample_numel < 2^31)
      const uint64_t seed = a.seeds[smp];
      normal4(seed, stream0, (uint64_t)group0<TILE>((int64_t)vs), z);
      normal4(seed, stream0, (uint64_t)group1<TILE>((int64_t)vs), z + 4);
    }
  }
  float s[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) s[i] = 0.f;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    if (on[j]) {  // (uniform: the row's) present operands in slot order: the bits of the narrower launch that holds exactly these
      float w[VEC];
      widen<T, float>(raw[j], w);
      if (j == slot) {  // (uniform: a kernarg scalar against the unrolled operand's number) the guided value takes this operand's place
        float cf[VEC];
        widen<T, float>(rc, cf);
#pragma unroll
        for (int i = 0; i < VEC; ++i) w[i] = guided_value<T>(w[i], cf[i], g);
        if (a.guided != nullptr) store8<T, float, TILE>(a.guided, v, w);  // (p is a value of T: the store's rounding is exact)
      }
      const float w0 = (float)c0[j];
#pragma unroll
      for (int i = 0; i < VEC; ++i) s[i] = fma_(w0, w[i], s[i]);
    }
  }
  if constexpr (NOISE) { if (n0) fma_noise8<float>(zeta0, z, s); }
  store8<T, float, TILE>(a.out, v, s);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// dtype x noise x operand count to the instantiation, and its kernarg
static void launch_guided_rolling_v1(const skr_step_plan& p, const void* const* inputs, void* out, const skr_step_guidance& gd, const uint64_t* seeds,
                                     const GuidedLaunch& l, const RowRef& tab, hipStream_t s) {
  with_step_type<false>(p.dtype_a, [&](auto tt) {
    with_bools([&](auto nz) {
      with_count<1, SKR_ROW_TERMS>(p.n_terms, [&](auto n) {
        using T = typename decltype(tt)::type;
        constexpr int N = decltype(n)::value, KMAX = guided_kmax(N);
        GuidedRollingArgs<KMAX> a;
        for (int k = 0; k < KMAX; ++k) a.in[k] = k < N ? inputs[k] : nullptr;
        a.cond = gd.cond; a.out = out; a.guided = gd.guided_out; a.seeds = seeds;
        a.xmap_lr = xmap_lr_for(l.chunks); a.bps_shift = l.bps_shift;
        a.tab = tab; a.slot = gd.slot;
        hipLaunchKernelGGL((guided_rolling_kernel_v1<T, N, decltype(nz)::value>), dim3((unsigned)l.chunks), dim3(BLOCK), 0, s, a);
      });
    }, l.noise);
  });
}

// The entry: the checks of skr_step_launch_guided_indexed_per_sample, in its order and with its codes.
static int guided_rolling_launch_impl(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                      const uint64_t* seeds_dev, int64_t numel, void* stream, const skr_step_row* rows, const int32_t* index,
                                      int32_t row_offset) {
  if (!plan || !guide || !rows || !index) return SKR_ERR_NULL;
  const skr_step_plan& p = *plan;
  GuidedLaunch l;
  if (const int rc = guided_prepare(p, *guide, inputs, out, seeds_dev, numel, true, &l)) return rc;
  if (numel == 0) return SKR_OK;
  if (!l.one_trip || row_offset < 0) return SKR_ERR_UNSUPPORTED;
  // a workgroup lies inside one sample, with or without noise
  constexpr int64_t CHUNK = (int64_t)BLOCK * VEC;
  if (p.sample_numel <= 0 || numel % p.sample_numel != 0) return SKR_ERR_SHAPE;
  if (p.sample_numel % CHUNK != 0 || p.sample_numel >= (1ll << 31)) return SKR_ERR_UNSUPPORTED;
  l.bps_shift = bps_shift_of(p.sample_numel / CHUNK);
  DeviceGuard device_guard(out);
  launch_guided_rolling_v1(p, inputs, out, *guide, seeds_dev, l, RowRef{rows, index, row_offset}, reinterpret_cast<hipStream_t>(stream));
  return finish_launch();
}

}  // namespace skr

extern "C" int skr_step_launch_guided_rolling(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                              const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev,
                                              const int32_t* sample_index_dev, int32_t row_offset, void* stream) {
  return skr::guided_rolling_launch_impl(plan, inputs, out, guide, seeds_dev, numel, stream, rows_dev, sample_index_dev, row_offset);
}
