// The guided solver step with device-resident scalars (include/skrample_hip.h, skr_step_launch_guided_indexed[_per_sample]): the row forms
// of guided_kernel_v1 (skr_step_guided.hip), so that a captured classifier-free-guidance loop serves any schedule AND any guidance scale.
//
//   p   = rn_T( u + rn_T( g * rn_T(c - u) ) )       u = inputs[slot], c = cond;  g = (float)row.convert_k[0]
//   out = sum_k c0[k]*v_k + zeta0*N(stream0)        v_slot = p, v_k = in_k otherwise;  c0 / zeta0 / stream0 from the row
//   guided_out = p                                  (when asked for)
//
// One kernel template, guided_rows_kernel_v1<T, K, NOISE, RowForm>, for the two forms whose row is read behind the loads
// (row_behind_loads, skr_step_common.h):
//   WholeBatch  skr_step_launch_guided_indexed              rows[index[0] + row_offset]
//   PerSample   skr_step_launch_guided_indexed_per_sample   rows[index[sample] + row_offset], one entry per sample
// Lane ownership, XCD chunk map, loads, stores, Philox block numbering and the fp32 tile layout are guided_kernel_v1's: every operand load
// and the cond load are issued first, the index entry and the row are fetched behind them -- scalar loads: the sample number goes through
// readfirstlane -- and the row's doubles are narrowed while the loads are in flight, with the conversion the host applies to a plan's.
// `slot`, `cond` and `guided_out` stay launch arguments (frozen into a graph); `slot` is compared per unrolled operand, so the register
// arrays are never indexed at run time.  A NOISE instantiation serves every row: one whose zeta0 narrows to zero skips the draw (a uniform
// branch), as a launch without noise does.  Every operation on an element is guided_kernel_v1's, in its order, so a row launch has the bits
// of skr_step_launch_guided with the row's values in its plan and guide->scale.
// There is no grid-stride row form: what the one-trip kernel does not cover is SKR_ERR_UNSUPPORTED.
#include "skr_step_guided.h"
#include "skr_device.h"

namespace skr {

// Kernarg of the row forms: GuidedArgs (skr_step_guided.hip) without the scalars a row carries.  What the first instructions need
// (operand pointers, chunk map) leads; up to 4 operands it is two 64-byte lines.
template <int KMAX>
struct GuidedRowArgs {
  const void* in[KMAX];
  const void* cond;
  void* out;
  void* guided;         // nullptr: p is not stored
  int32_t xmap_lr;      // log2(run length) of the XCD chunk map
  int32_t bps_shift;    // chunks per sample: log2 when >= 0, minus the count otherwise (see sample_of); read by PerSample and by a launch that draws
  const uint64_t* seeds;
  RowRef tab;
  int32_t slot;         // the operand that p replaces in the sum
};

// The row of a workgroup of sample `smp`.  The sample id is uniform over the workgroup but comes from the vector ALU when sample_of
// divides: through readfirstlane, so that the index entry and the row are scalar loads.  No bounds check, no clamp.
template <bool PER_SAMPLE>
__device__ __forceinline__ const skr_step_row* guided_row(const RowRef& r, uint32_t smp) {
  if constexpr (PER_SAMPLE) return r.rows + (r.index[__builtin_amdgcn_readfirstlane(smp)] + r.row_offset);
  else return row_of(r);
}

template <typename T, int K, bool NOISE, RowForm F>
__global__ __launch_bounds__(BLOCK) void guided_rows_kernel_v1(const GuidedRowArgs<guided_kmax(K)> a) {
  static_assert(row_behind_loads(F), "the guided launch has the two row forms that read their row behind the loads");
  constexpr bool TILE = sizeof(T) == 4;  // whole chunks are whole tiles: 32-bit tensors take the whole-line layout, as in guided_kernel_v1
  constexpr bool PER_SAMPLE = F == RowForm::PerSample;
  const uint32_t c = chunk_of(blockIdx.x, a.xmap_lr);
  const int64_t v = (int64_t)c * BLOCK + threadIdx.x;
  Raw<T> raw[K];
#pragma unroll
  for (int j = 0; j < K; ++j) raw[j] = load_raw<T, TILE>(a.in[j], v);
  Raw<T> rc = load_raw<T, TILE>(a.cond, v);
  __builtin_amdgcn_sched_barrier(0);  // every load is out before the first scalar of the arithmetic (the index entry, the row) is fetched
  [[maybe_unused]] uint32_t smp = 0, within = 0;
  if constexpr (NOISE || PER_SAMPLE) sample_of(c, a.bps_shift, smp, within);
  const skr_step_row* row = guided_row<PER_SAMPLE>(a.tab, smp);
  // (a row's doubles stay in SGPRs and are narrowed where they are used, as in masked_kernel_v1's table forms)
  double c0[K];
#pragma unroll
  for (int j = 0; j < K; ++j) c0[j] = row->coef0[j];
  const float zeta0 = (float)row->zeta0, g = (float)row->convert_k[0];
  const int32_t slot = a.slot;
  float z[VEC];
  [[maybe_unused]] bool n0 = false;
  if constexpr (NOISE) {
    n0 = zeta0 != 0.f;
    if (n0) {
      const uint64_t stream0 = row->stream0;
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
  if constexpr (NOISE) { if (n0) fma_noise8<float>(zeta0, z, s); }
  store8<T, float, TILE>(a.out, v, s);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// dtype x noise x form x operand count to the instantiation, and its kernarg
static void launch_guided_rows_v1(const skr_step_plan& p, const void* const* inputs, void* out, const skr_step_guidance& gd, const uint64_t* seeds,
                                  const GuidedLaunch& l, bool per_sample, const RowRef& tab, hipStream_t s) {
  with_step_type<false>(p.dtype_a, [&](auto tt) {
    with_bools([&](auto nz, auto ps) {
      with_count<1, SKR_ROW_TERMS>(p.n_terms, [&](auto n) {
        using T = typename decltype(tt)::type;
        constexpr int N = decltype(n)::value, KMAX = guided_kmax(N);
        constexpr RowForm F = decltype(ps)::value ? RowForm::PerSample : RowForm::WholeBatch;
        GuidedRowArgs<KMAX> a;
        for (int k = 0; k < KMAX; ++k) a.in[k] = k < N ? inputs[k] : nullptr;
        a.cond = gd.cond; a.out = out; a.guided = gd.guided_out; a.seeds = seeds;
        a.xmap_lr = xmap_lr_for(l.chunks); a.bps_shift = l.bps_shift;
        a.tab = tab; a.slot = gd.slot;
        hipLaunchKernelGGL((guided_rows_kernel_v1<T, N, decltype(nz)::value, F>), dim3((unsigned)l.chunks), dim3(BLOCK), 0, s, a);
      });
    }, l.noise, per_sample);
  });
}

// The two entries: skr_step_launch_guided's checks in its order and with its codes (guided_prepare), and on top of them the rows'.
static int guided_rows_launch_impl(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide, const uint64_t* seeds_dev,
                                   int64_t numel, void* stream, bool per_sample, const skr_step_row* rows, const int32_t* index, int32_t row_offset) {
  if (!plan || !guide || !rows || (per_sample && !index)) return SKR_ERR_NULL;
  const skr_step_plan& p = *plan;
  GuidedLaunch l;
  if (const int rc = guided_prepare(p, *guide, inputs, out, seeds_dev, numel, true, &l)) return rc;
  if (numel == 0) return SKR_OK;
  if (!l.one_trip || row_offset < 0) return SKR_ERR_UNSUPPORTED;
  if (per_sample) {  // a workgroup lies inside one sample, with or without noise
    constexpr int64_t CHUNK = (int64_t)BLOCK * VEC;
    if (p.sample_numel <= 0 || numel % p.sample_numel != 0) return SKR_ERR_SHAPE;
    if (p.sample_numel % CHUNK != 0 || p.sample_numel >= (1ll << 31)) return SKR_ERR_UNSUPPORTED;
    l.bps_shift = bps_shift_of(p.sample_numel / CHUNK);
  }
  DeviceGuard device_guard(out);
  launch_guided_rows_v1(p, inputs, out, *guide, seeds_dev, l, per_sample, RowRef{rows, index, row_offset}, reinterpret_cast<hipStream_t>(stream));
  return finish_launch();
}

}  // namespace skr

extern "C" int skr_step_launch_guided_indexed(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                              const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev, const int32_t* index_dev,
                                              int32_t row_offset, void* stream) {
  return skr::guided_rows_launch_impl(plan, inputs, out, guide, seeds_dev, numel, stream, false, rows_dev, index_dev, row_offset);
}

extern "C" int skr_step_launch_guided_indexed_per_sample(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                                         const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev,
                                                         const int32_t* sample_index_dev, int32_t row_offset, void* stream) {
  return skr::guided_rows_launch_impl(plan, inputs, out, guide, seeds_dev, numel, stream, true, rows_dev, sample_index_dev, row_offset);
}
