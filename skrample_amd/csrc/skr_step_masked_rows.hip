// The masked solver step with device-resident scalars (include/skrample_hip.h, skr_step_launch_masked_indexed and
// skr_step_launch_masked_indexed_per_sample): masked_kernel_v1 of skr_step_masked.hip reading coef0 / coef1 / zeta0 / stream0 from a
// skr_step_row when it runs, so that a captured in-painting loop serves any schedule of its length.
//
//   * one kernel family, masked_rows_kernel_v1<T, K, NOISE, PER_SAMPLE>: lane ownership, XCD chunk map, loads, mask index, Philox block
//     numbering, operation order and the one rounding are masked_kernel_v1's; a launch is bit for bit what skr_step_launch_masked gives with
//     the row's values in its plan.  Every operand load and the mask load are issued first; the row (whole batch: rows[index[0] + offset];
//     per sample: rows[index[sample] + offset], the sample id through readfirstlane) is fetched behind them, two dependent scalar loads
//     where the kernarg form reads its coefficients.  No address depends on the row.
//   * a NOISE instantiation serves every row: a row whose zeta0 narrows to zero skips the draw (a uniform branch), as the other row forms do.
//   * a translation unit of its own: the kernels of skr_step_masked.hip keep their symbols and their instruction streams.
// There is no grid-stride row form: what the one-trip kernel does not cover is SKR_ERR_UNSUPPORTED.
#include "skr_step_masked.h"
#include "skr_device.h"

namespace skr {

// Kernarg of the row forms: MaskedArgs without the scalars a row carries (two 64-byte lines up to 4 operands, as there).
template <int KMAX>
struct MaskedRowArgs {
  const void* in[KMAX];
  const void* mask;
  void* out;
  int32_t xmap_lr;
  int32_t bps_shift;
  uint32_t mask_numel;
  uint32_t mask_stride;
  const uint64_t* seeds;
  RowRef tab;
};

// The row of a workgroup of sample `smp`.  The sample id is uniform over the workgroup but comes from the vector ALU when chunk_sample
// divides: through readfirstlane, so that the index entry and the row are scalar loads.  No bounds check, no clamp.
template <bool PER_SAMPLE>
__device__ __forceinline__ const skr_step_row* masked_row(const RowRef& r, uint32_t smp) {
  if constexpr (PER_SAMPLE) return r.rows + (r.index[__builtin_amdgcn_readfirstlane(smp)] + r.row_offset);
  else return row_of(r);
}

template <typename T, int K, bool NOISE, bool PER_SAMPLE>
__global__ __launch_bounds__(BLOCK) void masked_rows_kernel_v1(const MaskedRowArgs<masked_kmax(K)> a) {
  constexpr bool TILE = sizeof(T) == 4;
  const uint32_t c = chunk_of(blockIdx.x, a.xmap_lr);
  const int64_t v = (int64_t)c * BLOCK + threadIdx.x;
  Raw<T> raw[K];
#pragma unroll
  for (int j = 0; j < K; ++j) raw[j] = load_raw<T, TILE>(a.in[j], v);
  uint32_t smp, within;
  chunk_sample(c, a.bps_shift, smp, within);
  const uint32_t vs = within * BLOCK + threadIdx.x;  // lane-vector within the sample
  const uint32_t e0 = 4u * (uint32_t)group0<TILE>((int64_t)vs);
  const uint32_t m0 = e0 % a.mask_numel;
  uint32_t m1 = m0 + 4u;
  if constexpr (TILE) m1 = (4u * (uint32_t)group1<TILE>((int64_t)vs)) % a.mask_numel;
  const int64_t mbase = (int64_t)smp * a.mask_stride;
  Raw<T> rm = load_mask8<T>(a.mask, mbase + m0, mbase + m1);
  __builtin_amdgcn_sched_barrier(0);  // every load is out before the index entry and the row are fetched
  const skr_step_row* row = masked_row<PER_SAMPLE>(a.tab, smp);
  // (the doubles stay in SGPRs and are narrowed where they are used: as floats they would be 2 K VGPRs live across the Philox rounds)
  double cd0[K], cd1[K];
#pragma unroll
  for (int j = 0; j < K; ++j) { cd0[j] = row->coef0[j]; cd1[j] = row->coef1[j]; }
  const float zeta0 = (float)row->zeta0;
  float z[VEC];
  bool n0 = false;
  if constexpr (NOISE) {
    n0 = zeta0 != 0.f;
    if (n0) {  // (uniform) a zero row skips the draw, as a launch without noise does
      const uint64_t stream0 = row->stream0;
      const uint64_t seed = a.seeds[smp];
      normal4(seed, stream0, (uint64_t)group0<TILE>((int64_t)vs), z);
      normal4(seed, stream0, (uint64_t)group1<TILE>((int64_t)vs), z + 4);
    }
  }
  float s[VEC], kn[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) { s[i] = 0.f; kn[i] = 0.f; }
#pragma unroll
  for (int j = 0; j < K; ++j) {
    float w[VEC];
    widen<T, float>(raw[j], w);
    const float w0 = (float)cd0[j], w1 = (float)cd1[j];
#pragma unroll
    for (int i = 0; i < VEC; ++i) s[i] = fma_(w0, w[i], s[i]);
    if (w1 != 0.f) {  // (uniform: the row's) an operand absent from the known form adds nothing to it, not even 0 * x
#pragma unroll
      for (int i = 0; i < VEC; ++i) kn[i] = fma_(w1, w[i], kn[i]);
    }
  }
  if constexpr (NOISE) { if (n0) fma_noise8<float>(zeta0, z, s); }
  float m[VEC], o[VEC];
  widen<T, float>(rm, m);
#pragma unroll
  for (int i = 0; i < VEC; ++i) o[i] = fma_(m[i], s[i], mul_(sub_(1.f, m[i]), kn[i]));
  store8<T, float, TILE>(a.out, v, o);
}

template <typename T, bool NOISE, bool PER_SAMPLE>
static void launch_masked_rows(const skr_step_plan& p, const void* const* inputs, void* out, const skr_step_mask& mk, const uint64_t* seeds,
                               const MaskedLaunch& l, const RowRef& tab, hipStream_t s) {
  with_count<1, SKR_ROW_TERMS>(p.n_terms, [&](auto n) {
    constexpr int N = decltype(n)::value;
    MaskedRowArgs<masked_kmax(N)> a;
    for (int k = 0; k < masked_kmax(N); ++k) a.in[k] = k < N ? inputs[k] : nullptr;
    a.mask = mk.mask; a.out = out; a.seeds = seeds;
    a.xmap_lr = xmap_lr_for(l.chunks); a.bps_shift = l.bps_shift;
    a.mask_numel = (uint32_t)mk.mask_numel; a.mask_stride = (uint32_t)mk.batch_stride;
    a.tab = tab;
    hipLaunchKernelGGL((masked_rows_kernel_v1<T, N, NOISE, PER_SAMPLE>), dim3((unsigned)l.chunks), dim3(BLOCK), 0, s, a);
  });
}

static int masked_rows_impl(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_mask* mask, const uint64_t* seeds_dev,
                            int64_t numel, const skr_step_row* rows, const int32_t* index, int32_t row_offset, bool per_sample, void* stream) {
  if (!plan || !mask || !rows || (per_sample && !index)) return SKR_ERR_NULL;
  MaskedLaunch l;
  if (const int rc = masked_prepare(*plan, *mask, inputs, out, seeds_dev, numel, true, &l)) return rc;
  if (numel == 0) return SKR_OK;
  if (!l.one_trip || row_offset < 0) return SKR_ERR_UNSUPPORTED;
  DeviceGuard device_guard(out);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const RowRef tab{rows, index, row_offset};
  with_step_type<false>(plan->dtype_a, [&](auto tt) {
    with_bools([&](auto nz, auto ps) {
      launch_masked_rows<typename decltype(tt)::type, decltype(nz)::value, decltype(ps)::value>(*plan, inputs, out, *mask, seeds_dev, l, tab, s);
    }, l.noise, per_sample);
  });
  return finish_launch();
}

}  // namespace skr

extern "C" int skr_step_launch_masked_indexed(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_mask* mask,
                                              const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev,
                                              const int32_t* index_dev, int32_t row_offset, void* stream) {
  return skr::masked_rows_impl(plan, inputs, out, mask, seeds_dev, numel, rows_dev, index_dev, row_offset, false, stream);
}

extern "C" int skr_step_launch_masked_indexed_per_sample(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_mask* mask,
                                                         const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev,
                                                         const int32_t* sample_index_dev, int32_t row_offset, void* stream) {
  return skr::masked_rows_impl(plan, inputs, out, mask, seeds_dev, numel, rows_dev, sample_index_dev, row_offset, true, stream);
}
