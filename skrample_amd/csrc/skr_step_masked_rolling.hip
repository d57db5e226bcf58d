// The masked solver step of a rolling batch (include/skrample_hip.h, skr_step_launch_masked_rolling): the per-sample row form of
// skr_step_masked_rows.hip with the three semantics Rolling<T> gave the plain step kernels (skr_step_fast.hip), so that in-painting
// requests sit in the slots of a rolling.RollingBatch beside each other and beside plain requests.
//
//   * one kernel family, masked_rolling_kernel_v1<T, K, NOISE>: lane ownership, XCD chunk map, loads, mask index, Philox keying and block
//     numbering, operation order and the one rounding are masked_kernel_v1's.  A workgroup first asks its own sample's index entry and
//     row what to touch -- the row fetch stands IN FRONT of the loads here, as in Rolling<T>'s step_kernel_k1 branch, two dependent
//     scalar round trips per wave:
//       inactive sample   a negative index entry (tested before row_offset is added) ends the workgroup before its first vector-memory
//                         instruction: no operand, mask, seed or row is read, `out` keeps its bytes;
//       absent operand    coef0[k] and coef1[k] both exactly zero (either sign) in the row: neither loaded nor accumulated into either
//                         form (history a request in its ramp-up does not have yet; `noise` on the last step; `original` / `noise` of
//                         a plain request sharing the batch).  Its bytes may be NaN or inf;
//       operand order     the present operands are summed in slot order, one fma each into s (a present operand whose coef0 is zero
//                         included, as in the lone launch) and one into k where its coef1 is not exactly zero: the bits of the
//                         narrower skr_step_launch_masked that holds exactly these operands.
//     The row is uniform over the workgroup (the sample id goes through readfirstlane, the index entry and the row are scalar loads), so
//     every such decision is a scalar branch; the row's doubles stay in SGPRs and are narrowed where they are used.
//   * the mask is always read for an active sample; a NOISE instantiation serves every row (a row whose zeta0 narrows to zero skips the draw).
//   * rolling_row / row_has of skr_step_fast.hip are restated here (masked_rolling_row / masked_row_has), and the translation unit is
//     its own: every existing kernel keeps its symbol and its instruction stream.
// There is no grid-stride form: what the one-trip kernel does not cover is SKR_ERR_UNSUPPORTED.
#include "skr_step_masked.h"
#include "skr_device.h"

namespace skr {

// Kernarg: that of the masked row forms (MaskedRowArgs of skr_step_masked_rows.hip).
template <int KMAX>
struct MaskedRollingArgs {
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

// The row of chunk c's sample, or nullptr for an inactive sample (index entry < 0, tested before row_offset is added).  The sample id
// goes through readfirstlane (the dividing form of chunk_sample runs on the vector ALU) so that the index entry and the row are scalar
// loads.  No bounds check, no clamp.
__device__ __forceinline__ const skr_step_row* masked_rolling_row(const RowRef& r, uint32_t c, int32_t bps_shift, uint32_t& smp, uint32_t& within) {
  chunk_sample(c, bps_shift, smp, within);
  smp = __builtin_amdgcn_readfirstlane(smp);
  const int32_t at = r.index[smp];
  return at < 0 ? nullptr : r.rows + (at + r.row_offset);
}
// an operand is present unless both of its coefficients are exactly zero (either sign): decided on the row's doubles, in SGPRs
__device__ __forceinline__ bool masked_row_has(const skr_step_row* row, int j) {
  return ((__builtin_bit_cast(uint64_t, row->coef0[j]) | __builtin_bit_cast(uint64_t, row->coef1[j])) << 1) != 0;
}

template <typename T, int K, bool NOISE>
__global__ __launch_bounds__(BLOCK) void masked_rolling_kernel_v1(const MaskedRollingArgs<masked_kmax(K)> a) {
  constexpr bool TILE = sizeof(T) == 4;
  const uint32_t c = chunk_of(blockIdx.x, a.xmap_lr);
  const int64_t v = (int64_t)c * BLOCK + threadIdx.x;
  uint32_t smp, within;
  const skr_step_row* row = masked_rolling_row(a.tab, c, a.bps_shift, smp, within);
  if (row == nullptr) return;  // inactive sample: nothing read, nothing written
  bool on[K];
  double cd0[K], cd1[K];  // (narrowed where they are used: the doubles sit in SGPRs, the floats would be 2 K VGPRs live across the loads)
#pragma unroll
  for (int j = 0; j < K; ++j) { on[j] = masked_row_has(row, j); cd0[j] = row->coef0[j]; cd1[j] = row->coef1[j]; }
  const float zeta0 = (float)row->zeta0;
  const uint64_t stream0 = row->stream0;
  // (each operand's pointer is fetched from the kernarg inside its branch, as in step_kernel_k1's rolling form)
  Raw<T> raw[K];
#pragma unroll
  for (int j = 0; j < K; ++j) if (on[j]) raw[j] = load_raw<T, TILE>(a.in[j], v);
  // the mask index of masked_kernel_v1: it belongs to the lane-vector within the sample
  const uint32_t vs = within * BLOCK + threadIdx.x;
  const uint32_t e0 = 4u * (uint32_t)group0<TILE>((int64_t)vs);
  const uint32_t m0 = e0 % a.mask_numel;
  uint32_t m1 = m0 + 4u;
  if constexpr (TILE) m1 = (4u * (uint32_t)group1<TILE>((int64_t)vs)) % a.mask_numel;
  const int64_t mbase = (int64_t)smp * a.mask_stride;
  Raw<T> rm = load_mask8<T>(a.mask, mbase + m0, mbase + m1);
  float z[VEC];
  bool n0 = false;
  if constexpr (NOISE) {
    n0 = zeta0 != 0.f;
    if (n0) {  // (uniform) a zero row skips the draw, as a launch without noise does
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
    if (on[j]) {  // (uniform: the row's) present operands in slot order: the bits of the narrower launch that holds exactly these
      float w[VEC];
      widen<T, float>(raw[j], w);
      const float w0 = (float)cd0[j], w1 = (float)cd1[j];
#pragma unroll
      for (int i = 0; i < VEC; ++i) s[i] = fma_(w0, w[i], s[i]);
      if (w1 != 0.f) {  // (uniform) an operand absent from the known form adds nothing to it, not even 0 * x
#pragma unroll
        for (int i = 0; i < VEC; ++i) kn[i] = fma_(w1, w[i], kn[i]);
      }
    }
  }
  if constexpr (NOISE) { if (n0) fma_noise8<float>(zeta0, z, s); }
  float m[VEC], o[VEC];
  widen<T, float>(rm, m);
#pragma unroll
  for (int i = 0; i < VEC; ++i) o[i] = fma_(m[i], s[i], mul_(sub_(1.f, m[i]), kn[i]));
  store8<T, float, TILE>(a.out, v, o);
}

template <typename T, bool NOISE>
static void launch_masked_rolling(const skr_step_plan& p, const void* const* inputs, void* out, const skr_step_mask& mk, const uint64_t* seeds,
                                  const MaskedLaunch& l, const RowRef& tab, hipStream_t s) {
  with_count<1, SKR_ROW_TERMS>(p.n_terms, [&](auto n) {
    constexpr int N = decltype(n)::value;
    MaskedRollingArgs<masked_kmax(N)> a;
    for (int k = 0; k < masked_kmax(N); ++k) a.in[k] = k < N ? inputs[k] : nullptr;
    a.mask = mk.mask; a.out = out; a.seeds = seeds;
    a.xmap_lr = xmap_lr_for(l.chunks); a.bps_shift = l.bps_shift;
    a.mask_numel = (uint32_t)mk.mask_numel; a.mask_stride = (uint32_t)mk.batch_stride;
    a.tab = tab;
    hipLaunchKernelGGL((masked_rolling_kernel_v1<T, N, NOISE>), dim3((unsigned)l.chunks), dim3(BLOCK), 0, s, a);
  });
}

}  // namespace skr

extern "C" int skr_step_launch_masked_rolling(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_mask* mask,
                                              const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev,
                                              const int32_t* sample_index_dev, int32_t row_offset, void* stream) {
  using namespace skr;
  if (!plan || !mask || !rows_dev || !sample_index_dev) return SKR_ERR_NULL;
  MaskedLaunch l;
  if (const int rc = masked_prepare(*plan, *mask, inputs, out, seeds_dev, numel, true, &l)) return rc;
  if (numel == 0) return SKR_OK;
  if (!l.one_trip || row_offset < 0) return SKR_ERR_UNSUPPORTED;
  DeviceGuard device_guard(out);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const RowRef tab{rows_dev, sample_index_dev, row_offset};
  with_step_type<false>(plan->dtype_a, [&](auto tt) {
    with_bools([&](auto nz) {
      launch_masked_rolling<typename decltype(tt)::type, decltype(nz)::value>(*plan, inputs, out, *mask, seeds_dev, l, tab, s);
    }, l.noise);
  });
  return finish_launch();
}
