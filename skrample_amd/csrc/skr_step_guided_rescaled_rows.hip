// The rescaled guided solver step with device-resident scalars (include/skrample_hip.h, skr_step_launch_guided_rescaled_indexed[_per_sample]):
// guided_rows_kernel_v1 (skr_step_guided_rows.hip) whose guided value is diffusers' rescale_noise_cfg of it when the row rescales, under
// the row's own phi -- convert_k[1] -- and the sample's factor r = factor_dev[s], what the statistics row launch wrote for it
// (skr_guidance_stats_rows.hip).  A captured classifier-free-guidance loop then serves any schedule, any guidance scale AND any
// guidance_rescale, zero included.
//
//   p   = rn_T( u + rn_T( g * rn_T(c - u) ) )       u = inputs[slot], c = cond;  g = (float)row.convert_k[0]
//   p'  = rn_T( rn_T(phi * rn_T(p * r)) + rn_T(psi * p) )   phi = (float)row.convert_k[1], psi = (float)(1.0 - row.convert_k[1]): the row's phi not +-0
//   p'  = p                                                  the row's phi exactly +-0: factor_dev[s] is NOT read (it may hold NaN)
//   out = sum_k c0[k]*v_k + zeta0*N(stream0)        v_slot = p', v_k = in_k otherwise;  c0 / zeta0 / stream0 from the row
//   guided_out = p'                                 (when asked for)
//
// One kernel template, guided_rescaled_rows_kernel_v1<T, K, NOISE, RowForm>, for the two forms whose row is read behind the loads:
//   WholeBatch  skr_step_launch_guided_rescaled_indexed              rows[index[0] + row_offset]
//   PerSample   skr_step_launch_guided_rescaled_indexed_per_sample   rows[index[sample] + row_offset], one entry per sample
// Statement order, lane ownership, XCD chunk map, Philox block numbering and the fp32 tile layout are guided_rows_kernel_v1's: every
// operand load and the cond load first, the index entry and the row as scalar loads behind them, the row's doubles in SGPRs, `slot` a
// kernarg scalar compared per unrolled operand.  Every operand takes its fma, zero coefficients included: there is no absent operand and
// no inactive sample here.  Whether the row rescales is a real branch, uniform over the workgroup (a scalar one, exec never masked), not
// arithmetic -- the lone step_guided(..., guidance_rescale=0.0) is the unrescaled launch, and 0 * inf would otherwise leak through -- and
// the factor's load sits inside it, so an unrescaled row never touches the factor.  A workgroup lies inside one sample in both forms (the
// factor is per sample), so both take the sample number from the chunk.  guided_value and rescaled_value are the shared ones
// (skr_step_guided.h): a rescaled row has the bits of skr_step_launch_guided_rescaled, an unrescaled one those of
// skr_step_launch_guided_indexed[_per_sample].  There is no grid-stride form.
#include "skr_step_guided.h"
#include "skr_device.h"

namespace skr {

// Kernarg: GuidedRowArgs (skr_step_guided_rows.hip) with the factor.  What the first instructions need (operand pointers, chunk map) leads.
template <int KMAX>
struct GuidedRescaledRowArgs {
  const void* in[KMAX];
  const void* cond;
  void* out;
  void* guided;         // nullptr: p' is not stored
  int32_t xmap_lr;      // log2(run length) of the XCD chunk map
  int32_t bps_shift;    // chunks per sample: log2 when >= 0, minus the count otherwise (see sample_of); read by every instantiation
  const uint64_t* seeds;
  const void* factor;   // T[samples]: read when the row rescales
  RowRef tab;
  int32_t slot;         // the operand that p' replaces in the sum
};

// `p` as a pointer into the constant address space: device memory no kernel of the launch writes, read by scalar loads from a uniform address
template <typename P>
__device__ __forceinline__ auto uniform(const P* p) {
  return (const __attribute__((address_space(4))) P*)p;
}

// the value of a 16-bit element given as its bits: what load_scalar<T> makes of it
template <typename T>
__device__ __forceinline__ float widen_bits(uint16_t b) {
  if constexpr (std::is_same<T, bf16_t>::value) return __uint_as_float((uint32_t)b << 16);
  else return (float)__builtin_bit_cast(_Float16, b);
}

template <typename T, int K, bool NOISE, RowForm F>
__global__ __launch_bounds__(BLOCK) void guided_rescaled_rows_kernel_v1(const GuidedRescaledRowArgs<guided_kmax(K)> a) {
  static_assert(row_behind_loads(F), "the rescaled guided row launch has the two row forms that read their row behind the loads");
  constexpr bool TILE = sizeof(T) == 4;  // whole chunks are whole tiles, as in guided_rows_kernel_v1
  constexpr bool PER_SAMPLE = F == RowForm::PerSample;
  const uint32_t c = chunk_of(blockIdx.x, a.xmap_lr);
  const int64_t v = (int64_t)c * BLOCK + threadIdx.x;
  Raw<T> raw[K];
#pragma unroll
  for (int j = 0; j < K; ++j) raw[j] = load_raw<T, TILE>(a.in[j], v);
  Raw<T> rc = load_raw<T, TILE>(a.cond, v);
  // Every load is out before the first scalar of the arithmetic (the index entry, the row) is fetched.  The scheduling barrier holds
  // inside this basic block only, and the branches below (sample_of's, the phi test, the draw) would otherwise let the compiler sink the
  // loads to their first use -- behind the row's round trips and the factor's: the empty statement that may write memory keeps them here.
  // What is read behind it is read-only for the launch and read through the constant address space, so that it stays scalar loads.
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  uint32_t smp, within;
  sample_of(c, a.bps_shift, smp, within);
  smp = __builtin_amdgcn_readfirstlane(smp);  // (uniform over the workgroup) the index entry, the row, the seed and a 32-bit factor are scalar loads
  int32_t at = 0;
  if constexpr (PER_SAMPLE) at = uniform(a.tab.index)[smp];
  else if (a.tab.index != nullptr) at = uniform(a.tab.index)[0];
  const auto row = uniform(a.tab.rows + (at + a.tab.row_offset));
  // (a row's doubles stay in SGPRs and are narrowed where they are used, as in guided_rows_kernel_v1)
  double c0[K];
#pragma unroll
  for (int j = 0; j < K; ++j) c0[j] = row->coef0[j];
  const float zeta0 = (float)row->zeta0, g = (float)row->convert_k[0];
  const double phi_d = row->convert_k[1];
  const bool rescales = (__builtin_bit_cast(uint64_t, phi_d) << 1) != 0;  // (uniform) phi is not +-0
  const int32_t slot = a.slot;
  float r = 0.f, phi = 0.f, psi = 0.f;
  [[maybe_unused]] uint16_t r16 = 0;
  if (rescales) {  // one uniform load behind the operand loads; an unrescaled row's factor is never touched
    if constexpr (TILE) r = uniform(reinterpret_cast<const float*>(a.factor))[smp];
    else r16 = reinterpret_cast<const uint16_t*>(a.factor)[smp];  // (a 16-bit value has no scalar load; widened where it is used, so that nothing waits for it here)
    phi = (float)phi_d;
    psi = (float)sub_(1.0, phi_d);  // 1 - phi formed in double, narrowed once
  }
  float z[VEC];
  [[maybe_unused]] bool n0 = false;
  if constexpr (NOISE) {
    n0 = zeta0 != 0.f;
    if (n0) {
      const uint64_t stream0 = row->stream0;
      const uint32_t vs = within * BLOCK + threadIdx.x;  // lane-vector within the sample (sample_numel < 2^31)
      const uint64_t seed = uniform(a.seeds)[smp];
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
      if (rescales) {  // (uniform: the row's) a real branch: p' = p otherwise
        if constexpr (!TILE) {
          uint32_t bits = r16;
          asm volatile("" : "+v"(bits));  // (the widening stays here: hoisted into the branch of the load it would wait for every load in flight)
          r = widen_bits<T>((uint16_t)bits);
        }
#pragma unroll
        for (int i = 0; i < VEC; ++i) w[i] = rescaled_value<T>(w[i], r, phi, psi);
      }
      if (a.guided != nullptr) store8<T, float, TILE>(a.guided, v, w);  // (p' is a value of T: the store's rounding is exact)
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
static void launch_guided_rescaled_rows_v1(const skr_step_plan& p, const void* const* inputs, void* out, const skr_step_guidance& gd, const skr_step_rescale& rs,
                                           const uint64_t* seeds, const GuidedLaunch& l, bool per_sample, const RowRef& tab, hipStream_t s) {
  with_step_type<false>(p.dtype_a, [&](auto tt) {
    with_bools([&](auto nz, auto ps) {
      with_count<1, SKR_ROW_TERMS>(p.n_terms, [&](auto n) {
        using T = typename decltype(tt)::type;
        constexpr int N = decltype(n)::value, KMAX = guided_kmax(N);
        constexpr RowForm F = decltype(ps)::value ? RowForm::PerSample : RowForm::WholeBatch;
        GuidedRescaledRowArgs<KMAX> a;
        for (int k = 0; k < KMAX; ++k) a.in[k] = k < N ? inputs[k] : nullptr;
        a.cond = gd.cond; a.out = out; a.guided = gd.guided_out; a.seeds = seeds; a.factor = rs.factor_dev;
        a.xmap_lr = xmap_lr_for(l.chunks); a.bps_shift = l.bps_shift;
        a.tab = tab; a.slot = gd.slot;
        hipLaunchKernelGGL((guided_rescaled_rows_kernel_v1<T, N, decltype(nz)::value, F>), dim3((unsigned)l.chunks), dim3(BLOCK), 0, s, a);
      });
    }, l.noise, per_sample);
  });
}

// The two entries: the checks of skr_step_launch_guided_indexed[_per_sample], in their order and with their codes, and what
// skr_step_launch_guided_rescaled adds where skr_step_launch_guided_rescaled_rolling puts it (guided_prepare, skr_step_guided.hip).
static int guided_rescaled_rows_launch_impl(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide, const skr_step_rescale* rescale,
                                            const uint64_t* seeds_dev, int64_t numel, void* stream, bool per_sample, const skr_step_row* rows, const int32_t* index,
                                            int32_t row_offset) {
  if (!plan || !guide || !rescale || !rows || (per_sample && !index)) return SKR_ERR_NULL;
  const skr_step_plan& p = *plan;
  GuidedLaunch l;
  if (const int rc = guided_prepare(p, *guide, inputs, out, seeds_dev, numel, true, &l, rescale)) return rc;
  if (numel == 0) return SKR_OK;
  if (!l.one_trip || row_offset < 0) return SKR_ERR_UNSUPPORTED;
  // a workgroup lies inside one sample, with or without noise and in both forms, and that sample is the statistic's
  constexpr int64_t CHUNK = (int64_t)BLOCK * VEC;
  if (p.sample_numel <= 0 || numel % p.sample_numel != 0 || rescale->sample_numel != p.sample_numel) return SKR_ERR_SHAPE;
  if (p.sample_numel % CHUNK != 0 || p.sample_numel >= (1ll << 31)) return SKR_ERR_UNSUPPORTED;
  l.bps_shift = bps_shift_of(p.sample_numel / CHUNK);
  DeviceGuard device_guard(out);
  launch_guided_rescaled_rows_v1(p, inputs, out, *guide, *rescale, seeds_dev, l, per_sample, RowRef{rows, index, row_offset}, reinterpret_cast<hipStream_t>(stream));
  return finish_launch();
}

}  // namespace skr

extern "C" int skr_step_launch_guided_rescaled_indexed(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                                       const skr_step_rescale* rescale, const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev,
                                                       const int32_t* index_dev, int32_t row_offset, void* stream) {
  return skr::guided_rescaled_rows_launch_impl(plan, inputs, out, guide, rescale, seeds_dev, numel, stream, false, rows_dev, index_dev, row_offset);
}

extern "C" int skr_step_launch_guided_rescaled_indexed_per_sample(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                                                  const skr_step_rescale* rescale, const uint64_t* seeds_dev, int64_t numel,
                                                                  const skr_step_row* rows_dev, const int32_t* sample_index_dev, int32_t row_offset, void* stream) {
  return skr::guided_rescaled_rows_launch_impl(plan, inputs, out, guide, rescale, seeds_dev, numel, stream, true, rows_dev, sample_index_dev, row_offset);
}
