// The masked solver step (include/skrample_hip.h, skr_step_launch_masked): the in-painting blend fused into the step launch.
//
//   s = sum_k c0[k]*in_k + zeta0*N(stream0)      the solver step, accumulated exactly as skr_step_launch accumulates it
//   k = sum_k c1[k]*in_k                         the re-noised known region, over the operands whose c1 is not exactly zero
//   out = fma(m, s, (1 - m) * k)                 one pass over HBM, one store, one rounding (store8's)
//
//   * one-trip kernel (masked_kernel_v1<T, K, NOISE, RowForm>): whole 2048-element chunks, samples made of whole chunks, operands / mask / output of one
//     16- or 32-bit dtype, fp32 arithmetic, <= 16 operands, mask_numel % 8 == 0.  Lane ownership, XCD chunk map, loads, stores and
//     Philox block numbering are those of step_kernel_k1's unpaced form (skr_step_fast.hip): every operand load is issued first, the
//     mask vector right behind them, the scalars and the Philox rounds while they are in flight.
//   * general kernel (masked_kernel_gen): grid-stride, one element per lane and trip, any size, any dtype combination skr_step_launch
//     takes, fp32 or fp64 arithmetic.
// Both evaluate the same operations in the same order on every element, so they agree bit for bit where both apply.
//
// Four entries, one template.  RowForm (skr_step_common.h) says where a launch's scalars come from, as for the plain step:
//   Kernarg     skr_step_launch_masked                      coef0 / coef1 / zeta0 / stream0 from the plan, narrowed on the host
//   WholeBatch  skr_step_launch_masked_indexed              from rows[index[0] + row_offset], read by the kernel behind its loads, so that a
//   PerSample   skr_step_launch_masked_indexed_per_sample   captured in-painting loop serves any schedule; per sample: rows[index[sample] + row_offset]
//   Rolling     skr_step_launch_masked_rolling              per-sample rows with the three semantics of step_kernel_k1's Rolling form (skr_step_fast.hip), for the
//                                                           slots of a rolling.RollingBatch: the row fetch stands IN FRONT of the loads,
//       inactive sample   a negative index entry (tested before row_offset is added) ends the workgroup before its first vector-memory
//                         instruction: no operand, mask, seed or row is read, `out` keeps its bytes;
//       absent operand    coef0[k] and coef1[k] both exactly zero (either sign) in the row: neither loaded nor accumulated into either
//                         form (history a request in its ramp-up does not have yet; `noise` on the last step; `original` / `noise` of
//                         a plain request sharing the batch).  Its bytes may be NaN or inf;
//       operand order     the present operands are summed in slot order, one fma each into s (a present operand whose coef0 is zero
//                         included, as in the lone launch) and one into k where its coef1 is not exactly zero: the bits of the
//                         narrower skr_step_launch_masked that holds exactly these operands.
// A row launch is bit for bit what skr_step_launch_masked gives with the row's values in its plan.  A row is uniform over the workgroup
// (the sample id goes through readfirstlane, the index entry and the row are scalar loads), so every decision taken from it is a scalar
// branch; the mask is always read for an active sample.  The row forms have no grid-stride kernel: what the one-trip kernel does not
// cover is SKR_ERR_UNSUPPORTED.
#include "skr_step_masked.h"
#include "skr_device.h"

namespace skr {

constexpr int masked_kmax(int k) { return k <= 4 ? 4 : (k <= 8 ? 8 : (k <= 12 ? 12 : 16)); }

// Kernarg of the one-trip kernel: what the first instructions need (operand pointers, chunk map) leads, as in OneTripArgs.
template <int KMAX>
struct MaskedArgs {
  const void* in[KMAX];
  const void* mask;
  void* out;
  int32_t xmap_lr;      // log2(run length) of the XCD chunk map
  int32_t bps_shift;    // chunks per sample: log2 when >= 0, minus the count otherwise (see sample_of)
  uint32_t mask_numel;  // elements of one sample's mask (a multiple of 8, below 2^31)
  uint32_t mask_stride; // elements between the masks of two samples: mask_numel or 0
  const uint64_t* seeds;
  uint64_t stream0;
  float zeta0;
  float c0[KMAX];
  float c1[KMAX];
};
// Kernarg of the three row forms: MaskedArgs without the scalars a row carries (two 64-byte lines up to 4 operands, as there).
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
template <RowForm F, int KMAX> using MaskedArgsOf = std::conditional_t<has_table(F), MaskedRowArgs<KMAX>, MaskedArgs<KMAX>>;

// The row of a workgroup of sample `smp` (WholeBatch, PerSample).  The sample id is uniform over the workgroup but comes from the vector
// ALU when sample_of divides: through readfirstlane, so that the index entry and the row are scalar loads.  No bounds check, no clamp.
// (Not row_at of skr_step_fast.hip: here the sample is already known, for the mask, when the row is fetched.)
template <bool PER_SAMPLE>
__device__ __forceinline__ const skr_step_row* masked_row(const RowRef& r, uint32_t smp) {
  if constexpr (PER_SAMPLE) return r.rows + (r.index[__builtin_amdgcn_readfirstlane(smp)] + r.row_offset);
  else return row_of(r);
}

template <typename T, int K, bool NOISE, RowForm F>
__global__ __launch_bounds__(BLOCK) void masked_kernel_v1(const MaskedArgsOf<F, masked_kmax(K)> a) {
  constexpr bool TILE = sizeof(T) == 4;  // whole chunks are whole tiles: 32-bit tensors take the whole-line layout, as in launch_k1
  constexpr bool TABLE = has_table(F), ROLLING = F == RowForm::Rolling;
  // (a row's doubles stay in SGPRs and are narrowed where they are used: as floats they would be 2 K VGPRs live across the loads / the Philox rounds)
  using Coef = std::conditional_t<TABLE, double, float>;
  const uint32_t c = chunk_of(blockIdx.x, a.xmap_lr);
  const int64_t v = (int64_t)c * BLOCK + threadIdx.x;
  uint32_t smp, within;
  Coef c0[K], c1[K];
  float zeta0;
  [[maybe_unused]] const skr_step_row* row;
  [[maybe_unused]] uint64_t stream0;  // (a row's)
  [[maybe_unused]] bool on[K];        // rolling: operand j is present; every other form holds all K
  // The statement order below is each form's own, and the compiled code depends on it: a rolling workgroup
  // asks its row what to touch IN FRONT of its loads, two dependent scalar round trips per wave; the other forms issue every load
  // first and fetch their scalars behind the barrier, while the loads are in flight.  No address depends on a row.
  if constexpr (ROLLING) {
    row = rolling_row(a.tab, c, a.bps_shift, smp, within);
    if (row == nullptr) return;  // inactive sample: nothing read, nothing written
#pragma unroll
    for (int j = 0; j < K; ++j) { on[j] = row_has(row, j); c0[j] = row->coef0[j]; c1[j] = row->coef1[j]; }
    zeta0 = (float)row->zeta0;
    stream0 = row->stream0;
  }
  // (rolling: each operand's pointer is fetched from the kernarg inside its branch, as in step_kernel_k1's rolling form)
  Raw<T> raw[K];  // (declared here, behind the row's scalars: even that order shows in the rolling form's registers)
#pragma unroll
  for (int j = 0; j < K; ++j) if (!ROLLING || on[j]) raw[j] = load_raw<T, TILE>(a.in[j], v);
  if constexpr (!ROLLING) sample_of(c, a.bps_shift, smp, within);
  const uint32_t vs = within * BLOCK + threadIdx.x;  // lane-vector within the sample (sample_numel < 2^31)
  // The mask index belongs to the lane-vector, not to the workgroup: a chunk may hold several wraps of the mask, or one in its middle.
  // With mask_numel % 8 == 0 a group of 4 consecutive elements never straddles a wrap, and the tile layout's two groups
  // (group0 / group1 of the lane-vector WITHIN the sample) are looked up separately.
  const uint32_t e0 = 4u * (uint32_t)group0<TILE>((int64_t)vs);
  const uint32_t m0 = e0 % a.mask_numel;
  uint32_t m1 = m0 + 4u;
  if constexpr (TILE) m1 = (4u * (uint32_t)group1<TILE>((int64_t)vs)) % a.mask_numel;
  const int64_t mbase = (int64_t)smp * a.mask_stride;
  Raw<T> rm = load_mask8<T>(a.mask, mbase + m0, mbase + m1);
  if constexpr (!ROLLING) {
    __builtin_amdgcn_sched_barrier(0);  // every load is out before the first scalar of the arithmetic (the index entry, the row) is fetched
    if constexpr (TABLE) {
      row = masked_row<F == RowForm::PerSample>(a.tab, smp);
#pragma unroll
      for (int j = 0; j < K; ++j) { c0[j] = row->coef0[j]; c1[j] = row->coef1[j]; }
      zeta0 = (float)row->zeta0;
    } else {
#pragma unroll
      for (int j = 0; j < K; ++j) { c0[j] = a.c0[j]; c1[j] = a.c1[j]; }
      zeta0 = a.zeta0;
    }
  }
  // A NOISE instantiation of a row form serves every row: one whose zeta0 narrows to zero skips the draw (a uniform branch), as a launch
  // without noise does.  The kernarg form draws unconditionally: the host chose its instantiation by the plan's zeta0.
  float z[VEC];
  [[maybe_unused]] bool n0 = false;
  if constexpr (NOISE) {
    if constexpr (TABLE) n0 = zeta0 != 0.f;
    if (!TABLE || n0) {
      if constexpr (TABLE && !ROLLING) stream0 = row->stream0;
      // (the kernarg's stream id is read where it is used, as its coefficients are: copied into stream0 first, the noisy kernarg
      //  instantiations compile to other instructions)
      const uint64_t* stream = &stream0;
      if constexpr (!TABLE) stream = &a.stream0;
      const uint64_t seed = a.seeds[smp];
      normal4(seed, *stream, (uint64_t)group0<TILE>((int64_t)vs), z);
      normal4(seed, *stream, (uint64_t)group1<TILE>((int64_t)vs), z + 4);
    }
  }
  float s[VEC], kn[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) { s[i] = 0.f; kn[i] = 0.f; }
#pragma unroll
  for (int j = 0; j < K; ++j) {
    if (!ROLLING || on[j]) {  // (uniform: the row's) present operands in slot order: the bits of the narrower launch that holds exactly these
      float w[VEC];
      widen<T, float>(raw[j], w);
      const float w0 = (float)c0[j], w1 = (float)c1[j];
#pragma unroll
      for (int i = 0; i < VEC; ++i) s[i] = fma_(w0, w[i], s[i]);
      if (w1 != 0.f) {  // (uniform: a kernarg or row scalar) an operand absent from the known form adds nothing to it, not even 0 * x
#pragma unroll
        for (int i = 0; i < VEC; ++i) kn[i] = fma_(w1, w[i], kn[i]);
      }
    }
  }
  if constexpr (NOISE) { if (!TABLE || n0) fma_noise8<float>(zeta0, z, s); }
  float m[VEC], o[VEC];
  widen<T, float>(rm, m);
#pragma unroll
  for (int i = 0; i < VEC; ++i) o[i] = fma_(m[i], s[i], mul_(sub_(1.f, m[i]), kn[i]));
  store8<T, float, TILE>(a.out, v, o);
}

// ---- general kernel: per-element accesses, run-time dtypes -----------------------------------------------------------------
struct MaskedGenArgs {
  const void* in[SKR_ROW_TERMS];
  double c0[SKR_ROW_TERMS];
  double c1[SKR_ROW_TERMS];
  const void* mask;
  void* out;
  const uint64_t* seeds;
  double zeta0;
  uint64_t stream0;
  int64_t numel, sample_numel, mask_numel, mask_stride;
  int32_t n, n_a, dt_a, dt_b, dt_out, dt_mask, noise;
};

// one rounding from Acc, the conversions of store8 (to a 16-bit dtype through the fp32 value, pinned in a register so that no fused
// multiply-add-and-convert rounds the exact sum instead).  The same function as store_any of skr_step_common.h (the backward kernels' store), kept apart: either
// body, used by both general kernels, changes the instructions of the other one.
template <typename Acc> __device__ __forceinline__ void store_elem(void* base, int64_t i, int dt, Acc v) {
  if (dt == SKR_BF16 || dt == SKR_F16) {
    float f = (float)v;
    asm("" : "+v"(f));
    if (dt == SKR_BF16) store_scalar<bf16_t, float>(base, i, f);
    else store_scalar<f16_t, float>(base, i, f);
  } else if (dt == SKR_F32) {
    store_scalar<float, Acc>(base, i, v);
  } else {
    store_scalar<double, Acc>(base, i, v);
  }
}

template <typename Acc>
__global__ __launch_bounds__(BLOCK) void masked_kernel_gen(const MaskedGenArgs a) {
  constexpr bool F64 = std::is_same<Acc, double>::value;  // (an fp64 tensor takes part in fp64 arithmetic only)
  for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < a.numel; e += (int64_t)gridDim.x * BLOCK) {
    const int64_t smp = e / a.sample_numel, r = e - smp * a.sample_numel;
    const Acc m = load_elem<Acc, F64>(a.mask, smp * a.mask_stride + r % a.mask_numel, a.dt_mask);
    Acc s = 0, kn = 0;
    for (int j = 0; j < a.n; ++j) {
      const Acc x = load_elem<Acc, F64>(a.in[j], e, j < a.n_a ? a.dt_a : a.dt_b);
      const Acc w0 = (Acc)a.c0[j], w1 = (Acc)a.c1[j];
      s = fma_(w0, x, s);
      if (w1 != (Acc)0) kn = fma_(w1, x, kn);
    }
    if (a.noise) {  // element r of the sample: Philox block r >> 2, lane r & 3 (sample_numel % 8 == 0, checked on the host)
      float z[4];
      normal4(a.seeds[smp], a.stream0, (uint64_t)r >> 2, z);
      const int lane = (int)(r & 3);
      const float zz = lane == 0 ? z[0] : (lane == 1 ? z[1] : (lane == 2 ? z[2] : z[3]));
      s = fma_((Acc)a.zeta0, (Acc)zz, s);
    }
    store_elem<Acc>(a.out, e, a.dt_out, fma_(m, s, mul_(sub_((Acc)1, m), kn)));
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// the one-trip launch of any form: dtype x noise x form x operand count to the instantiation, and its kernarg
static void launch_masked_v1(const skr_step_plan& p, const void* const* inputs, void* out, const skr_step_mask& mk, const uint64_t* seeds,
                             const MaskedLaunch& l, RowForm form, const RowRef& tab, hipStream_t s) {
  with_step_type<false>(p.dtype_a, [&](auto tt) {
    with_bools([&](auto nz) {
      with_row_form(form, [&](auto fm) {
        with_count<1, SKR_ROW_TERMS>(p.n_terms, [&](auto n) {
          using T = typename decltype(tt)::type;
          constexpr int N = decltype(n)::value, KMAX = masked_kmax(N);
          constexpr RowForm F = decltype(fm)::value;
          MaskedArgsOf<F, KMAX> a;
          for (int k = 0; k < KMAX; ++k) a.in[k] = k < N ? inputs[k] : nullptr;
          a.mask = mk.mask; a.out = out; a.seeds = seeds;
          a.xmap_lr = xmap_lr_for(l.chunks); a.bps_shift = l.bps_shift;
          a.mask_numel = (uint32_t)mk.mask_numel; a.mask_stride = (uint32_t)mk.batch_stride;
          if constexpr (has_table(F)) {
            a.tab = tab;
          } else {
            for (int k = 0; k < KMAX; ++k) { a.c0[k] = k < N ? (float)p.coef0[k] : 0.f; a.c1[k] = k < N ? (float)p.coef1[k] : 0.f; }
            a.stream0 = p.stream0; a.zeta0 = (float)p.zeta0;
          }
          hipLaunchKernelGGL((masked_kernel_v1<T, N, decltype(nz)::value, F>), dim3((unsigned)l.chunks), dim3(BLOCK), 0, s, a);
        });
      });
    }, l.noise);
  });
}

// Every check of a masked launch behind its NULL tests, in skr_step_launch_masked's order and with its codes; `rows`: for a row form, whose
// plan scalars are ignored.  SKR_OK with numel == 0 means "nothing to do".  (Declared in skr_step_masked.h: the channels-last entry asks it too.)
int masked_prepare(const skr_step_plan& p, const skr_step_mask& mk, const void* const* inputs, void* out, const uint64_t* seeds_dev, int64_t numel,
                          bool rows, MaskedLaunch* launch) {
  launch->noise = launch->one_trip = false;
  if (p.n_terms < 0 || p.n_group_a < 0 || p.n_group_a > p.n_terms || p.n_terms > SKR_ROW_TERMS) return SKR_ERR_TERMS;
  if (numel < 0) return SKR_ERR_SHAPE;
  if (p.out0_dtype == SKR_NONE) return SKR_ERR_NULL;
  if (p.out1_dtype != SKR_NONE || p.chain != 0.0 || p.zeta1 != 0.0 || p.convert_to != 0 || p.convert_from != 0 || mk.reserved != 0 ||
      (p.noise_mode != 0 && p.noise_mode != 1))
    return SKR_ERR_UNSUPPORTED;
  if (p.sample_numel <= 0 || numel % p.sample_numel != 0) return SKR_ERR_SHAPE;
  if (mk.mask_numel < 1 || p.sample_numel % mk.mask_numel != 0 || (mk.batch_stride != 0 && mk.batch_stride != mk.mask_numel)) return SKR_ERR_SHAPE;
  const bool noise = p.noise_mode == 1 && (rows || p.zeta0 != 0.0);
  if (noise && p.sample_numel % 8 != 0) return SKR_ERR_UNSUPPORTED;  // fused Philox needs every 8-element group inside one sample, as in skr_step_launch
  // the dtype combinations of skr_step_launch, with one output; the mask: a 16-bit dtype or the arithmetic's
  const int32_t db = p.n_group_a == p.n_terms ? p.dtype_a : p.dtype_b;
  if (!step_inputs_ok(p.dtype_a, db, p.acc_f64) || !step_output_ok(p.out0_dtype, p.dtype_a, p.acc_f64)) return SKR_ERR_DTYPE;
  if (mk.dtype != SKR_BF16 && mk.dtype != SKR_F16 && mk.dtype != SKR_F32 && !(mk.dtype == SKR_F64 && p.acc_f64)) return SKR_ERR_DTYPE;
  if (numel == 0) return SKR_OK;
  if ((p.n_terms > 0 && !inputs) || !out || !mk.mask || (noise && !seeds_dev)) return SKR_ERR_NULL;
  if (const int rc = check_ptrs(inputs, p.n_terms)) return rc;
  if (!aligned16(out) || !aligned16(mk.mask)) return SKR_ERR_ALIGN;
  launch->noise = noise;

  constexpr int64_t CHUNK = (int64_t)BLOCK * VEC;
  const int t = p.dtype_a;
  const bool one_dtype = (p.n_group_a == p.n_terms || p.dtype_b == t) && p.out0_dtype == t && mk.dtype == t && t != SKR_F64;
  if (g_tune.one_trip && !p.acc_f64 && one_dtype && p.n_terms >= 1 && (t != SKR_F32 || g_tune.tile) && numel % CHUNK == 0 &&
      numel / CHUNK <= 0x7fffffffll && p.sample_numel % CHUNK == 0 && p.sample_numel < (1ll << 31) && mk.mask_numel % 8 == 0) {
    launch->one_trip = true; launch->chunks = numel / CHUNK; launch->bps_shift = bps_shift_of(p.sample_numel / CHUNK);
  }
  return SKR_OK;
}

// The four entries (from the table test on: rows != nullptr exactly when has_table(form)).  A row form has no grid-stride kernel: what
// the one-trip kernel does not cover is SKR_ERR_UNSUPPORTED.
static int masked_launch_impl(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_mask* mask, const uint64_t* seeds_dev,
                              int64_t numel, void* stream, RowForm form, const skr_step_row* rows, const int32_t* index, int32_t row_offset) {
  if (!plan || !mask || (has_table(form) && (!rows || (per_sample_rows(form) && !index)))) return SKR_ERR_NULL;
  const skr_step_plan& p = *plan;
  const skr_step_mask& mk = *mask;
  MaskedLaunch l;
  if (const int rc = masked_prepare(p, mk, inputs, out, seeds_dev, numel, has_table(form), &l)) return rc;
  if (numel == 0) return SKR_OK;
  if (has_table(form) && (!l.one_trip || row_offset < 0)) return SKR_ERR_UNSUPPORTED;
  DeviceGuard device_guard(out);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);

  if (l.one_trip) {
    launch_masked_v1(p, inputs, out, mk, seeds_dev, l, form, RowRef{rows, index, row_offset}, s);
    return finish_launch();
  }

  MaskedGenArgs a;
  for (int k = 0; k < SKR_ROW_TERMS; ++k) {
    const bool live = k < p.n_terms;
    a.in[k] = live ? inputs[k] : nullptr;
    a.c0[k] = live ? p.coef0[k] : 0.0;
    a.c1[k] = live ? p.coef1[k] : 0.0;
  }
  a.mask = mk.mask; a.out = out; a.seeds = seeds_dev; a.zeta0 = p.zeta0; a.stream0 = p.stream0;
  a.numel = numel; a.sample_numel = p.sample_numel; a.mask_numel = mk.mask_numel; a.mask_stride = mk.batch_stride;
  a.n = p.n_terms; a.n_a = p.n_group_a; a.dt_a = p.dtype_a; a.dt_b = p.dtype_b; a.dt_out = p.out0_dtype; a.dt_mask = mk.dtype;
  a.noise = l.noise ? 1 : 0;
  const dim3 grid((unsigned)grid_blocks(numel, BLOCK, 256 * 64));
  with_bools([&](auto f64) { hipLaunchKernelGGL((masked_kernel_gen<std::conditional_t<decltype(f64)::value, double, float>>), grid, dim3(BLOCK), 0, s, a); }, p.acc_f64 != 0);
  return finish_launch();
}

}  // namespace skr

extern "C" int skr_step_launch_masked(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_mask* mask,
                                      const uint64_t* seeds_dev, int64_t numel, void* stream) {
  return skr::masked_launch_impl(plan, inputs, out, mask, seeds_dev, numel, stream, skr::RowForm::Kernarg, nullptr, nullptr, 0);
}

extern "C" int skr_step_launch_masked_indexed(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_mask* mask,
                                              const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev,
                                              const int32_t* index_dev, int32_t row_offset, void* stream) {
  return skr::masked_launch_impl(plan, inputs, out, mask, seeds_dev, numel, stream, skr::RowForm::WholeBatch, rows_dev, index_dev, row_offset);
}

extern "C" int skr_step_launch_masked_indexed_per_sample(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_mask* mask,
                                                         const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev,
                                                         const int32_t* sample_index_dev, int32_t row_offset, void* stream) {
  return skr::masked_launch_impl(plan, inputs, out, mask, seeds_dev, numel, stream, skr::RowForm::PerSample, rows_dev, sample_index_dev, row_offset);
}

extern "C" int skr_step_launch_masked_rolling(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_mask* mask,
                                              const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev,
                                              const int32_t* sample_index_dev, int32_t row_offset, void* stream) {
  return skr::masked_launch_impl(plan, inputs, out, mask, seeds_dev, numel, stream, skr::RowForm::Rolling, rows_dev, sample_index_dev, row_offset);
}
