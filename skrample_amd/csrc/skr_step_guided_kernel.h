// The one-trip kernel of the guided step, its kernargs and its launcher: what skr_step_guided.hip (which states the contract) and
// skr_step_guided_rescaled.hip (which only instantiates the RESCALE half) share.
#pragma once
#include "skr_step_guided.h"
#include "skr_device.h"

namespace skr {

constexpr int guided_kmax(int k) { return k <= 4 ? 4 : (k <= 8 ? 8 : (k <= 12 ? 12 : 16)); }

// Kernargs of the one-trip kernel, one per layout (offsets are part of the device code).  What the first instructions need (operand
// pointers, chunk map) leads, as in MaskedArgs; up to 4 operands a row form's is two 64-byte lines.
template <int KMAX>
struct GuidedArgs {  // Kernarg
  const void* in[KMAX];
  const void* cond;
  void* out;
  void* guided;         // nullptr: p' is not stored
  int32_t xmap_lr;      // log2(run length) of the XCD chunk map
  int32_t bps_shift;    // chunks per sample: log2 when >= 0, minus the count otherwise (see sample_of); read where sample_of runs
  const uint64_t* seeds;
  uint64_t stream0;
  float zeta0;
  float scale;          // g in the op-math type
  int32_t slot;         // the operand that p' replaces in the sum
  float c0[KMAX];
};
template <int KMAX>
struct GuidedRescaledArgs {  // Kernarg, rescaled
  const void* in[KMAX];
  const void* cond;
  void* out;
  void* guided;
  int32_t xmap_lr;
  int32_t bps_shift;    // of the statistic's sample (and the draw's)
  const uint64_t* seeds;
  const void* factor;   // T[samples]
  uint64_t stream0;
  float zeta0;
  float scale;
  float phi, psi;       // guidance_rescale and 1 - guidance_rescale, each narrowed once
  int32_t slot;
  float c0[KMAX];
};
template <int KMAX>
struct GuidedRowArgs {  // the three row forms: GuidedArgs without the scalars a row carries
  const void* in[KMAX];
  const void* cond;
  void* out;
  void* guided;
  int32_t xmap_lr;
  int32_t bps_shift;
  const uint64_t* seeds;
  RowRef tab;
  int32_t slot;
};
template <int KMAX>
struct GuidedRescaledRowArgs {  // the three row forms, rescaled
  const void* in[KMAX];
  const void* cond;
  void* out;
  void* guided;
  int32_t xmap_lr;
  int32_t bps_shift;
  const uint64_t* seeds;
  const void* factor;   // T[samples]: read for the rows that rescale
  RowRef tab;
  int32_t slot;
};
template <RowForm F, bool RESCALE, int KMAX>
using GuidedArgsOf = std::conditional_t<has_table(F), std::conditional_t<RESCALE, GuidedRescaledRowArgs<KMAX>, GuidedRowArgs<KMAX>>,
                                        std::conditional_t<RESCALE, GuidedRescaledArgs<KMAX>, GuidedArgs<KMAX>>>;

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

// The row of a workgroup of sample `smp` (WholeBatch, PerSample).  The sample id is uniform over the workgroup but comes from the vector
// ALU when sample_of divides: through readfirstlane, so that the index entry and the row are scalar loads.  No bounds check, no clamp.
template <bool PER_SAMPLE>
__device__ __forceinline__ const skr_step_row* guided_row(const RowRef& r, uint32_t smp) {
  if constexpr (PER_SAMPLE) return r.rows + (r.index[__builtin_amdgcn_readfirstlane(smp)] + r.row_offset);
  else return row_of(r);
}

// Rolling: an operand other than the slot is present unless its coef0 is exactly zero (either sign): decided on the row's double, in SGPRs
__device__ __forceinline__ bool guided_row_has(const skr_step_row* row, int j) { return (__builtin_bit_cast(uint64_t, row->coef0[j]) << 1) != 0; }
// a row rescales unless its phi is exactly zero (either sign)
__device__ __forceinline__ bool rescaling(double phi) { return (__builtin_bit_cast(uint64_t, phi) << 1) != 0; }

template <typename T, int K, bool NOISE, RowForm F, bool RESCALE>
__global__ __launch_bounds__(BLOCK) void guided_kernel_v1(const GuidedArgsOf<F, RESCALE, guided_kmax(K)> a) {
  constexpr bool TILE = sizeof(T) == 4;  // whole chunks are whole tiles: 32-bit tensors take the whole-line layout, as in launch_k1
  constexpr bool TABLE = has_table(F), ROLLING = F == RowForm::Rolling, PER_SAMPLE = F == RowForm::PerSample;
  // The rescaled WholeBatch and PerSample forms have three branches behind their loads (sample_of's, the phi test, the draw), and the
  // scheduling barrier holds inside its basic block only: the compiler would sink the loads to their first use, behind the row's round
  // trips and the factor's.  An empty statement that may write memory keeps them in front; what is read behind it -- index, row, seed,
  // a 32-bit factor -- is read-only for the launch and read through the constant address space, so that it stays scalar loads
  // (profiles/guided_rescale_rows_isa.txt).
  constexpr bool CLOBBER = RESCALE && row_behind_loads(F);
  // (a row's doubles stay in SGPRs and are narrowed where they are used: as floats they would be K VGPRs live across the loads / the Philox rounds)
  using Coef = std::conditional_t<TABLE, double, float>;
  using Row = std::conditional_t<CLOBBER, decltype(uniform((const skr_step_row*)nullptr)), const skr_step_row*>;
  const uint32_t c = chunk_of(blockIdx.x, a.xmap_lr);
  const int64_t v = (int64_t)c * BLOCK + threadIdx.x;
  [[maybe_unused]] uint32_t smp = 0, within = 0;
  Coef c0[K];
  float zeta0, g;
  int32_t slot;
  [[maybe_unused]] Row row;
  [[maybe_unused]] uint64_t stream0;  // (a row's)
  [[maybe_unused]] bool on[K];        // rolling: operand j is present; every other form holds all K
  [[maybe_unused]] double phi_d;      // a row's phi, and whether it rescales:
  [[maybe_unused]] bool rescales = false;
  // The statement order below is each form's own, and the compiled code depends on it: a rolling workgroup asks
  // its row what to touch IN FRONT of its loads, two dependent scalar round trips per wave; the other forms issue every load first and
  // fetch their scalars behind the barrier, while the loads are in flight.  No address depends on a row.
  if constexpr (ROLLING) {
    row = rolling_row(a.tab, c, a.bps_shift, smp, within);
    if (row == nullptr) return;  // inactive sample: nothing read, nothing written
    slot = a.slot;
#pragma unroll
    for (int j = 0; j < K; ++j) { c0[j] = row->coef0[j]; on[j] = j == slot || guided_row_has(row, j); }
    zeta0 = (float)row->zeta0, g = (float)row->convert_k[0];
    if constexpr (RESCALE) { phi_d = row->convert_k[1]; rescales = rescaling(phi_d); }
    stream0 = row->stream0;
  }
  // (rolling: each operand's pointer is fetched from the kernarg inside its branch)
  Raw<T> raw[K];
#pragma unroll
  for (int j = 0; j < K; ++j) if (!ROLLING || on[j]) raw[j] = load_raw<T, TILE>(a.in[j], v);
  Raw<T> rc = load_raw<T, TILE>(a.cond, v);
  // (declared here, behind the loads: at the top of the function the rescaled row forms compile to other code)
  [[maybe_unused]] float r = 0.f, phi = 0.f, psi = 0.f;
  [[maybe_unused]] uint16_t r16 = 0;  // CLOBBER: a 16-bit factor as its bits
  if constexpr (!ROLLING) {
    if constexpr (CLOBBER) asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);  // every load is out before the first scalar of the arithmetic (the index entry, the row) is fetched
    // (the unrescaled Kernarg form asks for its sample inside the draw -- only a launch that draws has samples at all --, and asked here
    //  its noisy instantiations compile to other code)
    if constexpr (RESCALE || PER_SAMPLE || (TABLE && NOISE)) sample_of(c, a.bps_shift, smp, within);
    if constexpr (TABLE) {
      if constexpr (CLOBBER) {
        smp = __builtin_amdgcn_readfirstlane(smp);  // (uniform over the workgroup) the index entry, the row, the seed and a 32-bit factor are scalar loads
        int32_t at = 0;  // (guided_row's lookup, spelt out: behind a function that takes a.tab by reference the kernarg is read ahead of the loads)
        if constexpr (PER_SAMPLE) at = uniform(a.tab.index)[smp];
        else if (a.tab.index != nullptr) at = uniform(a.tab.index)[0];
        row = uniform(a.tab.rows + (at + a.tab.row_offset));
      } else {
        row = guided_row<PER_SAMPLE>(a.tab, smp);
      }
#pragma unroll
      for (int j = 0; j < K; ++j) c0[j] = row->coef0[j];
      zeta0 = (float)row->zeta0, g = (float)row->convert_k[0];
      if constexpr (RESCALE) { phi_d = row->convert_k[1]; rescales = rescaling(phi_d); }
    } else {
      if constexpr (RESCALE) r = load_scalar<T>(a.factor, (int64_t)smp);  // (uniform: one sample per workgroup) unconditional
#pragma unroll
      for (int j = 0; j < K; ++j) c0[j] = a.c0[j];
      zeta0 = a.zeta0, g = a.scale;
      if constexpr (RESCALE) { phi = a.phi; psi = a.psi; }
    }
    slot = a.slot;
  }
  if constexpr (TABLE && RESCALE) {
    if (rescales) {  // one uniform load behind the operand loads; an unrescaled row's factor is never touched
      if constexpr (!CLOBBER) r = load_scalar<T>(a.factor, (int64_t)smp);
      else if constexpr (TILE) r = uniform(reinterpret_cast<const float*>(a.factor))[smp];
      else r16 = reinterpret_cast<const uint16_t*>(a.factor)[smp];  // (a 16-bit value has no scalar load; widened where it is used, so that nothing waits for it here)
      phi = (float)phi_d;
      psi = (float)sub_(1.0, phi_d);  // 1 - phi formed in double, narrowed once
    }
  }
  // A NOISE instantiation of a row form serves every row: one whose zeta0 narrows to zero skips the draw (a uniform branch), as a launch
  // without noise does.  The kernarg form draws unconditionally: the host chose its instantiation by the plan's zeta0.
  float z[VEC];
  [[maybe_unused]] bool n0 = false;
  if constexpr (NOISE) {
    if constexpr (TABLE) n0 = zeta0 != 0.f;
    if (!TABLE || n0) {
      if constexpr (!TABLE && !RESCALE) sample_of(c, a.bps_shift, smp, within);
      if constexpr (TABLE && !ROLLING) stream0 = row->stream0;
      // (the kernarg's stream id is read where it is used, as in masked_kernel_v1)
      const uint64_t* stream = &stream0;
      if constexpr (!TABLE) stream = &a.stream0;
      const uint32_t vs = within * BLOCK + threadIdx.x;  // lane-vector within the sample (sample_numel < 2^31)
      uint64_t seed;
      if constexpr (CLOBBER) seed = uniform(a.seeds)[smp];
      else seed = a.seeds[smp];
      normal4(seed, *stream, (uint64_t)group0<TILE>((int64_t)vs), z);
      normal4(seed, *stream, (uint64_t)group1<TILE>((int64_t)vs), z + 4);
    }
  }
  float s[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) s[i] = 0.f;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    if (!ROLLING || on[j]) {  // (uniform: the row's) present operands in slot order: the bits of the narrower launch that holds exactly these
      float w[VEC];
      widen<T, float>(raw[j], w);
      if (j == slot) {  // (uniform: a kernarg scalar against the unrolled operand's number) the guided value takes this operand's place
        float cf[VEC];
        widen<T, float>(rc, cf);
        if constexpr (!TABLE && RESCALE) {  // (one loop where the rescale is unconditional: as two, every instantiation compiles to other code)
#pragma unroll
          for (int i = 0; i < VEC; ++i) w[i] = rescaled_value<T>(guided_value<T>(w[i], cf[i], g), r, phi, psi);
        } else {
#pragma unroll
          for (int i = 0; i < VEC; ++i) w[i] = guided_value<T>(w[i], cf[i], g);
          if constexpr (RESCALE) {
            if (rescales) {  // (uniform: the row's) a real branch: p' = p otherwise
              if constexpr (CLOBBER && !TILE) {
                uint32_t bits = r16;
                asm volatile("" : "+v"(bits));  // (the widening stays here: hoisted into the branch of the load it would wait for every load in flight)
                r = widen_bits<T>((uint16_t)bits);
              }
#pragma unroll
              for (int i = 0; i < VEC; ++i) w[i] = rescaled_value<T>(w[i], r, phi, psi);
            }
          }
        }
        if (a.guided != nullptr) store8<T, float, TILE>(a.guided, v, w);  // (p' is a value of T: the store's rounding is exact)
      }
      const float w0 = (float)c0[j];
#pragma unroll
      for (int i = 0; i < VEC; ++i) s[i] = fma_(w0, w[i], s[i]);
    }
  }
  if constexpr (NOISE) { if (!TABLE || n0) fma_noise8<float>(zeta0, z, s); }
  store8<T, float, TILE>(a.out, v, s);
}

// What the entry checks of a guided launch leave behind for its launcher.
struct GuidedLaunch {
  bool step_out;   // the launch has a step output (out0_dtype is a dtype): false is the guidance-only form
  bool noise;      // the launch may draw: the plan's zeta0 decides for the kernarg form, noise_mode alone for the row forms (the row's zeta0 is data)
  bool one_trip;   // the one-trip vector kernel covers it (the row forms have no other)
  int64_t chunks;  // 2048-element chunks of the launch, and
  int bps_shift;   // chunks per sample as the kernels take them (sample_of; 0 where the kernel does not ask); both set when one_trip
  int32_t dtype_b, dtype_g;  // the dtype of group b (group a's when that group is empty) and of the group `slot` lies in
};

// The one-trip launch of any form of one RESCALE (`rs` non-null exactly when it is set): dtype x noise x form x operand count to the
// instantiation, and its kernarg.  A translation unit holds the kernels of the RESCALE it names: skr_step_guided.hip false,
// skr_step_guided_rescaled.hip true, 384 each, so that neither outlasts skr_step_fast.hip in the build.
template <bool RESCALE>
static void launch_guided_v1(const skr_step_plan& p, const void* const* inputs, void* out, const skr_step_guidance& gd, const skr_step_rescale* rs,
                                const uint64_t* seeds, const GuidedLaunch& l, RowForm form, const RowRef& tab, hipStream_t s) {
  with_step_type<false>(p.dtype_a, [&](auto tt) {
    with_bools([&](auto nz) {
      with_row_form(form, [&](auto fm) {
        with_count<1, SKR_ROW_TERMS>(p.n_terms, [&](auto n) {
          using T = typename decltype(tt)::type;
          constexpr int N = decltype(n)::value, KMAX = guided_kmax(N);
          constexpr RowForm F = decltype(fm)::value;
          GuidedArgsOf<F, RESCALE, KMAX> a;
          for (int k = 0; k < KMAX; ++k) a.in[k] = k < N ? inputs[k] : nullptr;
          a.cond = gd.cond; a.out = out; a.guided = gd.guided_out; a.seeds = seeds;
          a.xmap_lr = xmap_lr_for(l.chunks); a.bps_shift = l.bps_shift; a.slot = gd.slot;
          if constexpr (RESCALE) a.factor = rs->factor_dev;
          if constexpr (has_table(F)) {
            a.tab = tab;
          } else {
            for (int k = 0; k < KMAX; ++k) a.c0[k] = k < N ? (float)p.coef0[k] : 0.f;
            a.stream0 = p.stream0; a.zeta0 = (float)p.zeta0; a.scale = (float)gd.scale;
            if constexpr (RESCALE) { a.phi = (float)rs->phi; a.psi = (float)(1.0 - rs->phi); }
          }
          hipLaunchKernelGGL((guided_kernel_v1<T, N, decltype(nz)::value, F, RESCALE>), dim3((unsigned)l.chunks), dim3(BLOCK), 0, s, a);
        });
      });
    }, l.noise);
  });
}

// the RESCALE half, in skr_step_guided_rescaled.hip
void launch_guided_rescaled_v1(const skr_step_plan& p, const void* const* inputs, void* out, const skr_step_guidance& gd, const skr_step_rescale* rs,
                               const uint64_t* seeds, const GuidedLaunch& l, RowForm form, const RowRef& tab, hipStream_t s);

}  // namespace skr
