// Ragged-sample form of the single-output one-trip step kernel for MI355X (gfx950): the job of step_kernel_k1 (skr_step_fast.hip) for
// the three table forms when a sample is NOT made of whole 2048-element chunks -- most non-square SDXL latent buckets, e.g. (4,144,112)
// = 31.5 chunks.  A sample then takes ceil(sample_numel / 2048) workgroups of its own, the last of them partly empty; the step kernels
// use no LDS and no barriers, so a dead lane simply leaves.  Arithmetic, lane ownership within the sample and Philox block numbering
// are those of step_kernel_k1, so every sample has the bits skr_step_launch writes for it alone (tests/test_ragged_samples_gpu.py).
// A translation unit of its own, sharing only skr_step_common.h: the whole-chunk instantiations keep their device code
// (profiles/ragged_samples_isa.txt).
#include "skr_step_common.h"

namespace skr {

// Kernarg: what the first instructions need (pointers, chunk map, sample size) leads; the scalars are the row's, so no coefficient
// block follows and launches of <= 4 operands carry one 64-byte line plus the row reference.
template <int KMAX>
struct RaggedArgs {
  const void* in[KMAX];
  void* out0;
  const uint64_t* seeds;
  int32_t xmap_lr;        // log2(run length) of the XCD chunk map over batch * bps workgroups
  int32_t bps_shift;      // chunks per sample, the last one partial: log2 of a power of two, or minus the count (sample_of)
  uint32_t sample_numel;  // >= 2048, a multiple of 8 and not of 2048, < 2^31
  RowRef tab;
};

constexpr int ragged_kmax(int k) { return k <= 4 ? 4 : (k <= 8 ? 8 : (k <= 12 ? 12 : 16)); }

// Which of a lane's elements lie inside the sample (vs: the lane-vector within the sample).  16-bit tensors: the lane's 8 consecutive
// elements, all or none (sample_numel % 8 == 0).  32-bit tensors use the tile layout: two groups of 4 elements each, group1 64 groups
// behind group0, so group1 is dead wherever group0 is; only a sample's last chunk has dead groups.
template <typename T>
struct Live {
  bool g0, g1;
  __device__ __forceinline__ Live(uint32_t vs, uint32_t sample_numel) {
    if constexpr (sizeof(T) == 2) { g0 = g1 = 8u * vs < sample_numel; }
    else {
      g0 = 4u * (uint32_t)group0<true>((int64_t)vs) < sample_numel;
      g1 = 4u * (uint32_t)group1<true>((int64_t)vs) < sample_numel;
    }
  }
};

// load_raw / store8 of skr_step_common.h with dead groups left out: a dead group issues no load and no store (its registers read as
// zeros, its sums are never stored).  16-bit lanes reach these live as a whole (the kernel has returned for the others).
template <typename T>
__device__ __forceinline__ Raw<T> load_raw_live(const void* base, uint32_t vs, const Live<T>& live) {
  if constexpr (sizeof(T) == 2) return load_raw<T, false>(base, (int64_t)vs);
  else {
    Raw<T> r;
    const f32x4_t* p = reinterpret_cast<const f32x4_t*>(base);
    r.q[0] = __builtin_nontemporal_load(p + group0<true>((int64_t)vs));
    r.q[1] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if (live.g1) r.q[1] = __builtin_nontemporal_load(p + group1<true>((int64_t)vs));
    return r;
  }
}
template <typename T>
__device__ __forceinline__ void store8_live(void* base, uint32_t vs, const float v[VEC], const Live<T>& live) {
  if constexpr (sizeof(T) == 2) store8<T, float, false>(base, (int64_t)vs, v);
  else {
    f32x4_t* p = reinterpret_cast<f32x4_t*>(base);
    store16_stream(p + group0<true>((int64_t)vs), f32x4_t{v[0], v[1], v[2], v[3]});
    if (live.g1) store16_stream(p + group1<true>((int64_t)vs), f32x4_t{v[4], v[5], v[6], v[7]});
  }
}

// a sample's slice of a tensor: a uniform scalar offset, 16-byte aligned because sample_numel % 8 == 0
template <typename T> __device__ __forceinline__ const void* sample_base(const void* p, uint64_t offset) { return reinterpret_cast<const T*>(p) + offset; }
template <typename T> __device__ __forceinline__ void* sample_base(void* p, uint64_t offset) { return reinterpret_cast<T*>(p) + offset; }

// F: WholeBatch, PerSample or Rolling.  Each form keeps its row fetch where its whole-chunk twin has it: behind the scheduling barrier
// that follows the loads for WholeBatch and PerSample, in front of the loads -- with the inactive exit before the first vector-memory
// instruction and absent operands neither loaded nor summed -- for Rolling.  No paced variant.
template <typename T, int K, bool NOISE, RowForm F>
__global__ __launch_bounds__(BLOCK) void step_kernel_ragged(const RaggedArgs<ragged_kmax(K)> a) {
  static_assert(has_table(F), "the ragged form serves the table launches");
  constexpr bool TILE = sizeof(T) == 4;
  const uint32_t c = chunk_of(blockIdx.x, a.xmap_lr);
  uint32_t smp, within;
  [[maybe_unused]] const skr_step_row* row = nullptr;
  if constexpr (F == RowForm::Rolling) {
    row = rolling_row(a.tab, c, a.bps_shift, smp, within);
    if (row == nullptr) return;  // inactive sample: nothing read, nothing written
  } else {
    sample_of(c, a.bps_shift, smp, within);
    smp = __builtin_amdgcn_readfirstlane(smp);  // (the dividing form runs on the vector ALU: the slice offsets and the row fetch stay scalar)
  }
  within = __builtin_amdgcn_readfirstlane(within);
  const uint32_t vs = within * BLOCK + threadIdx.x;  // lane-vector within the sample
  const Live<T> live(vs, a.sample_numel);
  if (!live.g0) return;  // dead lane; a wave whose lanes are all dead ends here
  const uint64_t at = (uint64_t)smp * a.sample_numel;
  if constexpr (F == RowForm::Rolling) {
    bool on[K];
    double cd[K];  // (converted to float where they are used, see step_kernel_k1)
#pragma unroll
    for (int j = 0; j < K; ++j) { on[j] = row_has(row, j); cd[j] = row->coef0[j]; }
    const float zeta0 = (float)row->zeta0;
    const uint64_t stream0 = row->stream0;
    constexpr int AHEAD = (sizeof(T) == 2 && K > 12) ? 12 : K;  // 16-bit launches of more than 12 operands keep 12 loads in flight
    Raw<T> raw[K];
#pragma unroll
    for (int j = 0; j < AHEAD; ++j) if (on[j]) raw[j] = load_raw_live<T>(sample_base<T>(a.in[j], at), vs, live);
    float z[VEC];
    bool n0 = false;
    if constexpr (NOISE) {
      n0 = zeta0 != 0.f;
      if (n0) {
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
      if (on[j]) {  // present operands in slot order: the bits of the narrower launch that holds exactly these
        float w[VEC];
        widen<T, float>(raw[j], w);
        const float cj = (float)cd[j];
#pragma unroll
        for (int i = 0; i < VEC; ++i) s[i] = fma_(cj, w[i], s[i]);
      }
      if constexpr (AHEAD < K) {
        if (j + AHEAD < K) { if (on[j + AHEAD]) raw[j + AHEAD] = load_raw_live<T>(sample_base<T>(a.in[j + AHEAD], at), vs, live); }
      }
    }
    if constexpr (NOISE) { if (n0) fma_noise8<float>(zeta0, z, s); }
    store8_live<T>(sample_base<T>(a.out0, at), vs, s, live);
  } else {
    Raw<T> raw[K];
#pragma unroll
    for (int j = 0; j < K; ++j) raw[j] = load_raw_live<T>(sample_base<T>(a.in[j], at), vs, live);
    __builtin_amdgcn_sched_barrier(0);  // every load is out before the row is asked for (two dependent scalar loads)
    if constexpr (F == RowForm::PerSample) row = a.tab.rows + (a.tab.index[smp] + a.tab.row_offset);
    else row = row_of(a.tab);
    float cf[K];
#pragma unroll
    for (int j = 0; j < K; ++j) cf[j] = (float)row->coef0[j];
    const float zeta0 = (float)row->zeta0;
    float z[VEC];
    bool n0 = false;
    if constexpr (NOISE) {
      n0 = zeta0 != 0.f;  // (a zero row skips the draw, as a launch without noise does)
      if (n0) {
        const uint64_t stream0 = row->stream0;
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
      const float cj = cf[j];
#pragma unroll
      for (int i = 0; i < VEC; ++i) s[i] = fma_(cj, w[i], s[i]);
    }
    if constexpr (NOISE) { if (n0) fma_noise8<float>(zeta0, z, s); }
    store8_live<T>(sample_base<T>(a.out0, at), vs, s, live);
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// A single-output plan: one 16- or 32-bit dtype for the operands and out0, no second output, no rounded conversion, fp32 accumulation,
// 1 to SKR_ROW_TERMS operands (what step_kernel_k1 serves for the table forms).
static bool single_output_plan(const skr_step_plan& p) {
  if (p.out1_dtype != SKR_NONE || p.convert_to != 0 || p.convert_from != 0 || p.acc_f64) return false;
  if (p.n_terms < 1 || p.n_terms > SKR_ROW_TERMS) return false;
  if (p.dtype_a != SKR_BF16 && p.dtype_a != SKR_F16 && p.dtype_a != SKR_F32) return false;
  if (p.n_group_a != p.n_terms && p.dtype_b != p.dtype_a) return false;
  return p.out0_dtype == p.dtype_a;
}

bool ragged_launch(const skr_step_plan& p, int64_t numel, RowForm form) {
  constexpr int64_t CHUNK = (int64_t)BLOCK * VEC;
  if (!has_table(form) || !single_output_plan(p)) return false;
  const int64_t sn = p.sample_numel;
  if (sn < CHUNK || sn % 8 != 0 || sn % CHUNK == 0 || sn >= (1ll << 31) || numel <= 0 || numel % sn != 0) return false;
  if ((numel / sn) * ((sn + CHUNK - 1) / CHUNK) > 0x7fffffffll) return false;  // the grid limit of the whole-chunk kernels
  // a whole-batch row launch that the whole-chunk kernel takes (no draw, whole chunks in all) keeps it
  return per_sample_rows(form) || p.noise_mode == 1 || numel % CHUNK != 0;
}

template <typename T, bool NOISE>
static void launch_ragged_as(const skr_step_plan& p, const void* const* inputs, void* out0, const uint64_t* seeds, int64_t numel, hipStream_t stream,
                             RowForm form, const skr_step_row* rows, const int32_t* index, int32_t row_offset) {
  constexpr int64_t CHUNK = (int64_t)BLOCK * VEC;
  const int64_t bps = (p.sample_numel + CHUNK - 1) / CHUNK, chunks = (numel / p.sample_numel) * bps;
  with_count<1, SKR_ROW_TERMS>(p.n_terms, [&](auto n) {
    constexpr int N = decltype(n)::value;
    RaggedArgs<ragged_kmax(N)> ra;
    for (int k = 0; k < ragged_kmax(N); ++k) ra.in[k] = k < N ? inputs[k] : nullptr;
    ra.out0 = out0; ra.seeds = seeds;
    ra.xmap_lr = xmap_lr_for(chunks); ra.bps_shift = bps_shift_of(bps); ra.sample_numel = (uint32_t)p.sample_numel;
    ra.tab = RowRef{rows, index, row_offset};
    with_row_form(form, [&](auto fm) {
      constexpr RowForm F = decltype(fm)::value;
      if constexpr (has_table(F)) hipLaunchKernelGGL((step_kernel_ragged<T, N, NOISE, F>), dim3((unsigned)chunks), dim3(BLOCK), 0, stream, ra);
    });
  });
}

int launch_ragged(const skr_step_plan& p, const void* const* inputs, void* out0, const uint64_t* seeds, int64_t numel, hipStream_t stream,
                  RowForm form, const skr_step_row* rows, const int32_t* index, int32_t row_offset) {
  return with_step_type<false>(p.dtype_a, [&](auto t) {
    using T = typename decltype(t)::type;
    if (p.noise_mode == 1) launch_ragged_as<T, true>(p, inputs, out0, seeds, numel, stream, form, rows, index, row_offset);
    else launch_ragged_as<T, false>(p, inputs, out0, seeds, numel, stream, form, rows, index, row_offset);
    return finish_launch();
  });
}

}  // namespace skr
