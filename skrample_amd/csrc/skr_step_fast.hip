// One-trip compile-time kernels of the fused solver step for MI355X (gfx950): whole 2048-element chunks, 1-D grid,
// XCD-aware chunk map, paced load issue.  Bit-identical to the grid-stride / general kernels of skr_step.hip.
#include "skr_step_common.h"

namespace skr {

// ---- one-trip kernels: loads first, XCD-aware chunk map ------------------------------------------------
// Launches made of whole 2048-element chunks (every BASELINE config) take these.  One workgroup = one chunk of
// BLOCK lane-vectors, one trip, exactly numel/2048 workgroups on a 1-D grid:
//  * the operand pointers are the first thing read from the kernarg and the K loads are issued right behind them;
//    everything else the wave needs (seed, Philox key schedule, coefficients) is fetched while they are in flight.
//    (The grid-stride kernels above read geometry -> seed pointer -> seed -> key schedule before their first load:
//    three dependent scalar round trips per wave, 0.7 us on the 26 us headline launch.)
//  * chunk map: workgroups b and b+8 run on the same XCD (round-robin dispatch), so with the identity map every XCD
//    walks the tensor with a stride of 8 chunks.  The map hands each XCD runs of 2^lr consecutive chunks inside every
//    group of 8 runs: -0.2..0.3 us on the headline launch (tools/tune/tune_r2.hip).
// Arithmetic, lane ownership and Philox block numbering are exactly those of step_kernel_k / step_kernel_rk, so the
// results are bit-identical (tests/test_step_gpu.py::test_one_trip_kernels_agree_bitwise).
// Kernarg of the one-trip kernel: what the first instructions need (pointers, chunk map) leads, and launches of <= 4
// operands carry a 2-line block instead of 3 (every CU's scalar cache misses each line once per launch).
template <int KMAX>
struct OneTripArgs {
  const void* in[KMAX];
  void* out0;
  const uint64_t* seeds;
  int32_t xmap_lr;      // log2(run length) of the XCD chunk map
  int32_t bps_shift;    // log2(blocks per sample)
  uint64_t stream0;
  float c0[KMAX];
  float zeta0;
  RowRef tab;
};

// (chunk -> sample: sample_of; the rolling form's row and its present operands: rolling_row / row_has -- all three in skr_step_common.h,
//  shared with the masked step kernels of skr_step_masked.hip)

// The three kernels take the launch's RowForm (skr_step_common.h) as a template argument F.  WholeBatch and PerSample fetch their
// scalars from a row behind the loads (row_behind_loads(F)); per-sample rows (skr_step_launch_indexed_per_sample) are the whole-batch
// form with the row chosen by the workgroup's sample (tests/test_per_sample_isa.py compares the two).
// Rolling batches (skr_step_launch_rolling): RowForm::Rolling.  Per-sample rows in which a workgroup first asks its own sample's
// index entry and row what to touch: a negative entry ends the workgroup before its first vector-memory instruction, and an operand
// whose two coefficients are zero in the row is neither loaded nor accumulated (the history a sample in its multistep ramp-up does not
// have yet -- its bytes are the slot's previous occupant's, possibly NaN, and fma(0, NaN, s) is NaN).  The row is uniform over the
// workgroup, so every such decision is a scalar branch.  The row fetch therefore stands IN FRONT of the loads here, the order the
// other forms avoid (see step_kernel_k1): two dependent scalar round trips per wave, measured in tools/bench_rolling.py.

// The device-resident row of chunk c (WholeBatch and PerSample instantiations).  PER_SAMPLE: index holds one entry per sample and a workgroup reads its
// own sample's -- launches of whole chunks per sample only, so the sample, and with it the row, zeta and the draw / no-draw branch,
// is uniform over the workgroup.  The sample id goes through readfirstlane (the dividing form of sample_of runs on the vector ALU):
// the index fetch and the row fetch stay scalar loads, two dependent ones as in the whole-batch form.  No bounds check, no clamp.
template <bool PER_SAMPLE>
__device__ __forceinline__ const skr_step_row* row_at(const RowRef& r, uint32_t c, int32_t bps_shift) {
  if constexpr (PER_SAMPLE) {
    // sample_of without its branch: ahead of the row fetch a branch made the compiler hoist the division above the operand loads
    // and issue them once per arm.  Shift and divide instead (one of the two is by 0 / by 1): ~25 scalar-path instructions behind the loads.
    const uint32_t smp = (c >> (bps_shift < 0 ? 0 : bps_shift)) / (bps_shift < 0 ? (uint32_t)(-bps_shift) : 1u);
    // (the NULL test of row_of is kept although the entry point refuses a NULL index: the branch ends the basic block where the
    //  whole-batch form ends it, and instruction selection, which works block by block, then gives both forms the same registers --
    //  as one block, ten instantiations of 11+ operands took up to 25 more VGPRs and lost one to three waves per SIMD)
    return r.rows + ((r.index != nullptr ? r.index[__builtin_amdgcn_readfirstlane(smp)] : 0) + r.row_offset);
  } else {
    return row_of(r);
  }
}

// Rolling form: one operand's terms, added in two halves of four elements.  In this form every operand is summed in a block of its
// own, with the sums AND every operand still to come live across it; widened eight elements at a time, the eight temporaries on top of
// that cost the fp16 instantiations of 10+ operands one wave per SIMD against their per-sample forms (fp16 only: its conversions are the ones the compiler batches).  The empty asm statement ties the
// second half's conversions behind the first half's sums (it "rewrites" the raw registers and those sums), so four temporaries are live
// at a time.  Element by element the arithmetic is what it was.
template <typename T>
__device__ __forceinline__ void tie_halves(Raw<T>& r, float* a, float* b) {
  if constexpr (sizeof(T) == 2) asm volatile("" : "+v"(r.q), "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]));
  else asm volatile("" : "+v"(r.q[0]), "+v"(r.q[1]), "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]));
}
template <typename T>
__device__ __forceinline__ void add_operand(Raw<T>& r, float c, float s[VEC]) {
  float lo[VEC], hi[VEC];
  widen<T, float>(r, lo);
  if constexpr (!std::is_same<T, f16_t>::value) {  // (bf16 widens with a shift or a mask per element and fp32 not at all: tying them only costs registers)
#pragma unroll
    for (int i = 0; i < VEC; ++i) s[i] = fma_(c, lo[i], s[i]);
    return;
  }
#pragma unroll
  for (int i = 0; i < VEC / 2; ++i) s[i] = fma_(c, lo[i], s[i]);
  if constexpr (sizeof(T) == 2) asm volatile("" : "+v"(r.q), "+v"(s[0]), "+v"(s[1]), "+v"(s[2]), "+v"(s[3]));
  else asm volatile("" : "+v"(r.q[0]), "+v"(r.q[1]), "+v"(s[0]), "+v"(s[1]), "+v"(s[2]), "+v"(s[3]));
  widen<T, float>(r, hi);
#pragma unroll
  for (int i = VEC / 2; i < VEC; ++i) s[i] = fma_(c, hi[i], s[i]);
}
template <typename T>
__device__ __forceinline__ void add_operand2(Raw<T>& r, float c0, float c1, float s0[VEC], float s1[VEC]) {
  float lo[VEC], hi[VEC];
  widen<T, float>(r, lo);
  if constexpr (!std::is_same<T, f16_t>::value) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) s0[i] = fma_(c0, lo[i], s0[i]);
#pragma unroll
    for (int i = 0; i < VEC; ++i) s1[i] = fma_(c1, lo[i], s1[i]);
    return;
  }
#pragma unroll
  for (int i = 0; i < VEC / 2; ++i) s0[i] = fma_(c0, lo[i], s0[i]);
#pragma unroll
  for (int i = 0; i < VEC / 2; ++i) s1[i] = fma_(c1, lo[i], s1[i]);
  tie_halves<T>(r, s0, s1);
  widen<T, float>(r, hi);
#pragma unroll
  for (int i = VEC / 2; i < VEC; ++i) s0[i] = fma_(c0, hi[i], s0[i]);
#pragma unroll
  for (int i = VEC / 2; i < VEC; ++i) s1[i] = fma_(c1, hi[i], s1[i]);
}

// kernarg sizes: 4 / 8 / 12 / 16 / 20 operand slots (Adams-Bashforth 5-9 and UniP >= 5 give 10-18 operands: round 3)
constexpr int one_trip_kmax(int k) { return k <= 4 ? 4 : (k <= 8 ? 8 : (k <= 12 ? 12 : (k <= 16 ? 16 : 20))); }
constexpr int ONE_TRIP_MAX_K = 20;

template <typename T, int K, bool NOISE, bool TILE, bool PACE, RowForm F>
__global__ __launch_bounds__(BLOCK) void step_kernel_k1(const OneTripArgs<one_trip_kmax(K)> a) {
  const uint32_t c = chunk_of(blockIdx.x, a.xmap_lr);
  const int64_t v = (int64_t)c * BLOCK + threadIdx.x;
  if constexpr (F == RowForm::Rolling) {
    uint32_t smp, within;
    const skr_step_row* row = rolling_row(a.tab, c, a.bps_shift, smp, within);
    if (row == nullptr) return;  // inactive sample: nothing read, nothing written
    bool on[K];
    double cd[K];  // (converted to float where they are used: the doubles sit in SGPRs, the floats would be K VGPRs live across the loads)
#pragma unroll
    for (int j = 0; j < K; ++j) { on[j] = row_has(row, j); cd[j] = row->coef0[j]; }
    const float zeta0 = (float)row->zeta0;
    const uint64_t stream0 = row->stream0;
    // (each operand's pointer is fetched from the kernarg inside its branch -- one scalar round trip in front of its load.  Pinning the
    //  pointers in SGPRs ahead of the branches with an asm statement made them generic pointers and the loads flat_load: left as it is)
    // (16-bit launches of more than 12 operands keep 12 loads in flight: operand j + 12 is loaded where operand j has been summed, into
    //  the registers that frees -- with all of them in flight the 13-16-operand fp16 forms are a wave per SIMD below their per-sample forms)
    constexpr int AHEAD = (sizeof(T) == 2 && K > 12) ? 12 : K;
    Raw<T> raw[K];
#pragma unroll
    for (int j = 0; j < AHEAD; ++j) if (on[j]) raw[j] = load_raw<T, TILE>(a.in[j], v);
    float z[VEC];
    bool n0 = false;
    if constexpr (NOISE) {
      n0 = zeta0 != 0.f;
      if (n0) {
        const uint64_t seed = a.seeds[smp];
        const uint32_t vs = within * BLOCK + threadIdx.x;
        normal4(seed, stream0, (uint64_t)group0<TILE>((int64_t)vs), z);
        normal4(seed, stream0, (uint64_t)group1<TILE>((int64_t)vs), z + 4);
      }
    }
    float s[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) s[i] = 0.f;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      if (on[j]) add_operand<T>(raw[j], (float)cd[j], s);  // present operands in slot order: the bits of the narrower launch that holds exactly these
      if constexpr (AHEAD < K) {
        if (j + AHEAD < K) { if (on[j + AHEAD]) raw[j + AHEAD] = load_raw<T, TILE>(a.in[j + AHEAD], v); }
      }
    }
    if constexpr (NOISE) { if (n0) fma_noise8<float>(zeta0, z, s); }
    store8<T, float, TILE>(a.out0, v, s);
    return;
  }
  Raw<T> raw[K];
  float z[VEC];
  // The step's scalars come from the kernarg or, in the WholeBatch and PerSample instantiations (indexed launches), from the device-resident row
  // (two dependent scalar loads).  They are fetched AFTER the first global loads have been issued, and the choice is a
  // template parameter: as a run-time branch in front it put three scalar round trips before the first load of every wave
  // (+0.3 us on the headline launch), and the compiler sank the loads behind the branch wherever it stood.
  float cf[K], zeta0;
  uint64_t stream0;
#define SKR_SCALARS()                                                        \
  __builtin_amdgcn_sched_barrier(0);                                         \
  zeta0 = a.zeta0; stream0 = a.stream0;                                      \
  _Pragma("unroll") for (int j = 0; j < K; ++j) cf[j] = a.c0[j];             \
  if constexpr (row_behind_loads(F)) {                                       \
    const skr_step_row* row = row_at<per_sample_rows(F)>(a.tab, c, a.bps_shift); \
    _Pragma("unroll") for (int j = 0; j < K; ++j) cf[j] = (float)row->coef0[j]; \
    zeta0 = (float)row->zeta0;                                               \
    stream0 = row->stream0;                                                  \
  }
  // Paced issue.  One burst of K loads per wave is not the fastest order on this memory system: on the headline
  // launch (tools/tune/tune_r2.hip, 256x4x128x128 bf16, K = 4) all loads first runs 26.3 us, loads after the Philox
  // set-up 27.0 us, and the loads spread over the wave's Philox work -- one before the seed fetch, one after it, one
  // after each Philox block -- 25.9 us; without noise, ~1000 idle clocks (s_sleep 16) between the loads of a
  // 4-operand launch give 25.6 instead of 26.1 us (no gain measured for 2-output or 7/8-operand launches, which stay
  // unpaced).  The order is pinned by data dependencies: each later load takes its lane-vector index from an empty
  // asm statement that sits behind the work it has to follow (volatile asm statements keep their order), and
  // sched_barrier stops the machine scheduler from regrouping the segments.
  if constexpr (NOISE && PACE) {
    int64_t vj = v;
#define SKR_ISSUE(SLOT)                                                                      \
    _Pragma("unroll") for (int j = 0; j < K; ++j)                                            \
      if ((j * 4) / K == SLOT) raw[j] = load_raw<T, TILE>(a.in[j], vj);                      \
    __builtin_amdgcn_sched_barrier(0)
    SKR_ISSUE(0);
    SKR_ISSUE(1);  // (both before the wave parks on its scalar fetches: holding the second one back behind them cost 0.3 us)
    SKR_SCALARS();
    uint32_t smp, within;
    sample_of(c, a.bps_shift, smp, within);
    const uint64_t seed = a.seeds[smp];
    uint32_t vs = within * BLOCK + threadIdx.x;  // lane-vector within the sample
    normal4(seed, stream0, (uint64_t)group0<TILE>((int64_t)vs), z);
    asm volatile("" : "+v"(vj), "+v"(vs) : "v"(z[0]), "v"(z[1]), "v"(z[2]), "v"(z[3]));  // ... behind the first block
    __builtin_amdgcn_sched_barrier(0);
    SKR_ISSUE(2);
    normal4(seed, stream0, (uint64_t)group1<TILE>((int64_t)vs), z + 4);
    asm volatile("" : "+v"(vj) : "v"(z[4]), "v"(z[5]), "v"(z[6]), "v"(z[7]));           // ... behind the second
    __builtin_amdgcn_sched_barrier(0);
    SKR_ISSUE(3);
#undef SKR_ISSUE
    // the operands are first touched here: left alone, the compiler starts unpacking the early ones between the
    // segments and parks the wave on their arrival (microseconds under load) before the later loads are issued
#pragma unroll
    for (int j = 0; j < K; ++j) pin_raw(raw[j]);
  } else if constexpr (NOISE) {  // unpaced: every load first, then the Philox work
#pragma unroll
    for (int j = 0; j < K; ++j) raw[j] = load_raw<T, TILE>(a.in[j], v);
    SKR_SCALARS();
    uint32_t smp, within;
    sample_of(c, a.bps_shift, smp, within);
    const uint64_t seed = a.seeds[smp];
    const uint32_t vs = within * BLOCK + threadIdx.x;
    normal4(seed, stream0, (uint64_t)group0<TILE>((int64_t)vs), z);
    normal4(seed, stream0, (uint64_t)group1<TILE>((int64_t)vs), z + 4);
  } else if constexpr (PACE && (K == 4 || K == 5)) {  // tools/bench_plan.py: K=4 -1.1 %, K=5 -1.7 %, K=3 +6 % (left unpaced), K>=6 no change
    int64_t vj = v;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      raw[j] = load_raw<T, TILE>(a.in[j], vj);
      if (j < K - 1) {
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_sleep 16" : "+v"(vj));
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    SKR_SCALARS();
  } else {
#pragma unroll
    for (int j = 0; j < K; ++j) raw[j] = load_raw<T, TILE>(a.in[j], v);
    SKR_SCALARS();
  }
#undef SKR_SCALARS
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
  if constexpr (NOISE) { if (zeta0 != 0.f) fma_noise8<float>(zeta0, z, s); }  // (a zero row skips the draw, as a launch without noise does)
  store8<T, float, TILE>(a.out0, v, s);
}

// Kernarg of the one-trip Runge-Kutta stage kernel: as for step_kernel_k1, everything the first instructions need -- the
// operand pointers, the chunk map, both output pointers -- leads, and stages of <= 4 operands have all of it in the first
// 64-byte line (round 2's RkArgs kept xmap_lr in the third line, behind the coefficients: the first load of every wave
// waited for two scalar lines instead of one; tools/tune/tune_r3.hip "lib": K=2 24.05 -> 23.1 us, K=5 38.97 -> 37.8 us).
template <int KMAX>
struct RkOneTripArgs {
  const void* in[KMAX];
  void* out0;
  void* out1;
  const uint64_t* seeds;
  int32_t xmap_lr;
  int32_t bps_shift;
  float c1[KMAX];
  float chain;
  float ck[4];
  int32_t conv_to, conv_from;
  float zeta1;
  uint64_t stream1;
  RowRef tab;
};

// NOISE: the step's last stage of a stochastic tableau step adds zeta1 * N(stream1) to out1 (the derivative out0 is never noisy)
// BLK: threads per workgroup (256, or 128 = 1024-element chunks: tools/tune/tune_r3.hip measured the 5-operand stage 1-4 % faster so)
template <typename T, int K, bool TILE, bool NOISE, RowForm F, int BLK>
__global__ __launch_bounds__(BLK) void step_kernel_rk1(const RkOneTripArgs<(K <= 4 ? 4 : 8)> a) {
  const uint32_t c = chunk_of(blockIdx.x, a.xmap_lr);
  const int64_t v = (int64_t)c * BLK + threadIdx.x;
  // Rolling form: the inactive exit, and the operands behind the conversion pair that the row lacks are neither loaded nor summed (the
  // contract of skr_step_launch_rolling; a Runge-Kutta step has no ramp-up, so the samplers' own rows lack none)
  [[maybe_unused]] const skr_step_row* rolling = nullptr;
  [[maybe_unused]] bool on[K];
  if constexpr (F == RowForm::Rolling) {
    uint32_t smp, within;
    rolling = rolling_row(a.tab, c, a.bps_shift, smp, within);
    if (rolling == nullptr) return;
#pragma unroll
    for (int j = 0; j < K; ++j) on[j] = j < 2 || row_has(rolling, j);
  }
  Raw<T> raw[K];
  if constexpr (F == RowForm::Rolling) {
#pragma unroll
    for (int j = 0; j < K; ++j) if (on[j]) raw[j] = load_raw<T, TILE>(a.in[j], v);
  } else {
#pragma unroll
    for (int j = 0; j < K; ++j) raw[j] = load_raw<T, TILE>(a.in[j], v);
  }
  __builtin_amdgcn_sched_barrier(0);  // every load is out before the first scalar of the arithmetic is fetched
  float k[4] = {a.ck[0], a.ck[1], a.ck[2], a.ck[3]}, cf[K], chain = a.chain, zeta1 = a.zeta1;
  uint64_t stream1 = a.stream1;
#pragma unroll
  for (int j = 0; j < K; ++j) cf[j] = a.c1[j];
  if constexpr (has_table(F)) {
    const skr_step_row* row;
    if constexpr (F == RowForm::Rolling) row = rolling; else row = row_at<per_sample_rows(F)>(a.tab, c, a.bps_shift);
#pragma unroll
    for (int j = 0; j < K; ++j) cf[j] = (float)row->coef1[j];
#pragma unroll
    for (int i = 0; i < 4; ++i) k[i] = (float)row->convert_k[i];
    chain = (float)row->chain;
    zeta1 = (float)row->zeta1;
    stream1 = row->stream1;
  }
  float z1[VEC];
  bool n1 = false;
  if constexpr (NOISE) {
    n1 = zeta1 != 0.f;
    if (n1) {
      uint32_t smp, within;
      sample_of(c, a.bps_shift, smp, within);
      const uint64_t seed = a.seeds[smp];
      const uint32_t vs = within * BLK + threadIdx.x;
      normal4(seed, stream1, (uint64_t)group0<TILE>((int64_t)vs), z1);
      normal4(seed, stream1, (uint64_t)group1<TILE>((int64_t)vs), z1 + 4);
    }
  }
  float sv[VEC], ov[VEC], d[VEC], s1[VEC];
  widen<T, float>(raw[0], sv);
  widen<T, float>(raw[1], ov);
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    d[i] = convert_rounded<T, float>(sv[i], ov[i], a.conv_to, a.conv_from, k);
    s1[i] = fma_(cf[1], ov[i], fma_(cf[0], sv[i], 0.f));
  }
#pragma unroll
  for (int j = 2; j < K; ++j) {
    if constexpr (F == RowForm::Rolling) { if (!on[j]) continue; }
    float w[VEC];
    widen<T, float>(raw[j], w);
    const float cj = cf[j];
#pragma unroll
    for (int i = 0; i < VEC; ++i) s1[i] = fma_(cj, w[i], s1[i]);
  }
#pragma unroll
  for (int i = 0; i < VEC; ++i) s1[i] = fma_(chain, d[i], s1[i]);
  if constexpr (NOISE) { if (n1) fma_noise8<float>(zeta1, z1, s1); }
  store8<T, float, TILE>(a.out1, v, s1);
  store8<T, float, TILE>(a.out0, v, d);
}

// one-trip launches: whole chunks, and with in-kernel noise samples made of whole chunks (any number of them)
// (per-sample rows: a workgroup must belong to one sample with or without noise; table launches have no other kernel, so the
//  one_trip switch does not apply to them)
static bool one_trip_ok(int64_t numel, int64_t sample_numel, bool noise, RowForm form, int* bps_shift) {
  constexpr int64_t CHUNK = (int64_t)BLOCK * VEC;
  if ((!g_tune.one_trip && !has_table(form)) || numel % CHUNK != 0 || numel / CHUNK > 0x7fffffffll) return false;
  *bps_shift = 0;
  if (!noise && !per_sample_rows(form)) return true;
  if (sample_numel % CHUNK != 0) return false;
  const int64_t bps = sample_numel / CHUNK;
  if (bps > 0x3fffffffll) return false;
  *bps_shift = bps_shift_of(bps);
  return true;
}
// fp32 launches use the tile layout; with the tile switch off they are left to the other kernels, which table launches do not have
template <typename T> static bool tile_switched_off(RowForm form) { return sizeof(T) == 4 && !g_tune.tile && !has_table(form); }

// ---- host side ---------------------------------------------------------------------------------------------------
// The one place that maps a launch form to a kernel instantiation: calls
// f(type_tag<T>{}, bool_c<PACE>{}, std::integral_constant<RowForm, F>{}) with the template arguments of the kernel this form runs.
//   form        PACE
//   Kernarg     g_tune.pace where PACED, else false
//   WholeBatch  PACED
//   PerSample   PACED
//   Rolling     false
// PACED: this operand count has a paced instantiation (1-8-operand k1, noisy 2-11-operand k2; step_kernel_rk1 has no such parameter).
// TABLE: it has table instantiations (its operands fit a device-resident row); false is returned for a table form without one.
template <typename T, bool PACED, bool TABLE, typename Fn>
static bool with_form(RowForm form, Fn&& f) {
  if (!TABLE && has_table(form)) return false;
  with_row_form(form, [&](auto fm) {
    constexpr RowForm F = decltype(fm)::value;
    if constexpr (F == RowForm::Kernarg) {
      if (PACED && g_tune.pace) f(type_tag<T>{}, bool_c<PACED>{}, fm);
      else f(type_tag<T>{}, bool_c<false>{}, fm);
    } else if constexpr (TABLE) {
      f(type_tag<T>{}, bool_c<PACED && F != RowForm::Rolling>{}, fm);
    }
  });
  return true;
}

template <typename T, bool NOISE>
static int launch_k1(const StepArgs<float>& args, int bps_shift, hipStream_t stream) {
  constexpr bool TILE = sizeof(T) == 4;  // whole chunks are whole tiles
  const int64_t chunks = args.numel / ((int64_t)BLOCK * VEC);
  bool launched = true;
  with_count<1, ONE_TRIP_MAX_K>(args.n_terms, [&](auto n) {
    constexpr int N = decltype(n)::value;
    OneTripArgs<one_trip_kmax(N)> fa;
    fill_operands(args.in, args.c0, N, fa.in, fa.c0);
    fa.out0 = args.out0; fa.seeds = args.seeds; fa.zeta0 = args.zeta0; fa.stream0 = args.stream0;
    fa.bps_shift = bps_shift; fa.xmap_lr = xmap_lr_for(chunks);
    fa.tab = RowRef{args.rows, args.index, args.row_offset};
    // more than 8 operands: one unpaced instantiation each (plus the table forms while the operands fit a device-resident row)
    launched = with_form<T, (N <= 8), (N <= SKR_ROW_TERMS)>(args.form, [&](auto tt, auto pace, auto fm) {
      hipLaunchKernelGGL((step_kernel_k1<typename decltype(tt)::type, N, NOISE, TILE, decltype(pace)::value, decltype(fm)::value>), dim3((unsigned)chunks), dim3(BLOCK), 0, stream, fa);
    });
  });
  return launched ? finish_launch() : SKR_ERR_UNSUPPORTED;
}

template <typename T>
int launch_one_trip_k(const StepArgs<float>& args, bool noise, hipStream_t stream, bool& taken) {
  taken = false;
  int bps_shift = 0;
  if (!one_trip_ok(args.numel, args.sample_numel, noise, args.form, &bps_shift) || tile_switched_off<T>(args.form)) return SKR_OK;
  if (args.n_terms > ONE_TRIP_MAX_K) return SKR_OK;
  taken = true;
  return noise ? launch_k1<T, true>(args, bps_shift, stream) : launch_k1<T, false>(args, bps_shift, stream);
}
template int launch_one_trip_k<bf16_t>(const StepArgs<float>&, bool, hipStream_t, bool&);
template int launch_one_trip_k<f16_t>(const StepArgs<float>&, bool, hipStream_t, bool&);
template int launch_one_trip_k<float>(const StepArgs<float>&, bool, hipStream_t, bool&);

template <typename T, bool NOISE, int BLK>
static int launch_rk1(const StepArgs<float>& args, unsigned chunks, int bps_shift, hipStream_t stream) {
  constexpr bool TILE = sizeof(T) == 4;
  if constexpr (BLK == 128) {  // half-size chunks: twice as many of them, per sample too
    chunks *= 2;
    bps_shift = bps_shift >= 0 ? bps_shift + 1 : 2 * bps_shift;
  }
  with_count<2, 8>(args.n_terms, [&](auto n) {
    constexpr int N = decltype(n)::value;
    RkOneTripArgs<(N <= 4 ? 4 : 8)> ra;
    fill_operands(args.in, args.c1, N, ra.in, ra.c1);
    ra.seeds = args.seeds; ra.zeta1 = args.zeta1; ra.stream1 = args.stream1; ra.bps_shift = bps_shift;
    ra.out0 = args.out0; ra.out1 = args.out1; ra.chain = args.chain;
    for (int i = 0; i < 4; ++i) ra.ck[i] = (float)args.ck[i];
    ra.conv_to = args.conv_to; ra.conv_from = args.conv_from; ra.xmap_lr = xmap_lr_for(chunks); ra.tab = RowRef{args.rows, args.index, args.row_offset};
    with_form<T, false, true>(args.form, [&](auto tt, auto, auto fm) {
      hipLaunchKernelGGL((step_kernel_rk1<typename decltype(tt)::type, N, TILE, NOISE, decltype(fm)::value, BLK>), dim3(chunks), dim3(BLK), 0, stream, ra);
    });
  });
  return finish_launch();
}

template <typename T>
int launch_one_trip_rk(const StepArgs<float>& args, bool noise, hipStream_t stream, bool& taken) {
  taken = false;
  int bps_shift = 0;
  if (!one_trip_ok(args.numel, args.sample_numel, noise, args.form, &bps_shift) || tile_switched_off<T>(args.form)) return SKR_OK;
  if (noise && !has_table(args.form) && args.zeta0 != 0.f) return SKR_OK;  // (a noisy derivative does not occur; left to the general kernel)
  taken = true;
  const unsigned chunks = (unsigned)(args.numel / ((int64_t)BLOCK * VEC));
  // 128-thread workgroups for the 2-6 operand stages (tools/bench_plan.py rk, same box: K=4 33.5 vs 34.0 us, K=5 38.7 vs 39.8, K=6 43.7 vs
  // 45.2, K >= 7 unchanged; round 4, A/B/A/B on one box, profiles/r04_bench_plan_ab.txt: K=2 23.6-23.8 vs 24.1-24.2 us, K=3 29.16-29.26 vs
  // 29.17-29.30 -- round 3 had read K=2 / 3 as 1-2 % slower from runs on different boxes); rk_blk = 128 / 256 forces one size
  const bool small_blocks = g_tune.rk_blk == 128 || (g_tune.rk_blk == 0 && args.n_terms <= 6);
  if (small_blocks && chunks < 0x40000000u && bps_shift > -0x20000000)
    return noise ? launch_rk1<T, true, 128>(args, chunks, bps_shift, stream) : launch_rk1<T, false, 128>(args, chunks, bps_shift, stream);
  return noise ? launch_rk1<T, true, 256>(args, chunks, bps_shift, stream) : launch_rk1<T, false, 256>(args, chunks, bps_shift, stream);
}
template int launch_one_trip_rk<bf16_t>(const StepArgs<float>&, bool, hipStream_t, bool&);
template int launch_one_trip_rk<f16_t>(const StepArgs<float>&, bool, hipStream_t, bool&);
template int launch_one_trip_rk<float>(const StepArgs<float>&, bool, hipStream_t, bool&);

// ---- two outputs (UniPC / SPC steps): out0 fp32 state, out1 = chain*out0 + ... in the operands' 16-bit dtype ---------
//   out0 = sum_k c0[k]*in_k + zeta0*N(stream0)          NA 16-bit operands, then NB (0 or 1) fp32 operand
//   out1 = chain*out0 + sum_k c1[k]*in_k + zeta1*N(stream1)
// Same FMA order, zero-zeta guards, tile layout and Philox numbering as step_kernel<..., HAS1, TILE = true>, so the bits
// are the same; what changes is that every pointer and coefficient is in SGPRs before the first load, the term list is
// a template constant and the launch is one trip over an XCD-mapped 1-D grid.
template <int NMAX>
struct TwoOutArgs {
  const void* in[NMAX];
  void* out0;
  void* out1;
  const uint64_t* seeds;
  int32_t xmap_lr, bps_shift;
  uint64_t stream0, stream1;
  float chain, zeta0, zeta1;
  float c0[NMAX];
  float c1[NMAX];
  RowRef tab;
};
// operand count from which the no-noise two-output launches store non-temporally.  Round-4 A/B/A/B through the library on one box
// (tools/bench_plan.py ab, profiles/r04_bench_plan_ab.txt): 8 + 1 operands 294.0-295.1 us vs 299.4-299.9 us with write-through stores,
// 10 + 1 (BASELINE config 3 with Colored noise tensors) 338.2-338.5 vs 346.0-346.1 us
constexpr int NT_FROM_OPERANDS = 9;
constexpr int two_out_nmax(int n) { return n <= 4 ? 4 : (n <= 8 ? 8 : (n <= 12 ? 12 : (n <= 16 ? 16 : (n <= 20 ? 20 : 24)))); }

template <typename TA, int NA, int NB, bool NOISE, bool PACE, RowForm F, bool NT = false>
__global__ __launch_bounds__(BLOCK) void step_kernel_k2(const TwoOutArgs<two_out_nmax(NA + NB)> a) {
  const uint32_t c = chunk_of(blockIdx.x, a.xmap_lr);
  const int64_t v = (int64_t)c * BLOCK + threadIdx.x;
  if constexpr (F == RowForm::Rolling) {  // see step_kernel_k1: inactive exit, absent operands skipped, present ones in slot order
    uint32_t smp, within;
    const skr_step_row* row = rolling_row(a.tab, c, a.bps_shift, smp, within);
    if (row == nullptr) return;
    bool on[NA + NB];
    double cd0[NA + NB], cd1[NA + NB];  // (converted where they are used, see step_kernel_k1)
#pragma unroll
    for (int j = 0; j < NA + NB; ++j) { on[j] = row_has(row, j); cd0[j] = row->coef0[j]; cd1[j] = row->coef1[j]; }
    const float chain = (float)row->chain, zeta0 = (float)row->zeta0, zeta1 = (float)row->zeta1;
    const uint64_t stream0 = row->stream0, stream1 = row->stream1;
    Raw<TA> ra[NA];
    Raw<float> rb[NB > 0 ? NB : 1];
#pragma unroll
    for (int j = 0; j < NA; ++j) if (on[j]) ra[j] = load_raw<TA, true>(a.in[j], v);
#pragma unroll
    for (int j = 0; j < NB; ++j) if (on[NA + j]) rb[j] = load_raw<float, true>(a.in[NA + j], v);
    float z0[VEC], z1[VEC];
    bool n0 = false, n1 = false;
    if constexpr (NOISE) {
      n0 = zeta0 != 0.f;
      n1 = zeta1 != 0.f;
      if (n0 || n1) {
        const uint64_t seed = a.seeds[smp];
        const uint32_t vs = within * BLOCK + threadIdx.x;
        if (n0) { normal4(seed, stream0, (uint64_t)group0<true>((int64_t)vs), z0); normal4(seed, stream0, (uint64_t)group1<true>((int64_t)vs), z0 + 4); }
        if (n1) { normal4(seed, stream1, (uint64_t)group0<true>((int64_t)vs), z1); normal4(seed, stream1, (uint64_t)group1<true>((int64_t)vs), z1 + 4); }
      }
    }
    float s0[VEC], s1[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) { s0[i] = 0.f; s1[i] = 0.f; }
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      if (on[j]) add_operand2<TA>(ra[j], (float)cd0[j], (float)cd1[j], s0, s1);
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      if (on[NA + j]) add_operand2<float>(rb[j], (float)cd0[NA + j], (float)cd1[NA + j], s0, s1);
    }
    if constexpr (NOISE) { if (n0) fma_noise8<float>(zeta0, z0, s0); }
#pragma unroll
    for (int i = 0; i < VEC; ++i) s1[i] = fma_(chain, s0[i], s1[i]);
    if constexpr (NOISE) { if (n1) fma_noise8<float>(zeta1, z1, s1); }
    store8<TA, float, true, NT>(a.out1, v, s1);
    store8<float, float, true, NT>(a.out0, v, s0);
    return;
  }
  Raw<TA> ra[NA];
  Raw<float> rb[NB > 0 ? NB : 1];
  float z0[VEC], z1[VEC];
  bool n0 = false, n1 = false;
  float cf0[NA + NB], cf1[NA + NB], chain, zeta0, zeta1;  // kernarg or device-resident row, fetched behind the first loads
  uint64_t stream0, stream1;
#define SKR_SCALARS()                                                                      \
  __builtin_amdgcn_sched_barrier(0);                                                       \
  chain = a.chain; zeta0 = a.zeta0; zeta1 = a.zeta1; stream0 = a.stream0; stream1 = a.stream1; \
  _Pragma("unroll") for (int j = 0; j < NA + NB; ++j) { cf0[j] = a.c0[j]; cf1[j] = a.c1[j]; } \
  if constexpr (row_behind_loads(F)) {                                                     \
    const skr_step_row* row = row_at<per_sample_rows(F)>(a.tab, c, a.bps_shift);           \
    _Pragma("unroll") for (int j = 0; j < NA + NB; ++j) { cf0[j] = (float)row->coef0[j]; cf1[j] = (float)row->coef1[j]; } \
    chain = (float)row->chain; zeta0 = (float)row->zeta0; zeta1 = (float)row->zeta1;       \
    stream0 = row->stream0; stream1 = row->stream1;                                        \
  }
  if constexpr (NOISE && PACE) {
    // loads paced over the Philox work (see step_kernel_k1): six slots around the seed fetch and the four blocks
    int64_t vj = v;
#define SKR_ISSUE(SLOT)                                                                                   \
    _Pragma("unroll") for (int j = 0; j < NA; ++j)                                                        \
      if ((j * 6) / (NA + NB) == SLOT) ra[j] = load_raw<TA, true>(a.in[j], vj);                           \
    _Pragma("unroll") for (int j = 0; j < NB; ++j)                                                        \
      if (((NA + j) * 6) / (NA + NB) == SLOT) rb[j] = load_raw<float, true>(a.in[NA + j], vj);            \
    __builtin_amdgcn_sched_barrier(0)
    SKR_ISSUE(0);
    SKR_ISSUE(1);
    SKR_SCALARS();
    uint32_t smp, within;
    sample_of(c, a.bps_shift, smp, within);
    const uint64_t seed = a.seeds[smp];
    uint32_t vs = within * BLOCK + threadIdx.x;
    n0 = zeta0 != 0.f;
    n1 = zeta1 != 0.f;
    if (n0) normal4(seed, stream0, (uint64_t)group0<true>((int64_t)vs), z0);
    asm volatile("" : "+v"(vj), "+v"(vs));
    __builtin_amdgcn_sched_barrier(0);
    SKR_ISSUE(2);
    if (n0) normal4(seed, stream0, (uint64_t)group1<true>((int64_t)vs), z0 + 4);
    asm volatile("" : "+v"(vj), "+v"(vs));
    __builtin_amdgcn_sched_barrier(0);
    SKR_ISSUE(3);
    if (n1) normal4(seed, stream1, (uint64_t)group0<true>((int64_t)vs), z1);
    asm volatile("" : "+v"(vj), "+v"(vs));
    __builtin_amdgcn_sched_barrier(0);
    SKR_ISSUE(4);
    if (n1) normal4(seed, stream1, (uint64_t)group1<true>((int64_t)vs), z1 + 4);
    asm volatile("" : "+v"(vj));
    __builtin_amdgcn_sched_barrier(0);
    SKR_ISSUE(5);
#undef SKR_ISSUE
#pragma unroll
    for (int j = 0; j < NA; ++j) pin_raw(ra[j]);
#pragma unroll
    for (int j = 0; j < NB; ++j) pin_raw(rb[j]);
  } else {
#pragma unroll
    for (int j = 0; j < NA; ++j) ra[j] = load_raw<TA, true>(a.in[j], v);
#pragma unroll
    for (int j = 0; j < NB; ++j) rb[j] = load_raw<float, true>(a.in[NA + j], v);
    SKR_SCALARS();
    if constexpr (NOISE) {
      uint32_t smp, within;
      sample_of(c, a.bps_shift, smp, within);
      const uint64_t seed = a.seeds[smp];
      const uint32_t vs = within * BLOCK + threadIdx.x;
      n0 = zeta0 != 0.f;
      n1 = zeta1 != 0.f;
      if (n0) { normal4(seed, stream0, (uint64_t)group0<true>((int64_t)vs), z0); normal4(seed, stream0, (uint64_t)group1<true>((int64_t)vs), z0 + 4); }
      if (n1) { normal4(seed, stream1, (uint64_t)group0<true>((int64_t)vs), z1); normal4(seed, stream1, (uint64_t)group1<true>((int64_t)vs), z1 + 4); }
    }
  }
#undef SKR_SCALARS
  float s0[VEC], s1[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) { s0[i] = 0.f; s1[i] = 0.f; }
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    float w[VEC];
    widen<TA, float>(ra[j], w);
    const float w0 = cf0[j], w1 = cf1[j];
#pragma unroll
    for (int i = 0; i < VEC; ++i) s0[i] = fma_(w0, w[i], s0[i]);
#pragma unroll
    for (int i = 0; i < VEC; ++i) s1[i] = fma_(w1, w[i], s1[i]);
  }
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    float w[VEC];
    widen<float, float>(rb[j], w);
    const float w0 = cf0[NA + j], w1 = cf1[NA + j];
#pragma unroll
    for (int i = 0; i < VEC; ++i) s0[i] = fma_(w0, w[i], s0[i]);
#pragma unroll
    for (int i = 0; i < VEC; ++i) s1[i] = fma_(w1, w[i], s1[i]);
  }
  if constexpr (NOISE) { if (n0) fma_noise8<float>(zeta0, z0, s0); }
#pragma unroll
  for (int i = 0; i < VEC; ++i) s1[i] = fma_(chain, s0[i], s1[i]);
  if constexpr (NOISE) { if (n1) fma_noise8<float>(zeta1, z1, s1); }
  store8<TA, float, true, NT>(a.out1, v, s1);
  store8<float, float, true, NT>(a.out0, v, s0);
}

// PACED, TABLE: see with_form.  NT: non-temporal stores, an instantiation of the kernarg form alone
template <typename TA, int NA, int NB, bool NOISE, bool PACED, bool TABLE, bool NT = false>
static int launch_k2(const StepArgs<float>& args, int bps_shift, hipStream_t stream) {
  const int64_t chunks = args.numel / ((int64_t)BLOCK * VEC);
  TwoOutArgs<two_out_nmax(NA + NB)> ta;
  fill_operands(args.in, args.c0, NA + NB, ta.in, ta.c0);
  fill_operands(args.in, args.c1, NA + NB, ta.in, ta.c1);
  ta.out0 = args.out0; ta.out1 = args.out1; ta.seeds = args.seeds;
  ta.xmap_lr = xmap_lr_for(chunks); ta.bps_shift = bps_shift;
  ta.stream0 = args.stream0; ta.stream1 = args.stream1;
  ta.chain = args.chain; ta.zeta0 = args.zeta0; ta.zeta1 = args.zeta1;
  ta.tab = RowRef{args.rows, args.index, args.row_offset};
  const bool launched = with_form<TA, PACED, TABLE && !NT>(args.form, [&](auto tt, auto pace, auto fm) {
    hipLaunchKernelGGL((step_kernel_k2<typename decltype(tt)::type, NA, NB, NOISE, decltype(pace)::value, decltype(fm)::value, NT>), dim3((unsigned)chunks), dim3(BLOCK), 0, stream, ta);
  });
  return launched ? finish_launch() : SKR_ERR_UNSUPPORTED;
}

// store policy of the no-noise two-output launches (see store8): "two_nt" 1 / 0 forces it, -1 = where it measured faster
static bool nt_stores(int operands) { return g_tune.two_nt >= 0 ? g_tune.two_nt != 0 : NT_FROM_OPERANDS > 0 && operands >= NT_FROM_OPERANDS; }

// TUNED: the operand counts whose load pacing (with noise) and store policy (without) were measured; the others run unpaced, write-through
template <typename TA, int NA, int NB, bool TUNED>
static int launch_k2_as(const StepArgs<float>& args, bool noise, int bps_shift, hipStream_t stream) {
  constexpr bool TABLE = NA + NB <= SKR_ROW_TERMS;
  if (noise) return launch_k2<TA, NA, NB, true, TUNED, TABLE>(args, bps_shift, stream);
  if constexpr (TUNED && NA + NB >= NT_FROM_OPERANDS) {
    if (!has_table(args.form) && nt_stores(NA + NB)) return launch_k2<TA, NA, NB, false, false, false, true>(args, bps_shift, stream);
  }
  return launch_k2<TA, NA, NB, false, false, TABLE>(args, bps_shift, stream);
}

// The operand counts the samplers emit (tools/trace_plans.py): UniPC / SPC of order n give 2n+2 (+2 with a noise tensor) 16-bit operands
// and the previous corrected state in fp32; their first steps have no fp32 operand yet.  From order 5 on (12 + 1 operands and more)
// nothing was tuned.
template <int NA, int NB, bool TUNED> struct TwoOut { static constexpr int na = NA, nb = NB; static constexpr bool tuned = TUNED; };
template <typename... C> struct TwoOutList {};
using TwoOutCounts = TwoOutList<TwoOut<2, 0, true>, TwoOut<3, 0, true>, TwoOut<4, 0, true>, TwoOut<4, 1, true>, TwoOut<6, 1, true>, TwoOut<7, 1, true>, TwoOut<8, 1, true>,
                                TwoOut<10, 1, true>, TwoOut<12, 1, false>, TwoOut<14, 1, false>, TwoOut<16, 1, false>, TwoOut<18, 1, false>, TwoOut<20, 1, false>,
                                TwoOut<22, 1, false>>;

// launches the first entry of the list that has these operand counts (`taken`); none: SKR_OK, nothing launched
template <typename TA, typename... C>
static int launch_k2_of(TwoOutList<C...>, int na, int nb, const StepArgs<float>& args, bool noise, int bps_shift, hipStream_t stream, bool& taken) {
  int rc = SKR_OK;
  (void)((na == C::na && nb == C::nb && (taken = true, rc = launch_k2_as<TA, C::na, C::nb, C::tuned>(args, noise, bps_shift, stream), true)) || ...);
  return rc;
}

template <typename TA>
int launch_one_trip_two(const StepArgs<float>& args, bool noise, bool group_b_f32, hipStream_t stream, bool& taken) {
  taken = false;
  const int na = args.n_a, nb = args.n_terms - args.n_a;
  const bool table = has_table(args.form);  // (a table launch has no other kernel to go to: the tuning switches below do not apply to it)
  if (nb > 1 || (nb == 1 && !group_b_f32) || ((!g_tune.tile || !g_tune.two_out) && !table)) return SKR_OK;
  // measured (tools/bench_plan.py, 256x16x128x128): with Philox and <= 7 operands the general kernel is 1-2 % faster
  // (193 vs 197 us at 4+1, 239 vs 241 us at 6+1); from 8+1 on, and without noise, this kernel wins (344 vs 365 us at 10+1)
  if (noise && na + nb <= 7 && g_tune.two_out != 2 && !table) return SKR_OK;
  int bps_shift = 0;
  if (!one_trip_ok(args.numel, args.sample_numel, noise, args.form, &bps_shift)) return SKR_OK;
  return launch_k2_of<TA>(TwoOutCounts{}, na, nb, args, noise, bps_shift, stream, taken);
}
template int launch_one_trip_two<bf16_t>(const StepArgs<float>&, bool, bool, hipStream_t, bool&);
template int launch_one_trip_two<f16_t>(const StepArgs<float>&, bool, bool, hipStream_t, bool&);

}  // namespace skr
