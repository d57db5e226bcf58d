// The step of adaptive projected guidance for rolling batches (include/skrample_hip.h, skr_projected_guided_step_launch_rolling):
// rows[index[slot] + row_offset] for the slots of a rolling.RollingBatch built with guided=True, projected=True.  A kernel of its own, not
// projected_rows_kernel_v1 with a flag: that kernel puts all K operand loads in front of the row fetch, and a rolling launch needs the
// opposite -- the row stands IN FRONT of the loads, as in guided_kernel_v1's and thresholded_rolling_kernel_v1's Rolling forms:
//   inactive slot    a negative index entry, tested before row_offset is added (rolling_row): the workgroup ends before its first
//                    vector-memory instruction; out, guided_out and the momentum buffer keep their bytes
//   the row          coef0[0 .. K), zeta0, stream0 and convert_k[3] (beta) are scalar loads; the K doubles stay in SGPRs and are narrowed
//                    where they are used (as floats they would be K VGPRs live across the loads and the Philox rounds)
//   other operands   present iff coef0 is not zero (guided_row_has): an absent one is neither loaded nor summed, so a request in its
//                    multistep ramp-up has the bits of the narrower direct launch that holds exactly its operands, whatever the history
//                    ring holds; present ones are summed from zero in slot order
//   the slot         always loaded, whatever its coefficient, from ONE base address chosen before the load: proj->diff on a momentum row
//                    (beta != +-0: the statistic has just stored d there, on the row a request's average starts on as on any other, so the
//                    step has no third case) and inputs[slot] on a zero-momentum row, whose d = rn_T(c - u) is formed in registers
//   cond             needs nothing of the row beyond "active": its load is issued first, ahead of the coefficient tests
//   A_s, B_s         coef[2 slot], coef[2 slot + 1]: two scalar loads through the constant address space (written by the statistics launch
//                    in front, read-only for this one), asked for behind the operand loads
//   the draw         a row whose zeta0 narrows to zero skips it on a uniform branch; the seed is seeds[slot], block numbers are local to
//                    the sample
//   wide launches    each operand's load sits behind its coefficient test, with its pointer fetched from the kernarg inside the branch.
//                    16-bit launches of more than 12 operands keep 12 images in flight (11 operands and cond), as
//                    projected_rows_ahead does; 32-bit launches of more than 4 operands stage their last two (4 operands: the last one):
//                    operand j + AHEAD is loaded where operand j has been summed, into the registers that frees.  A staged operand at
//                    `slot` takes the chosen base like any other.  No instantiation uses scratch, none is below the occupancy of its
//                    per-sample twin (profiles/projected_guidance_rolling_isa.txt)
// Lane ownership, the XCD chunk map, the fp32 tile layout, Philox numbering, projected_diff / projected_value and the fp32 accumulate and
// round are projected_kernel_v1's.  There is no guidance-only form and no grid-stride form: whole 2048-element chunks, proj->sample_numel
// a multiple of 2048 -- a workgroup lies inside one slot --, one 16- or 32-bit dtype, 1 .. 16 operands, single output, no rounded conversion.
#include "skr_projected.h"
#include "skr_step_guided_kernel.h"

namespace skr {

template <int KMAX>
struct ProjectedRollingArgs {  // (the layout of ProjectedRowArgs, skr_step_projected_rows.hip)
  const void* in[KMAX];  // in[slot]: uncond, loaded by the workgroups of a zero-momentum row
  const void* cond;
  const void* diff;      // the batch's buffer, loaded by the workgroups of a momentum row
  void* out;
  void* guided;          // nullptr: p is not stored
  int32_t xmap_lr;
  int32_t bps_shift;     // chunks per slot of the statistic (and of the draw)
  const uint64_t* seeds;
  const float* coef;     // [2 * slots]: A_s, B_s
  RowRef tab;
  int32_t slot;
};

template <typename T, int K>
constexpr int projected_rolling_ahead() {
  if (sizeof(T) == 2) return K > 12 ? 11 : K;
  return K > 4 ? K - 2 : (K > 3 ? K - 1 : K);
}

template <typename T, int K, bool NOISE>
__global__ __launch_bounds__(BLOCK) void projected_rolling_kernel_v1(const ProjectedRollingArgs<guided_kmax(K)> a) {
  constexpr bool TILE = sizeof(T) == 4;
  constexpr int AHEAD = projected_rolling_ahead<T, K>();
  const uint32_t c = chunk_of(blockIdx.x, a.xmap_lr);
  const int64_t v = (int64_t)c * BLOCK + threadIdx.x;
  uint32_t smp, within;
  const skr_step_row* row = rolling_row(a.tab, c, a.bps_shift, smp, within);
  if (row == nullptr) return;  // inactive slot: nothing read, nothing written
  const Raw<T> rc = load_raw<T, TILE>(a.cond, v);
  const int32_t slot = a.slot;
  bool on[K];
  double c0[K];
#pragma unroll
  for (int j = 0; j < K; ++j) { c0[j] = row->coef0[j]; on[j] = j == slot || guided_row_has(row, j); }
  const float zeta0 = (float)row->zeta0;
  const bool stored = rescaling(row->convert_k[3]);  // (uniform) beta != +-0: d is the buffer's; otherwise it is formed from uncond
  const uint64_t stream0 = row->stream0;
  // (each operand's pointer is fetched from the kernarg inside its branch, as in step_kernel_k1; the slot's is one of two)
  Raw<T> raw[K];
#pragma unroll
  for (int j = 0; j < AHEAD; ++j) if (on[j]) raw[j] = load_raw<T, TILE>((j == slot && stored) ? a.diff : a.in[j], v);
  const float A = uniform(a.coef)[2 * smp], B = uniform(a.coef)[2 * smp + 1];
  float z[VEC];
  [[maybe_unused]] bool n0 = false;
  if constexpr (NOISE) {
    n0 = zeta0 != 0.f;
    if (n0) {  // (uniform: the row's)
      const uint32_t vs = within * BLOCK + threadIdx.x;  // lane-vector within the slot (sample_numel < 2^31)
      const uint64_t seed = a.seeds[smp];
      normal4(seed, stream0, (uint64_t)group0<TILE>((int64_t)vs), z);
      normal4(seed, stream0, (uint64_t)group1<TILE>((int64_t)vs), z + 4);
    }
  }
  float acc[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    if (on[j]) {  // (uniform: the row's) present operands in slot order: the bits of the narrower launch that holds exactly these
      float w[VEC];
      widen<T, float>(raw[j], w);
      if (j == slot) {  // (uniform) the difference, or uncond, stands here: the projected prediction takes its place
        float cf[VEC];
        widen<T, float>(rc, cf);
        if (!stored) {  // (uniform: the row's)
#pragma unroll
          for (int i = 0; i < VEC; ++i) w[i] = projected_diff<T>(w[i], cf[i]);
        }
#pragma unroll
        for (int i = 0; i < VEC; ++i) w[i] = projected_value<T>(cf[i], w[i], A, B);
        if (a.guided != nullptr) store8<T, float, TILE>(a.guided, v, w);  // (p is a value of T: the store's rounding is exact)
      }
      const float w0 = (float)c0[j];
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = fma_(w0, w[i], acc[i]);
    }
    if constexpr (AHEAD < K) {  // operand j + AHEAD is loaded where operand j has been summed, into the registers that frees
      if (j + AHEAD < K) { if (on[j + AHEAD]) raw[j + AHEAD] = load_raw<T, TILE>((j + AHEAD == slot && stored) ? a.diff : a.in[j + AHEAD], v); }
    }
  }
  if constexpr (NOISE) { if (n0) fma_noise8<float>(zeta0, z, acc); }
  store8<T, float, TILE>(a.out, v, acc);
}

}  // namespace skr

// The checks of skr_projected_guided_step_launch_indexed_per_sample in their order.
extern "C" int skr_projected_guided_step_launch_rolling(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                                        const skr_step_projection* proj, const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev,
                                                        const int32_t* sample_index_dev, int32_t row_offset, void* stream) {
  using namespace skr;
  if (!plan || !guide || !proj || !rows_dev || !sample_index_dev) return SKR_ERR_NULL;
  const skr_step_plan& p = *plan;
  const bool step_out = p.out0_dtype != SKR_NONE;
  const bool noise = step_out && p.noise_mode == 1;  // (whether a draw happens is the row's business)
  if (noise && numel > 0 && !seeds_dev) return SKR_ERR_NULL;
  if (p.n_terms < 0 || p.n_terms > SKR_ROW_TERMS || p.n_group_a < 0 || p.n_group_a > p.n_terms) return SKR_ERR_TERMS;
  if (guide->slot < 0 || guide->slot >= p.n_terms) return SKR_ERR_TERMS;
  if (numel < 0) return SKR_ERR_SHAPE;
  if (!step_out && !guide->guided_out) return SKR_ERR_NULL;  // no output at all
  if (p.noise_mode != 0 && p.noise_mode != 1) return SKR_ERR_UNSUPPORTED;
  if (p.out1_dtype != SKR_NONE || p.convert_to != 0 || p.convert_from != 0 || guide->reserved != 0) return SKR_ERR_UNSUPPORTED;  // (chain and zeta1 are row values nobody reads)
  if (proj->reserved != 0 || p.acc_f64 != 0) return SKR_ERR_UNSUPPORTED;
  if (!step_out) return SKR_ERR_UNSUPPORTED;  // the guidance-only form has no rolling form
  if (noise && numel > 0) {
    if (p.sample_numel <= 0 || numel % p.sample_numel != 0) return SKR_ERR_SHAPE;
    if (p.sample_numel % 8 != 0) return SKR_ERR_UNSUPPORTED;
  }
  if (proj->sample_numel < 2 || numel % proj->sample_numel != 0) return SKR_ERR_SHAPE;
  if (noise && numel > 0 && p.sample_numel != proj->sample_numel) return SKR_ERR_SHAPE;
  if (numel == 0) return SKR_OK;
  if (!inputs || !out || !guide->cond || !proj->coef_dev || !proj->diff) return SKR_ERR_NULL;  // (a row may carry momentum: the buffer is required)
  if (const int rc = check_ptrs(inputs, p.n_terms)) return rc;
  if (!aligned16(out) || !aligned16(guide->cond) || !aligned16(guide->guided_out) || !aligned16(proj->diff) || (reinterpret_cast<uintptr_t>(proj->coef_dev) & 3u) != 0)
    return SKR_ERR_ALIGN;
  const int32_t db = p.n_group_a == p.n_terms ? p.dtype_a : p.dtype_b;
  if (!step_inputs_ok(p.dtype_a, db, false) || !step_output_ok(p.out0_dtype, p.dtype_a, false)) return SKR_ERR_DTYPE;  // (an fp64 tensor among them)

  constexpr int64_t CHUNK = (int64_t)BLOCK * VEC;
  const int t = p.dtype_a;
  const bool one_dtype = db == t && p.out0_dtype == t;
  const bool one_trip = g_tune.one_trip && one_dtype && (t != SKR_F32 || g_tune.tile) && p.n_terms >= 1 && numel % CHUNK == 0 && numel / CHUNK <= 0x7fffffffll &&
                        proj->sample_numel % CHUNK == 0 && proj->sample_numel < (1ll << 31);
  if (!one_trip || row_offset < 0) return SKR_ERR_UNSUPPORTED;  // the rolling form has no other kernel
  DeviceGuard device_guard(out);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t chunks = numel / CHUNK;
  with_step_type<false>(t, [&](auto tt) {
    with_bools([&](auto nz) {
      with_count<1, SKR_ROW_TERMS>(p.n_terms, [&](auto n) {
        using T = typename decltype(tt)::type;
        constexpr int N = decltype(n)::value, KMAX = guided_kmax(N);
        ProjectedRollingArgs<KMAX> a;
        for (int k = 0; k < KMAX; ++k) a.in[k] = k < N ? inputs[k] : nullptr;
        a.cond = guide->cond; a.diff = proj->diff; a.out = out; a.guided = guide->guided_out; a.seeds = seeds_dev; a.coef = proj->coef_dev;
        a.xmap_lr = xmap_lr_for(chunks); a.bps_shift = bps_shift_of(proj->sample_numel / CHUNK);
        a.tab = RowRef{rows_dev, sample_index_dev, row_offset}; a.slot = guide->slot;
        hipLaunchKernelGGL((projected_rolling_kernel_v1<T, N, decltype(nz)::value>), dim3((unsigned)chunks), dim3(BLOCK), 0, s, a);
      });
    }, noise);
  });
  return finish_launch();
}
