// The masked solver step on channels-last operands: skr_step_launch_masked_channels_last (include/skrample_hip.h).
//
// skr_step_launch_masked (skr_step_masked.hip) over operands and an output that hold each sample as plane x channels, channel innermost.
// Storage position p of a sample is the logical element l(p) = (p % C) * plane + p / C.  Two things of a masked launch look at the layout:
//   the mask   stays in logical order and is broadcast over leading axes, so position p reads mask[l(p) % mask_numel]; a mask that
//              spells out trailing plane axes only (mask_numel divides plane) reads mask[(p / C) % mask_numel]: one value per PIXEL;
//   the draw   position p takes the normal of element l(p): lane l & 3 of Philox block l >> 2, as in skr_step_launch_channels_last.
// Everything else is elementwise.  Both kernels of this file evaluate skr_step_launch_masked's operations in its order on every element
//   s = sum_k c0[k]*in_k + zeta0*N     k = sum_k c1[k]*in_k over c1[k] != 0     out = fma(m, s, (1 - m) * k), rounded once
// so the output at p has the bits skr_step_launch_masked writes at l(p), and the two agree bit for bit where both apply.
// channels == 1 or plane == 1 is skr_step_launch_masked itself.  There are no row forms here.
#include "skr_step_masked.h"
#include "skr_device.h"
#include "skr_channels_last.h"
#include <atomic>

namespace skr {

std::atomic<int64_t> g_mcl_one_trip_launches{0}, g_mcl_general_launches{0};  // skr_stat("masked_channels_last_one_trip" / "..._general")

// ---- one-trip kernel ---------------------------------------------------------------------------------------------------------------
// step_kernel_cl1 (skr_step_channels_last.hip) with masked_kernel_v1's two coefficient sets: a lane owns one 16-byte vector of 8 storage
// elements, XCD chunk map, every operand load first and the mask load right behind them, the scalars and the Philox rounds while they
// are in flight, the draw exchanged over lane groups (cl_draw8, skr_channels_last.h), store8.
// The mask is indexed by pixel.  A lane's vector is two pixels (C = 4), one pixel (C = 8) or half a pixel (C = 16), so a lane needs two
// mask elements or one: one 32-bit load of two 16-bit elements at C = 4 (mask_numel is even, so pixels 2 vs and 2 vs + 1 never straddle
// a wrap, and the address is 4-byte aligned), one 16-bit load otherwise.  Plain loads, not non-temporal ones: neighbouring lanes share
// the line, and at C = 16 two lanes the very element.  The value is spread over the lane's 8 elements in registers.
template <int KMAX>
struct MaskedClArgs {
  const void* in[KMAX];
  const void* mask;
  void* out;
  int32_t xmap_lr;      // log2(run length) of the XCD chunk map
  int32_t bps_shift;    // chunks per sample: sample_of
  uint32_t mask_numel;  // elements of one sample's mask: even, divides plane
  uint32_t mask_stride; // elements between the masks of two samples: mask_numel or 0
  const uint64_t* seeds;
  uint64_t stream0;
  float zeta0;
  uint32_t quads;       // plane / 4: Philox blocks per channel
  float c0[KMAX];
  float c1[KMAX];
};

template <typename T>
__device__ __forceinline__ float widen16(uint32_t bits) {  // one 16-bit element (in the low half of `bits`, the high half zero) as fp32
  if constexpr (std::is_same<T, bf16_t>::value) return __uint_as_float(bits << 16);
  else return (float)__builtin_bit_cast(_Float16, (uint16_t)bits);
}

template <typename T, int K, int C, bool NOISE>
__global__ __launch_bounds__(BLOCK) void masked_kernel_cl1(const MaskedClArgs<(K <= 4 ? 4 : 8)> a) {
  static_assert(sizeof(T) == 2, "16-bit tensors");
  static_assert(C == 4 || C == 8 || C == 16, "lane groups of 2, 4 or 8");
  const uint32_t c = chunk_of(blockIdx.x, a.xmap_lr);
  const int64_t v = (int64_t)c * BLOCK + threadIdx.x;
  Raw<T> raw[K];
#pragma unroll
  for (int j = 0; j < K; ++j) raw[j] = load_raw<T, false>(a.in[j], v);
  uint32_t smp, within;
  sample_of(c, a.bps_shift, smp, within);
  const uint32_t vs = within * BLOCK + threadIdx.x;  // lane-vector within the sample (sample_numel < 2^31)
  const uint32_t pixel = C == 4 ? 2u * vs : (C == 8 ? vs : vs >> 1);  // the lane's (first) pixel, below plane
  const int64_t at = (int64_t)smp * a.mask_stride + pixel % a.mask_numel;
  uint32_t mbits;
  if constexpr (C == 4) mbits = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint16_t*>(a.mask) + at);  // pixels 2 vs, 2 vs + 1
  else mbits = reinterpret_cast<const uint16_t*>(a.mask)[at];
  __builtin_amdgcn_sched_barrier(0);  // every load is out before the first scalar of the arithmetic is fetched
  float c0[K], c1[K];
#pragma unroll
  for (int j = 0; j < K; ++j) { c0[j] = a.c0[j]; c1[j] = a.c1[j]; }
  [[maybe_unused]] float z[VEC];
  if constexpr (NOISE) cl_draw8<C>(a.seeds[smp], a.stream0, a.quads, vs, threadIdx.x, z);
  float s[VEC], kn[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) { s[i] = 0.f; kn[i] = 0.f; }
#pragma unroll
  for (int j = 0; j < K; ++j) {
    float w[VEC];
    widen<T, float>(raw[j], w);
    const float w0 = c0[j], w1 = c1[j];
#pragma unroll
    for (int i = 0; i < VEC; ++i) s[i] = fma_(w0, w[i], s[i]);
    if (w1 != 0.f) {  // (uniform: a kernarg scalar) an operand absent from the known form adds nothing to it, not even 0 * x
#pragma unroll
      for (int i = 0; i < VEC; ++i) kn[i] = fma_(w1, w[i], kn[i]);
    }
  }
  if constexpr (NOISE) fma_noise8<float>(a.zeta0, z, s);  // (the host chose the instantiation by the plan's zeta0, as for masked_kernel_v1)
  const float m_lo = widen16<T>(C == 4 ? (mbits & 0xFFFFu) : mbits), m_hi = C == 4 ? widen16<T>(mbits >> 16) : m_lo;
  float o[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    const float m = i < 4 ? m_lo : m_hi;
    o[i] = fma_(m, s[i], mul_(sub_(1.f, m), kn[i]));
  }
  store8<T, float, false>(a.out, v, o);
}

// ---- general grid-stride kernel ----------------------------------------------------------------------------------------------------
// Everything else skr_step_launch_masked takes: masked_kernel_gen's arithmetic (skr_step_masked.hip) with step_kernel_cl's element
// numbering (skr_step_channels_last.hip).  One element per lane and trip, l(p) worked out element by element, dtypes at run time.
struct MaskedClGenArgs {
  const void* in[SKR_ROW_TERMS];
  double c0[SKR_ROW_TERMS];
  double c1[SKR_ROW_TERMS];
  const void* mask;
  void* out;
  const uint64_t* seeds;
  double zeta0;
  uint64_t stream0;
  int64_t numel, sample_numel, mask_numel, mask_stride, channels, plane;
  int32_t n, n_a, dt_a, dt_b, dt_out, dt_mask, noise;
};

template <typename Acc>
__global__ __launch_bounds__(BLOCK) void masked_kernel_cl(const MaskedClGenArgs a) {
  constexpr bool F64 = std::is_same<Acc, double>::value;  // (an fp64 tensor takes part in fp64 arithmetic only)
  for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < a.numel; e += (int64_t)gridDim.x * BLOCK) {
    const int64_t smp = e / a.sample_numel, p = e - smp * a.sample_numel;
    const int64_t x = p / a.channels, ch = p - x * a.channels;
    const int64_t l = ch * a.plane + x;  // the logical element of storage position p
    const Acc m = load_elem<Acc, F64>(a.mask, smp * a.mask_stride + l % a.mask_numel, a.dt_mask);
    Acc s = 0, kn = 0;
    for (int j = 0; j < a.n; ++j) {
      const Acc w = load_elem<Acc, F64>(a.in[j], e, j < a.n_a ? a.dt_a : a.dt_b);
      const Acc w0 = (Acc)a.c0[j], w1 = (Acc)a.c1[j];
      s = fma_(w0, w, s);
      if (w1 != (Acc)0) kn = fma_(w1, w, kn);
    }
    if (a.noise) {  // element l of the sample: Philox block l >> 2, lane l & 3
      float z[4];
      normal4(a.seeds[smp], a.stream0, (uint64_t)l >> 2, z);
      const int lane = (int)(l & 3);
      const float zz = lane == 0 ? z[0] : (lane == 1 ? z[1] : (lane == 2 ? z[2] : z[3]));
      s = fma_((Acc)a.zeta0, (Acc)zz, s);
    }
    store_any<Acc>(a.out, e, a.dt_out, fma_(m, s, mul_(sub_((Acc)1, m), kn)));
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
// what the one-trip kernel takes (the header's list): the shared geometry with sample_numel < 2^31, and a mask of the tensors' dtype
// with an even element count that divides the plane
static bool mcl_one_trip_ok(const skr_step_plan& p, const skr_step_mask& mk, const skr_step_layout& l, int64_t numel, int* bps_shift) {
  if (mk.dtype != p.dtype_a || l.plane % mk.mask_numel != 0 || mk.mask_numel % 2 != 0) return false;
  return cl_one_trip_geometry(p, l, numel, (1ll << 31) - 1, bps_shift);
}

template <typename T>
static int launch_mcl1(const skr_step_plan& p, const skr_step_mask& mk, const skr_step_layout& l, const void* const* inputs, void* out,
                       const uint64_t* seeds, int64_t numel, bool noise, int bps_shift, hipStream_t stream) {
  const int64_t chunks = numel / ((int64_t)BLOCK * VEC);
  with_bools([&](auto nz) {
    with_count<1, 8>(p.n_terms, [&](auto n) {
      constexpr int N = decltype(n)::value, KMAX = N <= 4 ? 4 : 8;
      constexpr bool NOISE = decltype(nz)::value;
      MaskedClArgs<KMAX> a;
      for (int k = 0; k < KMAX; ++k) {
        a.in[k] = k < N ? inputs[k] : nullptr;
        a.c0[k] = k < N ? (float)p.coef0[k] : 0.f;
        a.c1[k] = k < N ? (float)p.coef1[k] : 0.f;
      }
      a.mask = mk.mask; a.out = out; a.seeds = seeds;
      a.xmap_lr = xmap_lr_for(chunks); a.bps_shift = bps_shift;
      a.mask_numel = (uint32_t)mk.mask_numel; a.mask_stride = (uint32_t)mk.batch_stride;
      a.stream0 = p.stream0; a.zeta0 = (float)p.zeta0; a.quads = (uint32_t)(l.plane / 4);
      const dim3 grid((unsigned)chunks), block(BLOCK);
      with_channels(l.channels, [&](auto c) { hipLaunchKernelGGL((masked_kernel_cl1<T, N, decltype(c)::value, NOISE>), grid, block, 0, stream, a); });
    });
  }, noise);
  return finish_launch();
}

static int launch_mcl_general(const skr_step_plan& p, const skr_step_mask& mk, const skr_step_layout& l, const void* const* inputs, void* out,
                              const uint64_t* seeds, int64_t numel, bool noise, hipStream_t stream) {
  MaskedClGenArgs a;
  for (int k = 0; k < SKR_ROW_TERMS; ++k) {
    const bool live = k < p.n_terms;
    a.in[k] = live ? inputs[k] : nullptr;
    a.c0[k] = live ? p.coef0[k] : 0.0;
    a.c1[k] = live ? p.coef1[k] : 0.0;
  }
  a.mask = mk.mask; a.out = out; a.seeds = seeds; a.zeta0 = p.zeta0; a.stream0 = p.stream0;
  a.numel = numel; a.sample_numel = p.sample_numel; a.mask_numel = mk.mask_numel; a.mask_stride = mk.batch_stride;
  a.channels = l.channels; a.plane = l.plane;
  a.n = p.n_terms; a.n_a = p.n_group_a; a.dt_a = p.dtype_a; a.dt_b = p.dtype_b; a.dt_out = p.out0_dtype; a.dt_mask = mk.dtype;
  a.noise = noise ? 1 : 0;
  const dim3 grid((unsigned)grid_blocks(numel, BLOCK, 256 * 64)), block(BLOCK);
  if (p.acc_f64) hipLaunchKernelGGL((masked_kernel_cl<double>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((masked_kernel_cl<float>), grid, block, 0, stream, a);
  return finish_launch();
}

}  // namespace skr

extern "C" int skr_step_launch_masked_channels_last(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_mask* mask,
                                                    const uint64_t* seeds_dev, const skr_step_layout* layout, int64_t numel, void* stream) {
  if (!plan || !mask) return SKR_ERR_NULL;
  const skr_step_plan& p = *plan;
  const skr_step_mask& mk = *mask;
  skr::MaskedLaunch ml;
  if (const int rc = skr::masked_prepare(p, mk, inputs, out, seeds_dev, numel, false, &ml)) return rc;
  if (const int rc = skr::layout_check(p, layout)) return rc;
  const skr_step_layout& l = *layout;
  if (numel == 0) return SKR_OK;
  if (l.channels == 1 || l.plane == 1) return skr_step_launch_masked(plan, inputs, out, mask, seeds_dev, numel, stream);  // l(p) = p
  skr::DeviceGuard device_guard(out);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int bps_shift = 0;
  if (skr::mcl_one_trip_ok(p, mk, l, numel, &bps_shift)) {
    ++skr::g_mcl_one_trip_launches;
    return p.dtype_a == SKR_BF16 ? skr::launch_mcl1<skr::bf16_t>(p, mk, l, inputs, out, seeds_dev, numel, ml.noise, bps_shift, s)
                                 : skr::launch_mcl1<skr::f16_t>(p, mk, l, inputs, out, seeds_dev, numel, ml.noise, bps_shift, s);
  }
  ++skr::g_mcl_general_launches;
  return skr::launch_mcl_general(p, mk, l, inputs, out, seeds_dev, numel, ml.noise, s);
}
