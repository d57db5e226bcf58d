/*
 * skrample_hip.h -- C ABI of the MI355X (gfx950) sampler-step engine.
 *
 * This is the drop-in boundary for the per-step hot path of Beinsezii/skrample.  The reference is
 * pure Python and has no FFI of its own; each entry point below names the reference interface whose
 * tensor arithmetic it replaces (file:line under the reference tree).  The Python side
 * (skrample_amd/_hip.py) binds these with ctypes; INTEGRATION.md shows the binding a reference
 * maintainer would add.
 *
 * Conventions: plain pointers and sizes only; every buffer is caller-owned device memory; launches
 * are asynchronous on the caller's hipStream_t (passed as void*); every function returns an int
 * status (0 = SKR_OK) and never throws; no hidden global state except the loaded code object.
 * Thread-safe for concurrent callers on distinct streams.
 */
#ifndef SKRAMPLE_HIP_H
#define SKRAMPLE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKR_ABI_VERSION 15
#define SKR_MAX_TERMS 80 /* 2 x 35-stage tableau pairs + base + noise, see skr_step_plan */

/* Devices and streams: every entry point launches on the device that owns its output buffer (queried from the pointer when
 * the process sees more than one GPU; single-GPU processes skip the query) and restores the caller's current device before
 * returning.  `stream` is a hipStream_t of that device (NULL = its default stream).  Calls are asynchronous; distinct
 * streams may be driven from distinct threads. */

enum skr_status {
  SKR_OK = 0,
  SKR_ERR_NULL = 1,        /* required pointer is NULL */
  SKR_ERR_DTYPE = 2,       /* dtype combination has no kernel */
  SKR_ERR_TERMS = 3,       /* n_terms out of range or terms not grouped by dtype */
  SKR_ERR_ALIGN = 4,       /* a buffer is not 16-byte aligned */
  SKR_ERR_SHAPE = 5,       /* numel / sample_numel / shape arguments inconsistent */
  SKR_ERR_LAUNCH = 6,      /* hipLaunchKernel failed (see skr_last_hip_error) */
  SKR_ERR_UNSUPPORTED = 7, /* valid request outside what the kernels cover */
  SKR_ERR_LIBRARY = 8,     /* an external library failed its self-check: a new hipFFT plan transformed unit impulses wrongly (skr_noise_colored_any / skr_colorize) */
  SKR_ERR_CAPTURE = 9,     /* the stream is capturing and this shape's first use must build per-length tables or plans: run it once eagerly first */
};

enum skr_dtype { SKR_BF16 = 0, SKR_F16 = 1, SKR_F32 = 2, SKR_F64 = 3, SKR_NONE = -1 };

/*
 * One fused solver step:
 *
 *     out0[e] = sum_k coef0[k] * in_k[e]  + zeta0 * N(seed[s(e)], stream0, e)
 *     out1[e] = chain * out0[e] + sum_k coef1[k] * in_k[e] + zeta1 * N(seed[s(e)], stream1, e)
 *
 * evaluated in fp32 (fp64 if acc_f64) registers and rounded once per output, in a single pass over
 * HBM.  `chain` uses out0 before its rounding to out0_dtype.  N() is the Philox4x32-10 / Box-Muller
 * normal of oracle/skr_oracle/noise.py::philox_normal, keyed by the per-sample seed (s(e) =
 * e / sample_numel), so results do not depend on how a batch is sharded over GPUs.
 *
 * Replaces, per sampler (coefficients are computed on the host in fp64 by skrample_amd.sampling):
 *   - DiffusionModel.to_x / from_x / ModelConvert.output_to   skrample/sampling/models.py:92-224
 *   - DiffusionModel.forward (sample*G + output*D + noise*z)   skrample/sampling/models.py:53-67
 *   - Euler / DPM / Adams / UniP._sample_packed tensor math    skrample/sampling/structured.py:167-436
 *   - UniPC.sample_packed (corrector out0 + predictor out1)    skrample/sampling/structured.py:469-497
 *   - RKWrapperCore.step_tableau_inside_out (one stage)        skrample/diffusers.py:746-796
 *   - the dtype casts around them                              skrample/diffusers.py:575-599
 *
 * Inputs must be grouped by dtype: terms [0, n_group_a) have dtype_a, the rest dtype_b.
 */
typedef struct skr_step_plan {
  int32_t n_terms;     /* 0..SKR_MAX_TERMS */
  int32_t n_group_a;   /* terms [0,n_group_a) are dtype_a, [n_group_a,n_terms) dtype_b */
  int32_t dtype_a;     /* skr_dtype */
  int32_t dtype_b;     /* skr_dtype; ignored when n_group_a == n_terms */
  int32_t out0_dtype;  /* skr_dtype, SKR_NONE if out0 is not stored */
  int32_t out1_dtype;  /* skr_dtype, SKR_NONE if there is no second output */
  int32_t acc_f64;     /* 1 = accumulate in double (compute_scale=float64), else float */
  int32_t noise_mode;  /* 0 = none, 1 = in-kernel Philox normals */
  double coef0[SKR_MAX_TERMS];
  double coef1[SKR_MAX_TERMS];
  double chain;
  double zeta0, zeta1;
  uint64_t stream0, stream1; /* Philox stream id of the draw feeding out0 / out1 */
  int64_t sample_numel;      /* elements per batch item (prod(shape[1:])) */
  /* Optional rounded pair conversion (Runge-Kutta wrapper, skrample/diffusers.py:819-834): when
   * convert_to or convert_from is non-zero, out0 is NOT the coef0 combination but
   *     out0 = from_x(s, to_x(s, o)),  s = inputs[0], o = inputs[1]  (both of dtype_a)
   * evaluated one rounded op at a time in dtype_a's arithmetic, exactly as the reference's tensor ops:
   *   to_x   1: (s - k0*o)/k1   2: k1*s - k0*o   3: o*k0        (0: o)
   *   from_x 1: (s - k2*x)/k3   2: (k2*s - x)/k3 3: x/k2        (0: x)
   * out1 = chain*out0 + sum_k coef1[k]*in_k (+ noise) as usual.  Requires out1. */
  int32_t convert_to, convert_from;
  double convert_k[4];
} skr_step_plan;

int skr_step_launch(const skr_step_plan* plan, const void* const* inputs, void* out0, void* out1,
                    const uint64_t* seeds_dev /* [batch] device, may be NULL if noise_mode==0 */,
                    int64_t numel, void* stream);

/*
 * The transposed step (autograd of skr_step_launch).  A step is linear in its tensor operands and its coefficients are host
 * numbers, so the gradient of every operand is a fixed combination of the incoming gradients of out0 / out1 -- no saved tensors:
 *
 *     grad_k[e] = a[k] * g0[e] + b[k] * g1[e]        (forward: a[k] = coef0[k], b[k] = chain * coef0[k] + coef1[k])
 *
 * evaluated in fp32 (fp64 if acc_f64) registers and rounded to the gradient's dtype as the step's outputs are (store8): once from
 * fp32; from fp64 to a 16-bit gradient through fp32, i.e. twice.  One pass over HBM: g0 (and g1) read once, one gradient written per
 * operand.  Launches of whole 2048-element chunks with one 16/32-bit dtype throughout, fp32 arithmetic and <= 16 gradients take the
 * one-trip kernel; anything else (mixed dtypes, ragged sizes, fp64, more gradients) a grid-stride kernel of per-element accesses.  g1 may be NULL (g1_dtype = SKR_NONE); g0 is required (a caller with only an out1
 * gradient passes it as g0 with b as a).  Gradients are grouped by dtype as the operands of skr_step_plan: [0, n_group_a) have
 * dtype_a, the rest dtype_b.  The noise terms have no gradient; the derivative of a rounded pair conversion (convert_*) is affine
 * in (s, o) and folded into a[0..1] by the caller, so there is no conversion mode here.  Every buffer 16-byte aligned.
 */
typedef struct skr_step_grad_plan {
  int32_t n_grads;   /* 1..SKR_MAX_TERMS */
  int32_t n_group_a; /* grads [0,n_group_a) are dtype_a, [n_group_a,n_grads) dtype_b */
  int32_t dtype_a;   /* skr_dtype */
  int32_t dtype_b;   /* skr_dtype; ignored when n_group_a == n_grads */
  int32_t g0_dtype;  /* skr_dtype of the incoming gradient of out0 */
  int32_t g1_dtype;  /* skr_dtype of the second incoming gradient, SKR_NONE if absent */
  int32_t acc_f64;   /* 1 = evaluate in double */
  int32_t reserved;  /* 0 */
  double a[SKR_MAX_TERMS];
  double b[SKR_MAX_TERMS];
} skr_step_grad_plan;

int skr_step_backward_launch(const skr_step_grad_plan* plan, const void* g0, const void* g1, void* const* grads, int64_t numel,
                             void* stream);

/*
 * Device-resident step scalars -- SURVEY.md 8(f) rank 1; replaces the per-step host work of
 * SkrampleWrapperScheduler.step (skrample/diffusers.py:565-567: timestep -> index lookup with an .item() sync) and of the
 * schedule evaluation inside every sampler step (skrample/scheduling.py:51-62, skrample/sampling/interface.py:34-59).
 *
 * A launch recorded into a HIP graph freezes its kernel arguments, so a graph built on skr_step_launch serves exactly one
 * schedule.  skr_step_launch_indexed takes the step's scalars from device memory instead: the kernel reads
 *     row = rows_dev[(index_dev ? index_dev[0] : 0) + row_offset]
 * when it runs.  `plan` fixes the structure only (operand count and dtypes, outputs, noise_mode, whether a rounded conversion
 * exists); its coef0 / coef1 / chain / zeta / stream / convert_k values are ignored, and convert_to / convert_from must be
 * the row's kinds.  One captured loop therefore serves any schedule of its length (rewrite the rows: new sigmas, shift,
 * begin index, stochasticity) and several resident schedules (move index_dev), with no re-capture and no host sync.
 * Rows with zeta = 0 skip the draw exactly as a launch without noise does.  Covered: launches the one-trip kernels take
 * (whole 2048-element chunks, <= 16 operands -- the size of a row --, fp32 accumulation) and, for single-output plans, ragged samples
 * (below, behind skr_step_launch_rolling); anything else returns SKR_ERR_UNSUPPORTED.
 */
#define SKR_ROW_TERMS 16
typedef struct skr_step_row {
  double coef0[SKR_ROW_TERMS];
  double coef1[SKR_ROW_TERMS];
  double chain;
  double zeta0, zeta1;
  uint64_t stream0, stream1;
  double convert_k[4];
} skr_step_row;

int skr_step_launch_indexed(const skr_step_plan* plan, const void* const* inputs, void* out0, void* out1,
                            const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev,
                            const int32_t* index_dev /* device int32, may be NULL */, int32_t row_offset, void* stream);

/*
 * Per-sample rows: the same launch with one index PER SAMPLE.  The batch is numel / plan->sample_numel samples, sample_index_dev
 * holds that many device int32, and the workgroups of sample s read
 *     row = rows_dev[sample_index_dev[s] + row_offset]
 * so every sample of one launch follows its own resident schedule (another shift, sigma family, stochasticity or begin index per
 * request of a batch).  A sample whose row has zeta = 0 skips its draw while its batch neighbours draw; Philox stays keyed by the
 * sample's seed and the element's position within the sample, so a sample's result is bit-identical to what
 * skr_step_launch_indexed gives it with that row for the whole batch.
 * Covered: what skr_step_launch_indexed covers, and a workgroup must lie inside one sample: plan->sample_numel must be a positive
 * multiple of 2048 that divides numel, with or without noise (SKR_ERR_SHAPE / SKR_ERR_UNSUPPORTED otherwise) -- or, for a
 * single-output plan, a ragged sample size (below, behind skr_step_launch_rolling), whose workgroups are the sample's own as well.
 * A NULL sample_index_dev is SKR_ERR_NULL.
 * Index validity is the caller's business, as with index_dev: every sample_index_dev[s] + row_offset must name a row of the
 * table.  The kernel neither checks nor clamps an index -- an entry outside the table reads whatever lies there (or faults) --
 * so validate on the host before uploading (skrample_amd.graphs.CapturedLoop does).
 */
int skr_step_launch_indexed_per_sample(const skr_step_plan* plan, const void* const* inputs, void* out0, void* out1,
                                       const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev,
                                       const int32_t* sample_index_dev /* device int32[numel / sample_numel] */, int32_t row_offset,
                                       void* stream);

/*
 * Rolling batches (continuous batching): skr_step_launch_indexed_per_sample with samples that may sit at different positions of
 * their loops, or be absent.  Contract, coverage and error codes are those of skr_step_launch_indexed_per_sample; on top of them
 *   inactive sample  sample_index_dev[s] < 0 (tested before row_offset is added): the workgroups of sample s return before their
 *                    first vector-memory instruction.  Nothing of that sample is read; out0 / out1 keep their bytes there.
 *   absent operand   an operand k whose coef0[k] and coef1[k] are both exactly zero (+0 or -0) in the sample's row is not loaded and
 *                    adds nothing to either output: its bytes may be anything, NaN and inf included (the slot's previous occupant).
 *                    The pair of a rounded conversion (operands 0 and 1 when plan->convert_to / convert_from is set) is always
 *                    loaded.  A row whose zeta is zero skips the draw.
 *   operand order    the operands that are present are accumulated in slot order, so a sample's result has the bits of the narrower
 *                    launch (skr_step_launch) that holds exactly those operands in that order.
 * `plan` is therefore the WIDEST step of the sampler (its steady state); a sample still in its multistep ramp-up has a row with
 * zeros in the slots of the history it does not have yet.  Index validity stays the caller's business: every non-negative
 * sample_index_dev[s] + row_offset must name a row of the table; the kernel neither checks nor clamps
 * (skrample_amd.rolling.RollingBatch validates on the host).
 */
int skr_step_launch_rolling(const skr_step_plan* plan, const void* const* inputs, void* out0, void* out1,
                            const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev,
                            const int32_t* sample_index_dev /* device int32[numel / sample_numel], < 0: inactive */, int32_t row_offset,
                            void* stream);

/*
 * Ragged samples: samples that are NOT whole 2048-element chunks (most non-square SDXL latent buckets: (4,144,112) is 31.5 chunks).
 * No new entry: skr_step_launch_indexed, skr_step_launch_indexed_per_sample and skr_step_launch_rolling take them for SINGLE-OUTPUT
 * plans -- out1_dtype == SKR_NONE, no convert_to / convert_from, one 16- or 32-bit dtype for the operands and out0, fp32 accumulation
 * (acc_f64 == 0), 1 .. SKR_ROW_TERMS operands.  A launch is ragged when
 *     plan->sample_numel >= 2048,  % 8 == 0,  % 2048 != 0,  < 2^31,   numel == batch * plan->sample_numel,
 * and batch * ceil(sample_numel / 2048) workgroups fit the grid of the whole-chunk kernels (INT32_MAX).  Every sample then gets
 * ceil(sample_numel / 2048) workgroups of its own, the last of them partly empty: lanes and 4-element groups behind the sample's
 * end issue no load and no store (csrc/skr_step_ragged.hip).
 *   skr_step_launch_indexed_per_sample, skr_step_launch_rolling   every such launch takes the ragged form.
 *   skr_step_launch_indexed   when the plan draws (noise_mode == 1) or numel is not whole chunks; plan->sample_numel must then be given
 *                             and divide numel, with or without noise.  A launch the whole-chunk kernels take keeps them; a numel that is
 *                             not whole chunks with no usable sample_numel stays SKR_ERR_UNSUPPORTED.
 * Contract: every sample of a ragged launch has, bit for bit, what skr_step_launch writes for that sample alone with its row's values in
 * the plan -- for the rolling form the plan that holds exactly the sample's present operands, in slot order.  No byte outside
 * [out0, out0 + numel * sizeof(T)) is written, and an inactive slot's bytes are not written either (its neighbour's partly empty last
 * chunk ends at the neighbour's last element).  The checks keep their order and their codes: the ragged test stands where the
 * whole-chunk test stands, and everything else answers as before -- samples below 2048 elements or not a multiple of 8, two-output
 * plans, rounded conversions, acc_f64 and two dtype groups on samples that are not whole chunks are SKR_ERR_UNSUPPORTED.  The masked,
 * guided, rescaled, statistics, backward, channels-last and noise entries have no ragged form.
 */

/*
 * Device-resident positions of a rolling batch: computes, on the device, the sample_index_dev a skr_step_launch_rolling reads and the
 * timestep vector the network reads, from per-slot state the host wrote (and validated) once when the request was admitted, and
 * moves every running slot on by one step.  One thread per slot, no allocation, no synchronisation, launched on `stream`
 * (capturable): a tick needs no host-to-device copy.  For every slot b, with p = position_dev[b] and n = length_dev[b]:
 *   active    0 <= p < n <= max_steps:  sample_index_dev[b] = b * max_steps + p,  timesteps_dev[b] = times_dev[b * max_steps + p]
 *             (moved as bits),  position_dev[b] = p + 1;
 *   inactive  anything else (n = 0 is a free slot, p = n a finished one):  sample_index_dev[b] = -1;  timesteps_dev[b] and
 *             position_dev[b] keep their bytes -- the timestep stays the last one the slot had, and an idle slot can tick for ever
 *             without its position overflowing.
 * An index that reaches the step kernel therefore names a row inside the slot's own run of the table (max_steps rows per slot), by
 * construction: this kernel is the validation the step kernels do not make.
 * Checked before the launch, without dereferencing a pointer: any NULL pointer is SKR_ERR_NULL; capacity < 1, max_steps < 1 or
 * capacity * max_steps > INT32_MAX is SKR_ERR_SHAPE.
 */
int skr_rolling_advance(int32_t* position_dev /* [capacity] in / out */, const int32_t* length_dev /* [capacity] run length, 0 = free */,
                        const float* times_dev /* [capacity * max_steps] timestep of every row */,
                        int32_t* sample_index_dev /* [capacity] out */, float* timesteps_dev /* [capacity] out */, int32_t capacity,
                        int32_t max_steps, void* stream);

/*
 * The masked step -- the keep-region blend of in-painting / masked image-to-image loops, fused into the step launch.  Such a loop
 * runs, after every scheduler step,  known = add_noise(original, noise, next timestep);  latent = mask * prev + (1 - mask) * known
 * (a step launch, an add_noise launch and three or four elementwise kernels).  Both the step and the re-noised known region are
 * linear forms over tensor operands with host coefficients, so one launch evaluates
 *
 *     out[e] = m[e] * (sum_k coef0[k] * in_k[e] + zeta0 * N(seed[s(e)], stream0, e))  +  (1 - m[e]) * (sum_k coef1[k] * in_k[e])
 *
 * in one pass, with one store and one rounding.  Plan contract: out1_dtype must be SKR_NONE (`out` has out0_dtype); coef1 is the
 * known-region form; chain, zeta1 and convert_* must be zero (SKR_ERR_UNSUPPORTED otherwise); sample_numel is required, with or
 * without noise; in-kernel Philox noise (noise_mode == 1, zeta0, stream0) has the keying and block numbering of skr_step_launch; the
 * dtype groups are those of skr_step_launch; at most SKR_ROW_TERMS operands (SKR_ERR_TERMS beyond).
 * Arithmetic, in the accumulate type (fp32, fp64 if acc_f64):
 *     s   the step form exactly as skr_step_launch accumulates it: operands in slot order from 0, one fma each, the noise term last
 *         (skipped when zeta0 == 0);
 *     k   the known form, accumulated the same way over the operands whose coef1 is not exactly zero, in slot order;
 *     out = fma(m, s, (1 - m) * k), rounded once to out0_dtype as the step kernels round.
 * So where m == 1 (and k is finite) `out` has the bits skr_step_launch gives for coef0 / zeta0 / stream0 alone, and where m == 0 (and s
 * is finite) the bits it gives for coef1 as its coef0 over exactly the operands present in it, without noise.
 * Launches of whole 2048-element chunks whose samples are whole chunks, with one 16- or 32-bit dtype for operands, mask and output,
 * fp32 arithmetic and mask_numel % 8 == 0 take a one-trip vector kernel; everything else (ragged sizes, small samples, other
 * mask_numel, mixed dtypes, fp64) a grid-stride per-element kernel.  The two agree bit for bit ("one_trip" 0 forces the second).
 * Checked before the launch, without dereferencing device memory: NULL pointers SKR_ERR_NULL; mask_numel < 1, mask_numel not dividing
 * sample_numel, sample_numel not dividing numel, or a batch_stride other than 0 or mask_numel SKR_ERR_SHAPE; a misaligned pointer
 * SKR_ERR_ALIGN.
 */
typedef struct skr_step_mask {
  const void* mask;       /* device, 16-byte aligned */
  int32_t dtype;          /* skr_dtype of the mask: bf16 / f16 / f32 (f64 only with acc_f64) */
  int32_t reserved;       /* 0 */
  int64_t mask_numel;     /* elements of ONE sample's mask; must divide plan->sample_numel.
                             Element i of a sample (i = e % sample_numel) reads mask[i % mask_numel]:
                             (C,H,W) latents with a (1,H,W) mask -> H*W; a full mask -> sample_numel */
  int64_t batch_stride;   /* mask_numel: one mask per sample;  0: one mask for the whole batch */
} skr_step_mask;

int skr_step_launch_masked(const skr_step_plan* plan, const void* const* inputs, void* out,
                           const skr_step_mask* mask, const uint64_t* seeds_dev, int64_t numel, void* stream);

/*
 * The transposed masked step (autograd of skr_step_launch_masked).  The masked step is linear in its operands, its coefficients are
 * host numbers and its mask is data, so the gradient of operand k needs no saved operand:
 *
 *     grad_k[e] = (a[k] * m[e] + b[k] * (1 - m[e])) * g[e]        (forward: a[k] = coef0[k], b[k] = coef1[k])
 *
 * `plan` is skr_step_grad_plan unchanged: a / b as above, g0_dtype the dtype of `g`, g1_dtype SKR_NONE (SKR_ERR_UNSUPPORTED otherwise),
 * gradients grouped by dtype as in skr_step_backward_launch, 1..SKR_ROW_TERMS of them (SKR_ERR_TERMS beyond: the forward takes no
 * more operands).  `mask` is skr_step_mask unchanged, with the forward's meaning of mask_numel and batch_stride; `sample_numel` is the
 * forward plan's.  The noise term has no gradient, and neither has the mask.
 * Arithmetic, in the accumulate type (fp32, fp64 if acc_f64):
 *     t = 1 - m;   w = fma(a, m, b * t);   grad = w * g
 * rounded once to the gradient's dtype as skr_step_backward_launch rounds.  So where m == 1 a gradient is a * g with the bits
 * skr_step_backward_launch gives for that a, and where m == 0 it is b * g.  One pass over HBM: g and the mask read once, one
 * gradient written per operand.
 * Launches of whole 2048-element chunks whose samples are whole chunks, with one 16- or 32-bit dtype for g, mask and every gradient,
 * fp32 arithmetic and mask_numel % 8 == 0 take a one-trip vector kernel (kernarg slots of 4 / 8 / 16 gradients); everything else
 * (ragged sizes, samples below a chunk, other mask_numel, two dtype groups, fp64) a grid-stride per-element kernel.  The two agree
 * bit for bit ("one_trip" 0 forces the second).
 * Checked before the launch, without dereferencing device memory: a NULL plan, mask, g, mask->mask, grads or gradient SKR_ERR_NULL;
 * a dtype code that names no tensor dtype SKR_ERR_DTYPE; n_grads outside 1..SKR_ROW_TERMS SKR_ERR_TERMS; a misaligned pointer
 * SKR_ERR_ALIGN; mask_numel < 1, mask_numel not dividing sample_numel, sample_numel not dividing numel, or a batch_stride other than 0
 * or mask_numel SKR_ERR_SHAPE; an fp64 mask without acc_f64 SKR_ERR_UNSUPPORTED.  numel == 0 is SKR_OK with nothing launched.
 */
int skr_step_masked_backward_launch(const skr_step_grad_plan* plan, const void* g, const skr_step_mask* mask, void* const* grads,
                                    int64_t numel, int64_t sample_numel, void* stream);

/*
 * The masked step with device-resident scalars: skr_step_launch_masked as skr_step_launch_indexed and
 * skr_step_launch_indexed_per_sample make skr_step_launch, so that one captured in-painting loop serves any schedule of its length
 * (other sigmas, shift, begin index / strength, stochasticity), keeps several schedules resident and lets every sample follow its own.
 * `plan` fixes the structure only: operand count and dtype groups, out0_dtype (out1_dtype must be SKR_NONE), noise_mode, sample_numel,
 * acc_f64 == 0, convert_* == 0.  Its coef0 / coef1 / zeta0 / stream0 values are ignored; when the kernel runs it reads them from
 *     indexed      rows_dev[(index_dev ? index_dev[0] : 0) + row_offset]
 *     per sample   rows_dev[sample_index_dev[s] + row_offset]            for the workgroups of sample s
 * skr_step_row is used unchanged; the row's chain, zeta1, stream1 and convert_k are not read.  The mask descriptor is skr_step_mask
 * unchanged: the mask's pointer, layout and dtype are launch arguments (frozen into a captured graph), its contents are data.
 * Arithmetic: that of skr_step_launch_masked, and bit for bit what skr_step_launch_masked gives with the row's values in its plan: s is
 * accumulated in slot order, one fma per operand, the noise last -- a row whose zeta0 is exactly zero skips the draw, as in the other
 * row forms --; k over the operands whose row coef1 is not exactly zero; out = fma(m, s, (1 - m) * k), rounded once.  The row's
 * doubles are narrowed to fp32 on the device with the conversion the host applies to a plan's doubles.  A sample of a per-sample
 * launch has the bits the indexed launch gives it with that row for the whole batch.
 * Covered: exactly what the one-trip kernel of skr_step_launch_masked takes -- whole 2048-element chunks, samples made of whole chunks,
 * one 16- or 32-bit dtype for operands, mask and output, fp32 arithmetic, 1..SKR_ROW_TERMS operands, mask_numel % 8 == 0.  Anything
 * else is SKR_ERR_UNSUPPORTED ("one_trip" 0 and fp32 tensors with "tile" 0 included): there is no grid-stride row form.
 * Checked before the launch, without dereferencing device memory, in the order and with the codes of skr_step_launch_masked; on top of
 * them a NULL rows_dev is SKR_ERR_NULL, a NULL sample_index_dev in the per-sample entry is SKR_ERR_NULL, and a launch with
 * noise_mode == 1 needs seeds_dev whatever its rows hold.  out1_dtype != SKR_NONE, acc_f64 or a non-zero convert_* is
 * SKR_ERR_UNSUPPORTED, as is a negative row_offset.
 * Index validity is the caller's business, as with skr_step_launch_indexed: index_dev[0] + row_offset, and every
 * sample_index_dev[s] + row_offset, must name a row of the table.  The kernel neither checks nor clamps an index -- an entry outside
 * the table reads whatever lies there (or faults) -- so validate on the host before uploading (skrample_amd.graphs.CapturedLoop does).
 * Neither entry takes a negative index or skips an operand: the rolling form is skr_step_launch_masked_rolling, below.
 */
int skr_step_launch_masked_indexed(const skr_step_plan* plan, const void* const* inputs, void* out,
                                   const skr_step_mask* mask, const uint64_t* seeds_dev, int64_t numel,
                                   const skr_step_row* rows_dev, const int32_t* index_dev /* device int32, may be NULL */,
                                   int32_t row_offset, void* stream);

int skr_step_launch_masked_indexed_per_sample(const skr_step_plan* plan, const void* const* inputs, void* out,
                                              const skr_step_mask* mask, const uint64_t* seeds_dev, int64_t numel,
                                              const skr_step_row* rows_dev,
                                              const int32_t* sample_index_dev /* device int32[numel / sample_numel] */,
                                              int32_t row_offset, void* stream);

/*
 * The masked step of a rolling batch: skr_step_launch_masked_indexed_per_sample with samples that may sit at different positions of
 * their in-painting loops, be plain (unmasked) requests, or be absent -- what skr_step_launch_rolling is to
 * skr_step_launch_indexed_per_sample.  Structure, coverage, checks and error codes are those of
 * skr_step_launch_masked_indexed_per_sample: `plan` fixes the structure only, skr_step_row and skr_step_mask are used unchanged, whole
 * 2048-element chunks, samples made of whole chunks, one 16- or 32-bit dtype for operands, mask and output, fp32 arithmetic,
 * 1..SKR_ROW_TERMS operands, mask_numel % 8 == 0, batch_stride mask_numel or 0; anything else is SKR_ERR_UNSUPPORTED ("one_trip" 0 and
 * fp32 tensors with "tile" 0 included).  A NULL rows_dev or sample_index_dev is SKR_ERR_NULL, a negative row_offset
 * SKR_ERR_UNSUPPORTED, and a launch with noise_mode == 1 needs seeds_dev whatever its rows hold.  On top of that contract
 *   inactive sample  sample_index_dev[s] < 0 (tested before row_offset is added): the workgroups of sample s return before their
 *                    first vector-memory instruction.  No operand, mask, seed or row of that sample is read; `out` keeps its bytes there.
 *   absent operand   an operand k whose coef0[k] and coef1[k] are both exactly zero (+0 or -0) in the sample's row is not loaded and
 *                    adds nothing to either form: its bytes may be anything, NaN and inf included (the history a request in its
 *                    multistep ramp-up does not have yet, the re-noising tensor on the last step, the original and the re-noising
 *                    tensor of a plain request that shares the batch).  The mask is always read for an active sample.
 *   operand order    the operands that are present are accumulated in slot order with the arithmetic of skr_step_launch_masked,
 *                    operation for operation: s over every present operand, one fma each (a present operand whose coef0 is zero
 *                    included), the noise last and skipped when the row's zeta0 narrows to zero; k over the present operands whose
 *                    coef1 is not exactly zero; out = fma(m, s, (1 - m) * k), rounded once.  A sample's result therefore has the bits
 *                    skr_step_launch_masked gives for that sample alone with a plan that holds exactly the present operands in that
 *                    order, with the row's values.
 * `plan` is therefore the WIDEST masked step of the sampler.  Index validity stays the caller's business: every non-negative
 * sample_index_dev[s] + row_offset must name a row of the table; the kernel neither checks nor clamps
 * (skrample_amd.rolling.RollingBatch validates on the host).
 */
int skr_step_launch_masked_rolling(const skr_step_plan* plan, const void* const* inputs, void* out,
                                   const skr_step_mask* mask, const uint64_t* seeds_dev, int64_t numel,
                                   const skr_step_row* rows_dev,
                                   const int32_t* sample_index_dev /* device int32[numel / sample_numel], < 0: inactive */,
                                   int32_t row_offset, void* stream);

/*
 * Step programs -- a plan the library keeps, launched by handle. Replaces the per-step host work of a REPLAYED step
 * (skrample/diffusers.py:565-599 redoes the whole step algebra every call; skrample_amd lowers each distinct step once,
 * sampling/program.py): the plan -- coefficients, dtypes, conversion kinds, sample size -- is handed over and validated once,
 * a launch passes only what changes from call to call: operand / output / seed pointers and the two Philox stream ids.
 * skr_program_launch(prog, ...) == skr_step_launch(plan with stream0 / stream1 replaced, ..., numel, stream), bit for bit.
 * A program is immutable after creation and may be launched from several threads; destroy it when no launch is in flight
 * on the host side (device work already enqueued is unaffected).
 */
typedef struct skr_program skr_program;
int skr_program_create(const skr_step_plan* plan, int64_t numel, skr_program** out);
int skr_program_launch(const skr_program* prog, const void* const* inputs, void* out0, void* out1,
                       const uint64_t* seeds_dev, uint64_t stream0, uint64_t stream1, void* stream);
void skr_program_destroy(skr_program* prog);

/*
 * Channels-last steps.  Every operand and output holds each sample as `plane` x `channels` elements with the channel innermost
 * (torch.channels_last / channels_last_3d storage): storage position p of a sample is the logical element
 *     l(p) = (p % channels) * plane + p / channels.
 * A step is elementwise, so over operands that share one dense layout only the Philox draw depends on the layout.  The output at p
 * has, bit for bit, the value skr_step_launch writes at l(p) for the same plan over the logically equal contiguous operands: same
 * operand slot order, one fma per operand, noise last, `chain`, one rounding -- and the normal of element l(p), so a seed gives the
 * same noise in either memory format.
 * Checks: those of skr_step_launch, in its order and with its codes; then a NULL layout SKR_ERR_NULL; channels < 1, plane < 1 or
 * channels * plane != plan->sample_numel SKR_ERR_SHAPE; a launch that draws with a non-zero convert_* SKR_ERR_UNSUPPORTED.
 * A launch that does not draw (noise_mode 0, both zetas zero, channels == 1 or plane == 1) is skr_step_launch itself.  A launch that
 * draws runs the one-trip channels-last kernel -- bf16 / fp16, one dtype for operands and out0, no out1, fp32 arithmetic, 1..8
 * operands, channels 4 / 8 / 16, plane % 4 == 0, whole 2048-element chunks, samples made of whole chunks -- or the general
 * grid-stride one (everything else skr_step_launch draws for); the two agree bit for bit, and skr_set_tuning("one_trip", 0) forces
 * the general kernel.
 */
typedef struct skr_step_layout {
  int64_t channels;  /* C: innermost storage axis of a sample */
  int64_t plane;     /* product of the other sample axes (H*W, D*H*W) */
} skr_step_layout;

int skr_step_launch_channels_last(const skr_step_plan* plan, const void* const* inputs,
                                  void* out0, void* out1, const uint64_t* seeds_dev,
                                  const skr_step_layout* layout, int64_t numel, void* stream);

/* A program that remembers the layout: skr_program_launch launches it as skr_step_launch_channels_last does.  The checks of
 * skr_program_create, then the layout's (NULL, channels, plane, convert_*) as above. */
int skr_program_create_channels_last(const skr_step_plan* plan, int64_t numel,
                                     const skr_step_layout* layout, skr_program** out);

/*
 * The masked step on channels-last operands: skr_step_launch_masked over operands and `out` that hold each sample as plane x channels,
 * channel innermost, exactly as for skr_step_launch_channels_last.  The mask stays in LOGICAL order and skr_step_mask is unchanged:
 * storage position p of sample s reads mask[s * batch_stride + l(p) % mask_numel].  A mask that spells out only trailing plane axes
 * (mask_numel divides plane: (B,1,H,W), (1,1,H,W), (H,W), (W,), or (B,1,1,H,W) over 5-D latents) therefore reads
 * mask[(p / channels) % mask_numel]; a full-size mask (mask_numel == sample_numel) reads mask[l(p)].
 * The output at p has, bit for bit, the value skr_step_launch_masked writes at l(p) for the same plan over the logically equal
 * contiguous operands and the same mask: s in slot order with one fma per operand and the noise last, k over the operands whose coef1
 * is not exactly zero, out = fma(m, s, (1 - m) * k) rounded once, and the normal of element l(p) (Philox block l >> 2, lane l & 3).
 * Checks, before any launch and without reading device memory: those of skr_step_launch_masked, in its order and with its codes; then
 * a NULL layout SKR_ERR_NULL; channels < 1, plane < 1 or channels * plane != plan->sample_numel SKR_ERR_SHAPE.  numel == 0 is SKR_OK
 * with nothing launched.
 * channels == 1 or plane == 1 (l(p) = p) is skr_step_launch_masked itself.  Otherwise the one-trip channels-last kernel runs -- bf16 /
 * fp16, one dtype for operands, mask and out, fp32 arithmetic, 1..8 operands, channels 4 / 8 / 16, plane % 4 == 0, whole 2048-element
 * chunks, samples made of whole chunks, mask_numel even and dividing plane -- or the general grid-stride one (everything else
 * skr_step_launch_masked accepts: fp32 tensors, fp64 accumulation, two dtype groups, up to SKR_ROW_TERMS operands, any channel count,
 * any plane, ragged sizes, full-size masks, odd mask_numel, a mask of another dtype); the two agree bit for bit, and
 * skr_set_tuning("one_trip", 0) forces the general kernel.  There are no row forms (indexed / per-sample / rolling) in channels-last.
 */
int skr_step_launch_masked_channels_last(const skr_step_plan* plan, const void* const* inputs, void* out,
                                         const skr_step_mask* mask, const uint64_t* seeds_dev,
                                         const skr_step_layout* layout, int64_t numel, void* stream);

/*
 * The guided step -- classifier-free guidance fused into the step launch.  A guided loop evaluates the network on a doubled batch,
 * splits the output into `uncond` and `cond` and forms, with three tensor ops,
 *     d = cond - uncond;   m = guidance_scale * d;   noise_pred = uncond + m
 * before the scheduler step reads noise_pred.  Guidance replaces one operand of the step's linear form by a value computed from two,
 * so one launch evaluates, with T the dtype of the dtype group `slot` lies in, u = inputs[slot][e], c = cond[e]:
 *
 *     p          = rn_T( u + rn_T( g_M * rn_T(c - u) ) )
 *     out[e]     = rn( sum_k coef0[k] * v_k + zeta0 * N(seed[s(e)], stream0, e) ),   v_slot = p,  v_k = inputs[k][e] otherwise
 *     guided_out[e] = p                                                              (when guided_out is given)
 *
 * Arithmetic of p: torch's.  Every operation is a separate one in the op-math type M -- fp32 for bf16, fp16 and fp32 tensors, fp64 for
 * fp64 tensors --, g_M is `scale` converted to M once, nothing is contracted (for T = float the multiply and the add stay two
 * instructions), and for a 16-bit T each fp32 result is rounded to fp32 first and to T after.  So p has the bits of the three torch
 * lines over tensors of dtype T with a Python-number scale.  Under acc_f64 with a 16-bit T the guidance is still fp32 op-math, and p is
 * widened exactly.
 * One exception, torch's own: for T = fp16 the elements from the last multiple of 2048 below numel on -- the partial last block of
 * torch's elementwise kernel on gfx950 -- have g_M * d rounded to fp16 ONCE, from the exact product, because torch's kernel fuses
 * the multiply with the conversion there.  The entry does the same for those elements, so p still has torch's bits on ragged sizes.
 * Arithmetic of out: that of skr_step_launch -- from zero, operands in slot order, one fma each, the noise term last (skipped when
 * zeta0 == 0), one rounding by the store.  `out` therefore has, bit for bit, what skr_step_launch writes for the same plan over the
 * operand list whose entry `slot` is a tensor holding p; guided_out is that tensor.
 * Plan contract (the masked launch's): out1_dtype must be SKR_NONE (`out` has out0_dtype); chain, zeta1 and convert_* must be zero
 * (SKR_ERR_UNSUPPORTED otherwise); coef1 is ignored; at most SKR_ROW_TERMS operands (SKR_ERR_TERMS beyond); the dtype groups are those
 * of skr_step_launch; sample_numel is read by a launch that draws only, with skr_step_launch's rules.
 * Guidance-only form: out0_dtype == SKR_NONE with out == NULL and n_terms == 1 (so slot == 0) stores p alone; guided_out is then
 * required, and nothing is drawn.
 * Launches of whole 2048-element chunks (samples made of whole chunks when the launch draws) with one 16- or 32-bit dtype for operands,
 * cond and both outputs and fp32 arithmetic take a one-trip vector kernel; everything else (ragged sizes, small samples, two dtype
 * groups, fp64, the guidance-only form) a grid-stride per-element kernel.  The two agree bit for bit ("one_trip" 0 forces the second).
 * Checked before the launch, without dereferencing device memory, in this order (skr_step_launch's, with what the guidance adds):
 *   a NULL plan or guide SKR_ERR_NULL;  a launch that draws without seeds SKR_ERR_NULL;  n_terms outside 0..SKR_ROW_TERMS or n_group_a
 *   outside 0..n_terms SKR_ERR_TERMS;  slot outside 0..n_terms-1 SKR_ERR_TERMS;  numel < 0 SKR_ERR_SHAPE;  no output at all (out0_dtype
 *   SKR_NONE and no guided_out) SKR_ERR_NULL;  a noise_mode other than 0 / 1, a second output, chain, zeta1, convert_*, a non-zero
 *   `reserved`, or out0_dtype SKR_NONE outside the guidance-only form SKR_ERR_UNSUPPORTED;  the sample size of a launch that draws
 *   SKR_ERR_SHAPE / SKR_ERR_UNSUPPORTED as in skr_step_launch;  numel == 0 SKR_OK with nothing launched;  a NULL inputs, operand, out or
 *   cond SKR_ERR_NULL;  a misaligned operand, out, cond or guided_out SKR_ERR_ALIGN;  a dtype combination skr_step_launch does not take
 *   -- an fp64 group, the slot's or not, without acc_f64 among them -- SKR_ERR_DTYPE.
 */
typedef struct skr_step_guidance {
  const void* cond;     /* device, 16-byte aligned; dtype, shape and layout of inputs[slot] */
  void* guided_out;     /* device, 16-byte aligned, that dtype; NULL: the guided prediction is not stored */
  double scale;         /* guidance scale g */
  int32_t slot;         /* inputs[slot] is uncond; the guided value takes ITS place in the sum */
  int32_t reserved;     /* 0 */
} skr_step_guidance;

int skr_step_launch_guided(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                           const uint64_t* seeds_dev, int64_t numel, void* stream);

/*
 * The guided step with device-resident scalars: skr_step_launch_guided as skr_step_launch_indexed and
 * skr_step_launch_indexed_per_sample make skr_step_launch, so that one captured classifier-free-guidance loop serves any schedule of its
 * length AND any guidance scale, keeps several of them resident and lets every sample follow its own.
 * What is frozen and what is data: `plan` fixes the structure only -- operand count and dtype groups, out0_dtype (out1_dtype must be
 * SKR_NONE), noise_mode, sample_numel, acc_f64 == 0, chain == zeta1 == 0, convert_* == 0.  guide->cond, guide->guided_out and guide->slot
 * are launch arguments, frozen into a captured graph (a device-resident slot would index the kernel's register arrays at run time).
 * The plan's coef0 / zeta0 / stream0 values and guide->scale are ignored; when the kernel runs it reads coef0[k], zeta0, stream0 and the
 * guidance scale from
 *     indexed      rows_dev[(index_dev ? index_dev[0] : 0) + row_offset]
 *     per sample   rows_dev[sample_index_dev[s] + row_offset]            for the workgroups of sample s
 * skr_step_row is used unchanged.  The guidance scale is the row's convert_k[0]: a guided launch has no rounded conversion (the plan's
 * convert_* must be zero), so that field is free.  The row's coef1, chain, zeta1, stream1 and convert_k[1..3] are not read.
 * Arithmetic: that of skr_step_launch_guided, and bit for bit what skr_step_launch_guided gives with the row's values in its plan and in
 * guide->scale: g is narrowed to fp32 once; the row's doubles are narrowed on the device with the conversion the host applies to a plan's
 * doubles; the operands are accumulated in slot order, one fma each, with p in the place of inputs[slot]; the noise comes last -- a row
 * whose zeta0 is exactly zero skips the draw, as in the other row forms --; one rounding by the store; guided_out = p when guided_out is
 * given.  A sample of a per-sample launch has the bits the indexed launch gives it with that row for the whole batch.
 * Covered: exactly what the one-trip kernel of skr_step_launch_guided takes -- whole 2048-element chunks (samples made of whole chunks when
 * noise_mode == 1), one 16- or 32-bit dtype for operands, cond and both outputs, fp32 arithmetic, 1..SKR_ROW_TERMS operands.  In the
 * per-sample entry a workgroup must lie inside one sample: plan->sample_numel must be a positive multiple of 2048 that divides numel, with
 * or without noise (SKR_ERR_SHAPE / SKR_ERR_UNSUPPORTED otherwise).  Anything else is SKR_ERR_UNSUPPORTED -- ragged sizes, two dtype
 * groups, fp64, acc_f64, the guidance-only form, "one_trip" 0 and fp32 tensors with "tile" 0 included: there is no grid-stride row form.
 * Checked before the launch, without dereferencing device memory, in the order and with the codes of skr_step_launch_guided; on top of
 * them a NULL rows_dev is SKR_ERR_NULL, a NULL sample_index_dev in the per-sample entry is SKR_ERR_NULL (both beside the NULL plan), a
 * launch with noise_mode == 1 needs seeds_dev whatever its rows hold, and a negative row_offset is SKR_ERR_UNSUPPORTED.
 * Index validity is the caller's business, as with skr_step_launch_indexed: index_dev[0] + row_offset, and every
 * sample_index_dev[s] + row_offset, must name a row of the table.  The kernel neither checks nor clamps an index -- an entry outside
 * the table reads whatever lies there (or faults) -- so validate on the host before uploading (skrample_amd.graphs.CapturedLoop does).
 */
int skr_step_launch_guided_indexed(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                   const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev,
                                   const int32_t* index_dev /* device int32, may be NULL */, int32_t row_offset, void* stream);

int skr_step_launch_guided_indexed_per_sample(const skr_step_plan* plan, const void* const* inputs, void* out,
                                              const skr_step_guidance* guide, const uint64_t* seeds_dev, int64_t numel,
                                              const skr_step_row* rows_dev,
                                              const int32_t* sample_index_dev /* device int32[numel / sample_numel] */,
                                              int32_t row_offset, void* stream);

/*
 * The guided step of a rolling batch: skr_step_launch_guided_indexed_per_sample with samples that may sit at different positions of
 * their guided loops, each under its own guidance scale, or be absent -- what skr_step_launch_rolling is to
 * skr_step_launch_indexed_per_sample.  Structure, coverage, checks, their order and their codes are those of
 * skr_step_launch_guided_indexed_per_sample: `plan` fixes the structure only, skr_step_row and skr_step_guidance are used unchanged (the
 * scale is the row's convert_k[0]; guide->scale is ignored; guide->cond, guide->guided_out and guide->slot are launch arguments), whole
 * 2048-element chunks, samples made of whole chunks with or without noise, one 16- or 32-bit dtype for operands, cond and both outputs,
 * fp32 arithmetic, 1..SKR_ROW_TERMS operands; anything else is SKR_ERR_UNSUPPORTED (ragged sizes, two dtype groups, fp64, acc_f64, the
 * guidance-only form, "one_trip" 0 and fp32 tensors with "tile" 0 included): there is no grid-stride form, so the fp16 ragged-tail rule
 * of skr_step_launch_guided cannot arise.  A NULL rows_dev or sample_index_dev is SKR_ERR_NULL, a negative row_offset
 * SKR_ERR_UNSUPPORTED, and a launch with noise_mode == 1 needs seeds_dev whatever its rows hold.  On top of that contract
 *   inactive sample  sample_index_dev[s] < 0 (tested before row_offset is added): the workgroups of sample s return before their
 *                    first vector-memory instruction.  No operand, cond, seed or row of that sample is read; `out` and `guided_out`
 *                    keep their bytes there.
 *   absent operand   an operand k != slot whose coef0[k] is exactly zero (+0 or -0) in the sample's row is neither loaded nor summed:
 *                    its bytes may be anything, NaN and inf included (the history a request in its multistep ramp-up does not have
 *                    yet, the slot's previous occupant's).  The row's coef1 is not read.  inputs[slot] and cond are always loaded for
 *                    an active sample, and p takes its one fma whatever coef0[slot] is, as in skr_step_launch_guided.
 *   operand order    the operands that are present are accumulated in slot order, one fma each, with p in the place of inputs[slot];
 *                    the noise comes last and is skipped when the row's zeta0 narrows to zero; one rounding by the store;
 *                    guided_out = p when guided_out is given.  An active sample therefore has, bit for bit, what
 *                    skr_step_launch_guided gives for that sample alone with a plan that holds exactly the present operands in that
 *                    order, the row's values and guide->scale = convert_k[0] -- in `out` and in `guided_out`.
 * `plan` is therefore the WIDEST guided step of the sampler.  Index validity stays the caller's business: every non-negative
 * sample_index_dev[s] + row_offset must name a row of the table; the kernel neither checks nor clamps
 * (skrample_amd.rolling.RollingBatch validates on the host).
 * Measured (profiles/rolling_guided.txt; 64 x 4x128x128 bf16, DPM-2): the launch takes 9.10 us where torch's three
 * lines plus skr_step_launch_rolling take 20.66 us (0.44; 6 tensor passes against 12); a RollingBatch tick with device-resident positions
 * 31.07 against 43.43 us; a host-published tick is host-bound (154.80 against 176.33 us, inside the run-to-run spread).
 */
int skr_step_launch_guided_rolling(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                   const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev,
                                   const int32_t* sample_index_dev /* device int32[numel / sample_numel], < 0: inactive */,
                                   int32_t row_offset, void* stream);

/*
 * Rescaled guidance -- the line that follows the three guidance lines in SDXL-style, v-prediction and zero-terminal-SNR pipelines
 * (diffusers' rescale_noise_cfg), with p the guided prediction, c = cond and phi = guidance_rescale:
 *     std_text = c.std(dim=all but 0, keepdim=True);   std_cfg = p.std(dim=all but 0, keepdim=True)
 *     resc = p * (std_text / std_cfg);                 p' = phi * resc + (1 - phi) * p
 * A whole-sample reduction has to finish before the elementwise part starts, so the fused form is two launches: the statistic below
 * (2 tensor passes), then skr_step_launch_guided_rescaled with its per-sample factor.
 *
 * skr_guidance_rescale_factor: per sample s -- the contiguous span of sample_numel elements s * sample_numel .. in storage order --
 *     p[e]        the guided value of skr_step_launch_guided, fp16 tail rule (by the element's index in the WHOLE launch) included: the
 *                 tensor torch would have taken the std of; T = dtype, M its op-math type (fp32; fp64 for fp64 tensors), g_M = scale in M
 *     std_x       the unbiased (n - 1) standard deviation of the T-valued elements x = c, p of the sample, accumulated in DOUBLE as the
 *                 shifted sums S1 = sum(x - K), S2 = sum((x - K)^2) with the pivot K = the sample's first element (a sample whose mean
 *                 is far above its std does not cancel);  var = max((S2 - S1 * S1 / n) / (n - 1), 0), std = sqrt(var), each operation
 *                 a separate IEEE double operation
 *     r           rn_T( div_M( rn_T(rn_M(std_c)), rn_T(rn_M(std_p)) ) ): IEEE division, nothing guarded -- std_p == 0 gives the inf or
 *                 NaN torch gives
 *     factor_dev[s] = r;   stats_dev[2 s] = std_c, stats_dev[2 s + 1] = std_p when stats_dev is given
 * Order of summation (fixed: two stages, no atomics; it depends on sample_numel and dtype only -- not on the batch, the sample's
 * position or alignment, a grid heuristic or any skr_set_tuning key -- so a sample has the same factor bits alone and inside any batch):
 *   stage 1  one workgroup of 256 lanes per 2048-element span j of a sample (span j holds the sample's elements 2048 j .. 2048 j + 2047,
 *            the last one what is left).  Lane t owns the span's elements 8 t .. 8 t + 7 and adds them in that order to four running
 *            doubles that start at zero (S1 += d, then S2 = fma(d, d, S2), for c and for p).  The 64 lanes of a wave are reduced by a
 *            shuffle tree, v += v[lane + o] for o = 32, 16, 8, 4, 2, 1; the four waves through LDS as ((w0 + w1) + w2) + w3.  Four
 *            doubles per span go to partials_dev: S1c, S2c, S1p, S2p at 4 * (s * spans + j), spans = ceil(sample_numel / 2048).
 *            A span that is 16-byte aligned and whole is read with 16-byte non-temporal loads, any other element by element: same
 *            lanes, same order, same bits.
 *   stage 2  one wave per sample: each of the four quantities is summed over the sample's spans in index order from zero.
 * partials_dev: SKR_GUIDANCE_PARTIALS(numel, sample_numel) doubles of device workspace, 8-byte aligned, overwritten.
 * Checked before the launch, without dereferencing device memory: a NULL uncond, cond, factor_dev or partials_dev SKR_ERR_NULL;
 * numel < 0, sample_numel < 2 or numel % sample_numel != 0 SKR_ERR_SHAPE;  numel == 0 SKR_OK with nothing launched;  uncond or cond
 * not 16-byte aligned SKR_ERR_ALIGN;  a dtype other than bf16, fp16, fp32 or fp64 SKR_ERR_DTYPE;  more than INT32_MAX spans in all
 * SKR_ERR_UNSUPPORTED.  Allocates nothing, never synchronises: capturable.
 */
#define SKR_GUIDANCE_PARTIALS(numel, sample_numel) (4 * ((numel) / (sample_numel)) * (((sample_numel) + 2047) / 2048))

int skr_guidance_rescale_factor(const void* uncond, const void* cond, int32_t dtype, double scale, int64_t numel, int64_t sample_numel,
                                void* factor_dev /* T[numel / sample_numel] */,
                                double* stats_dev /* [2 * samples]: std(cond), std(p); may be NULL */,
                                double* partials_dev /* [SKR_GUIDANCE_PARTIALS(numel, sample_numel)] */, void* stream);

/*
 * skr_step_launch_guided_rescaled: skr_step_launch_guided with p replaced by p'.  With r = factor_dev[s(e)], phi_M = phi and
 * psi_M = 1.0 - phi (evaluated in double, as Python evaluates 1 - guidance_rescale before torch sees it) each narrowed to M once:
 *     resc = rn_T(p * r);   a = rn_T(phi_M * resc);   b = rn_T(psi_M * p);   p' = rn_T(a + b)
 * every operation a separate one in M, each result rounded to fp32 and then to T, nothing contracted.  `out` has the bits
 * skr_step_launch writes with a tensor holding p' in `slot`; guided_out = p' (what history and pred_original_sample read).  phi == 0
 * is not special-cased.  fp16: p * r is a product of two fp16 values -- exact in fp32, so no rule applies; the two scalar products are
 * torch's tensor-times-Python-number kernel, as g * d is, and have its single rounding from the last multiple of 2048 below numel on.
 * Launches the one-trip kernel of skr_step_launch_guided takes, with rescale->sample_numel a multiple of 2048 below 2^31 -- a
 * workgroup then lies inside one sample and the factor is one uniform load -- take a one-trip kernel of the same shape; everything
 * else (ragged sizes, small samples, two dtype groups, fp64, the guidance-only form) the grid-stride per-element kernel.  The two
 * agree bit for bit ("one_trip" 0 forces the second).
 * Checks: those of skr_step_launch_guided, in its order and with its codes; among them a NULL rescale beside the NULL plan or guide
 * SKR_ERR_NULL; a non-zero rescale->reserved beside the guide's SKR_ERR_UNSUPPORTED; behind the sample size of a launch that draws:
 * rescale->sample_numel < 2 or not dividing numel SKR_ERR_SHAPE, then a drawing plan whose sample_numel differs SKR_ERR_SHAPE;
 * a NULL factor_dev beside the NULL operands SKR_ERR_NULL.  factor_dev needs the alignment of T only.
 */
typedef struct skr_step_rescale {
  const void* factor_dev;  /* device T[numel / sample_numel]: what skr_guidance_rescale_factor wrote */
  double phi;              /* guidance_rescale */
  int64_t sample_numel;    /* elements per sample of the statistic */
  int64_t reserved;        /* 0 */
} skr_step_rescale;

int skr_step_launch_guided_rescaled(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                    const skr_step_rescale* rescale, const uint64_t* seeds_dev, int64_t numel, void* stream);

/*
 * Rescaled guidance in a rolling batch: the two launches above with every per-request scalar taken from the sample's row,
 * rows_dev[sample_index_dev[s] + row_offset] -- convert_k[0] the guidance scale (as in skr_step_launch_guided_rolling), convert_k[1]
 * phi = guidance_rescale (skr_step_launch_guided_rolling does not read it).  convert_k[2..3], coef1, chain, zeta1 and stream1 are not
 * read.  Neither entry has a grid-stride form.  A tick is the statistics launch, then the step launch, with the same index, rows and
 * row_offset; index validity is the caller's business, as in skr_step_launch_guided_rolling.
 *
 * skr_guidance_rescale_factor_rolling: skr_guidance_rescale_factor with the scale of sample s its row's convert_k[0], and
 *   inactive sample    sample_index_dev[s] < 0 (tested before row_offset is added): every workgroup of the sample, in both stages,
 *                      returns before its first vector-memory instruction.  Nothing of the sample is read; factor_dev[s],
 *                      stats_dev[2 s .. 2 s + 1] and the sample's partials keep their bytes.
 *   unrescaled sample  the row's convert_k[1] is exactly zero (+0 or -0): the same exit in both stages.  A request that does not
 *                      rescale costs no statistics traffic, and its factor is never written.
 *   active, rescaled   factor_dev[s] -- and stats_dev[2 s .. 2 s + 1] when given -- have, bit for bit, what
 *                      skr_guidance_rescale_factor writes for that sample alone with scale = convert_k[0]: the documented order of
 *                      summation (2048-element spans, lane t owning elements 8 t .. 8 t + 7, the shuffle tree o = 32 .. 1,
 *                      ((w0 + w1) + w2) + w3, stage 2 in span order) and the partials layout SKR_GUIDANCE_PARTIALS, unchanged.
 * Coverage is the rolling step's: bf16, fp16 or fp32, sample_numel a positive multiple of 2048 that divides numel.  Every span is then
 * whole and 16-byte aligned -- the kernels have the vector path only -- and the fp16 tail rule cannot arise (numel % 2048 == 0).
 * Checked before the launch, without dereferencing device memory, in this order: a NULL uncond, cond, factor_dev, partials_dev,
 * rows_dev or sample_index_dev SKR_ERR_NULL;  numel < 0, sample_numel < 2 or sample_numel not dividing numel SKR_ERR_SHAPE;
 * numel == 0 SKR_OK with nothing launched;  uncond or cond not 16-byte aligned SKR_ERR_ALIGN;  a dtype that is no tensor dtype
 * SKR_ERR_DTYPE;  fp64, sample_numel % 2048 != 0, a negative row_offset or more than INT32_MAX spans SKR_ERR_UNSUPPORTED.
 * Allocates nothing, never synchronises: capturable.
 */
int skr_guidance_rescale_factor_rolling(const void* uncond, const void* cond, int32_t dtype, int64_t numel, int64_t sample_numel,
                                        const skr_step_row* rows_dev,
                                        const int32_t* sample_index_dev /* device int32[numel / sample_numel], < 0: inactive */,
                                        int32_t row_offset, void* factor_dev /* T[numel / sample_numel] */,
                                        double* stats_dev /* [2 * samples]: std(cond), std(p); may be NULL */,
                                        double* partials_dev /* [SKR_GUIDANCE_PARTIALS(numel, sample_numel)] */, void* stream);

/*
 * skr_step_launch_guided_rescaled_rolling: skr_step_launch_guided_rolling whose guided value is p' for the samples that rescale.
 * Structure, coverage, checks, their order and their codes are those of skr_step_launch_guided_rolling; on top of them, in the places
 * where skr_step_launch_guided_rescaled puts its own: a NULL rescale SKR_ERR_NULL (beside the NULL plan), a non-zero
 * rescale->reserved SKR_ERR_UNSUPPORTED, a NULL rescale->factor_dev SKR_ERR_NULL (beside the NULL operands), and
 * rescale->sample_numel != plan->sample_numel SKR_ERR_SHAPE.  rescale->phi and guide->scale are ignored: both are row values.
 * Inactive sample, absent operand and operand order are exactly those of skr_step_launch_guided_rolling, and
 *   rescaled sample    the row's convert_k[1] is not +-0.  phi_M is that value narrowed once, psi_M = 1.0 - convert_k[1] formed in
 *                      double on the device and narrowed once, r = factor_dev[s] one uniform load behind the operand loads, and
 *                      p' = rn_T(rn_T(phi_M * rn_T(p * r)) + rn_T(psi_M * p)) as in skr_step_launch_guided_rescaled.  `out` and
 *                      `guided_out` have, bit for bit, what skr_step_launch_guided_rescaled gives that sample alone with a plan
 *                      holding exactly the present operands in order, the row's values, guide->scale = convert_k[0] and
 *                      rescale = {&factor_dev[s], convert_k[1], sample_numel, 0}.
 *   unrescaled sample  the row's convert_k[1] is exactly +-0.  factor_dev[s] is NOT read -- it may hold NaN or be uninitialised --,
 *                      p' = p, and the sample has the bits skr_step_launch_guided_rolling gives it.  A branch, uniform over the
 *                      workgroup, not arithmetic: 0 * inf does not leak through.
 */
int skr_step_launch_guided_rescaled_rolling(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                            const skr_step_rescale* rescale, const uint64_t* seeds_dev, int64_t numel,
                                            const skr_step_row* rows_dev,
                                            const int32_t* sample_index_dev /* device int32[numel / sample_numel], < 0: inactive */,
                                            int32_t row_offset, void* stream);

/*
 * Rescaled guidance in captured loops: the two launches of rescaled guidance with every per-row scalar taken from the row that
 * skr_step_launch_guided_indexed[_per_sample] reads --
 *     indexed      rows_dev[(index_dev ? index_dev[0] : 0) + row_offset]
 *     per sample   rows_dev[sample_index_dev[s] + row_offset]            for the workgroups of sample s
 * -- convert_k[0] the guidance scale, convert_k[1] phi = guidance_rescale (skr_step_launch_guided_indexed[_per_sample] do not read it).
 * convert_k[2..3], coef1, chain, zeta1 and stream1 are not read.  A captured loop then serves any schedule, any scale and any
 * guidance_rescale, zero included, without a re-capture.  A step is the statistics launch, then the step launch, with the same index,
 * rows and row_offset.  There is no inactive-sample semantic: every index names a row.  Index validity is the caller's business, as with
 * skr_step_launch_guided_indexed: index_dev[0] + row_offset, and every sample_index_dev[s] + row_offset, must name a row of the table;
 * the kernels neither check nor clamp an index (skrample_amd.graphs.CapturedLoop validates on the host).  No entry has a grid-stride form.
 *
 * skr_guidance_rescale_factor_indexed[_per_sample]: skr_guidance_rescale_factor with the scale of sample s its row's convert_k[0], and
 *   unrescaled row   the row's convert_k[1] is exactly zero (+0 or -0): every workgroup that reads the row, in both stages, returns
 *                    before its first vector-memory instruction -- in the indexed form every workgroup of the launch.  Nothing is
 *                    read; factor_dev, stats_dev and the partials keep their bytes there.
 *   rescaled row     factor_dev[s] -- and stats_dev[2 s .. 2 s + 1] when given -- and the sample's partials have, bit for bit, what
 *                    skr_guidance_rescale_factor writes for that sample alone with scale = convert_k[0]: the documented order of
 *                    summation and the partials layout SKR_GUIDANCE_PARTIALS, unchanged.
 * Coverage and checks are those of skr_guidance_rescale_factor_rolling, in its order and with its codes: bf16, fp16 or fp32,
 * sample_numel a positive multiple of 2048 that divides numel; a NULL uncond, cond, factor_dev, partials_dev or rows_dev -- or a NULL
 * sample_index_dev in the per-sample entry; index_dev may be NULL -- SKR_ERR_NULL;  numel < 0, sample_numel < 2 or sample_numel not
 * dividing numel SKR_ERR_SHAPE;  numel == 0 SKR_OK with nothing launched;  uncond or cond not 16-byte aligned SKR_ERR_ALIGN;  a dtype
 * that is no tensor dtype SKR_ERR_DTYPE;  fp64, sample_numel % 2048 != 0, a negative row_offset or more than INT32_MAX spans
 * SKR_ERR_UNSUPPORTED.  Allocates nothing, never synchronises: capturable.
 */
int skr_guidance_rescale_factor_indexed(const void* uncond, const void* cond, int32_t dtype, int64_t numel, int64_t sample_numel,
                                        const skr_step_row* rows_dev, const int32_t* index_dev /* device int32, may be NULL */,
                                        int32_t row_offset, void* factor_dev /* T[numel / sample_numel] */,
                                        double* stats_dev /* [2 * samples]: std(cond), std(p); may be NULL */,
                                        double* partials_dev /* [SKR_GUIDANCE_PARTIALS(numel, sample_numel)] */, void* stream);

int skr_guidance_rescale_factor_indexed_per_sample(const void* uncond, const void* cond, int32_t dtype, int64_t numel, int64_t sample_numel,
                                                   const skr_step_row* rows_dev,
                                                   const int32_t* sample_index_dev /* device int32[numel / sample_numel] */,
                                                   int32_t row_offset, void* factor_dev /* T[numel / sample_numel] */,
                                                   double* stats_dev /* [2 * samples]: std(cond), std(p); may be NULL */,
                                                   double* partials_dev /* [SKR_GUIDANCE_PARTIALS(numel, sample_numel)] */, void* stream);

/*
 * skr_step_launch_guided_rescaled_indexed[_per_sample]: skr_step_launch_guided_indexed[_per_sample] whose guided value is p' when the
 * row rescales.  Structure, coverage, checks, their order and their codes are those of skr_step_launch_guided_indexed[_per_sample]; on
 * top of them, in the places where skr_step_launch_guided_rescaled_rolling puts them: a NULL rescale SKR_ERR_NULL (beside the NULL
 * plan), a non-zero rescale->reserved SKR_ERR_UNSUPPORTED, a NULL rescale->factor_dev SKR_ERR_NULL (beside the NULL operands), and
 * rescale->sample_numel != plan->sample_numel SKR_ERR_SHAPE.  The factor is per sample, so in BOTH entries a workgroup must lie inside
 * one sample: plan->sample_numel must be a positive multiple of 2048 that divides numel, with or without noise (SKR_ERR_SHAPE /
 * SKR_ERR_UNSUPPORTED otherwise).  rescale->phi and guide->scale are ignored: both are row values.  Every operand takes its fma, zero
 * coefficients included: there is no absent-operand rule here.
 *   rescaled row     the row's convert_k[1] is not +-0.  phi_M is that value narrowed once, psi_M = 1.0 - convert_k[1] formed in double
 *                    on the device and narrowed once, r = factor_dev[s] one uniform load behind the operand loads, and
 *                    p' = rn_T(rn_T(phi_M * rn_T(p * r)) + rn_T(psi_M * p)) as in skr_step_launch_guided_rescaled.  `out` and
 *                    `guided_out` have, bit for bit, what skr_step_launch_guided_rescaled gives with the row's values in its plan, in
 *                    guide->scale and in rescale->phi -- for a sample of the per-sample entry: that launch on the sample alone with
 *                    rescale->factor_dev = &factor_dev[s].
 *   unrescaled row   the row's convert_k[1] is exactly +-0.  factor_dev is NOT read -- it may hold NaN or be uninitialised --, p' = p,
 *                    and the launch (the sample) has the bits skr_step_launch_guided_indexed[_per_sample] gives it.  A branch, uniform
 *                    over the workgroup, not arithmetic: 0 * inf does not leak through.
 */
int skr_step_launch_guided_rescaled_indexed(const skr_step_plan* plan, const void* const* inputs, void* out, const skr_step_guidance* guide,
                                            const skr_step_rescale* rescale, const uint64_t* seeds_dev, int64_t numel,
                                            const skr_step_row* rows_dev, const int32_t* index_dev /* device int32, may be NULL */,
                                            int32_t row_offset, void* stream);

int skr_step_launch_guided_rescaled_indexed_per_sample(const skr_step_plan* plan, const void* const* inputs, void* out,
                                                       const skr_step_guidance* guide, const skr_step_rescale* rescale,
                                                       const uint64_t* seeds_dev, int64_t numel, const skr_step_row* rows_dev,
                                                       const int32_t* sample_index_dev /* device int32[numel / sample_numel] */,
                                                       int32_t row_offset, void* stream);

/*
 * A solver step replayed one rounded tensor operation at a time -- the reference's arithmetic when its samplers are called on tensors
 * directly (StructuredSampler.sample, skrample/sampling/structured.py:70-86 with :167-497 and models.py:53-224; no scheduler wrapper,
 * or a wrapper with compute_scale=None): every `*`, `+`, `-`, `/` is a torch op of its own in the TENSOR dtype -- operands widened to the
 * op-math type (fp32 for bf16 / fp16 / fp32 tensors, fp64 for fp64; a Python scalar is converted to it first), one operation, the result
 * rounded to the tensor dtype.  skr_step_launch evaluates the collapsed form in fp32 and rounds once (closer to the exact value, not
 * the reference's bits); skr_tape_launch runs the recorded sequence itself, values on chip (a register file in LDS), one pass over HBM:
 *
 *     LOAD   r[dst] = inputs[a][e]                        STORE  outputs[b][e] = r[a]
 *     MUL_S  r[dst] = rnd(r[a] * k)    DIV_S  rnd(r[a] / k)    ADD_S  rnd(r[a] + k)    RSUB_S  rnd(k - r[a])    RDIV_S  rnd(k / r[a])
 *     ADD    r[dst] = rnd(r[a] + r[b]) SUB    rnd(r[a] - r[b]) MUL    rnd(r[a] * r[b]) DIV     rnd(r[a] / r[b]) NEG     -r[a]
 *     ADD_MS r[dst] = rnd(r[a] + rnd(r[b] * k))   SUB_MS  rnd(r[a] - rnd(r[b] * k))   RSUB_MS  rnd(rnd(r[b] * k) - r[a])   MULZ_S  rnd(rnd(r[a] * k) + 0)
 *       (two ops of the lines above in one visit, for a product nothing else reads: `total + p * q`, `s - sigma * o`, `0 + p * q` -- same roundings)
 *
 * (IEEE operations, no contraction; rnd = round-to-nearest-even to `dtype`.  The scalar k: converted to the op-math type for MUL_S / DIV_S /
 * RDIV_S, but rounded to `dtype` FIRST for ADD_S / RSUB_S -- torch's add / sub / rsub of a Python number to a 16-bit CPU tensor do that, its
 * mul / div do not.)  Every tensor has `dtype` and `numel` elements; register
 * numbers are < SKR_TAPE_REGS (the host allocates them); SKR_ERR_TERMS for a malformed tape.
 */
#define SKR_TAPE_MAX_OPS 96
#define SKR_TAPE_REGS 16
#define SKR_TAPE_MAX_INPUTS 24
#define SKR_TAPE_MAX_OUTPUTS 4
enum skr_tape_code {
  SKR_TAPE_LOAD = 0, SKR_TAPE_STORE = 1, SKR_TAPE_MUL_S = 2, SKR_TAPE_DIV_S = 3, SKR_TAPE_ADD_S = 4, SKR_TAPE_RSUB_S = 5, SKR_TAPE_RDIV_S = 6,
  SKR_TAPE_ADD = 7, SKR_TAPE_SUB = 8, SKR_TAPE_MUL = 9, SKR_TAPE_DIV = 10, SKR_TAPE_NEG = 11,
  SKR_TAPE_ADD_MS = 12, SKR_TAPE_SUB_MS = 13, SKR_TAPE_RSUB_MS = 14, SKR_TAPE_MULZ_S = 15
};
typedef struct skr_tape_op {
  int32_t code; /* skr_tape_code */
  int32_t dst, a, b;
  double k;
} skr_tape_op;
typedef struct skr_tape {
  int32_t n_ops, n_inputs, n_outputs;
  int32_t dtype; /* skr_dtype of every tensor */
  skr_tape_op ops[SKR_TAPE_MAX_OPS];
} skr_tape;
int skr_tape_launch(const skr_tape* tape, const void* const* inputs, void* const* outputs, int64_t numel, void* stream);

/*
 * Noise generators -- replace skrample/pytorch/noise.py behind BatchTensorNoise.generate
 * (noise.py:438-446) / SkrampleWrapperCore.get_step_noise (diffusers.py:312-346).
 * One launch (or a short fixed chain of launches) produces the whole [batch, *unit] tensor; every
 * reduction is per sample.  `seeds_dev` holds one 64-bit seed per batch item; `stream` numbers the
 * draw (the wrapper passes the step index) so repeated calls give fresh, reproducible noise.
 * Output dtype, every entry below (skr_noise_random, _brownian, _offset, _pyramid*, _colored*, skr_colorize and the rolling forms):
 * all arithmetic is fp32 and does not depend on out_dtype; a bf16 / fp16 element is the fp32 value rounded ONCE to nearest even, a
 * float64 element the fp32 value widened -- on every store path (packed or scalar, any alignment of `out`, any position of the sample
 * in the batch).  So draw(bf16 / fp16) has the bits of RNE(draw(fp32)), and a sample's bits depend on its seed and streams alone.
 * Exception, float64 only: the Colored plane kernels exist for double in their run-time-geometry form alone and colored_inverse128
 * not at all, so a float64 draw of those planes agrees with the fp32 draw to fp32 rounding (tests/test_noise_dtype_contract_gpu.py).
 */

/* Random.generate (noise.py:58-74): out = N() */
int skr_noise_random(void* out, int32_t out_dtype, const uint64_t* seeds_dev, uint64_t stream_id,
                     int64_t batch, int64_t sample_numel, void* stream);

/* Brownian.generate (noise.py:210-242; the tree itself is torchsde.BrownianInterval, an un-vendored dependency):
 *   out = scale * (S_to - S_from),   S_x = sum_{k < n_streams} weights_x[k] * N(stream_ids[k])
 * The Brownian path W(t) on [0,1] is a fixed linear function of per-node normals (terminal value + one
 * Brownian-bridge midpoint normal per dyadic interval), so W(t) is a weighted sum of at most depth+1 node normals; the
 * host walks the tree in fp64 and passes the node stream ids (ascending) with each endpoint's weights (host pointers,
 * copied into the launch; a node off one endpoint's path has weight 0 there).  n_streams <= 64.
 * cache_f32 (optional, [batch*sample_numel] fp32, updated in place) receives S_to; with from_cache != 0 it is read as
 * S_from first (weights_from may then be null) -- the sequential-steps case, where each query starts where the last
 * one ended, costs one path instead of two.  Cache hits and misses produce identical bits. */
#define SKR_MAX_WEIGHTED_STREAMS 64
int skr_noise_brownian(void* out, int32_t out_dtype, const uint64_t* seeds_dev, const uint64_t* stream_ids,
                       const double* weights_to, const double* weights_from, int32_t n_streams, double scale,
                       float* cache_f32, int32_t from_cache, int64_t batch, int64_t sample_numel, void* stream);

/* Offset.generate (noise.py:84-113): out = N(stream_base) + strength^2 * N(stream_offset)[broadcast].
 * `unit_shape[ndim]` (ndim <= 4) is the per-sample shape; bit k of keep_mask set = dimension k of the unit
 * shape keeps its size in the offset tensor (reference OffsetProps.dims), otherwise it is broadcast. */
int skr_noise_offset(void* out, int32_t out_dtype, const uint64_t* seeds_dev, uint64_t stream_base,
                     uint64_t stream_offset, int64_t batch, const int64_t* unit_shape, int32_t ndim,
                     uint32_t keep_mask, double strength, void* stream);

/* skr_noise_offset for a rolling batch: every sample at its own draw, inactive samples at no cost.  sample_index_dev[batch] is the vector a
 * skr_step_launch_rolling reads (published by the host, or computed by skr_rolling_advance; no other device state).  For every sample b:
 *   inactive  sample_index_dev[b] < 0: the workgroups of sample b return on a scalar branch before their first vector-memory
 *             instruction and before any LDS or Philox work.  Nothing of the sample is read, its seed included; `out` keeps its bytes there.
 *   active    its draw number is d = sample_index_dev[b] - b * rows_per_slot, the sample's position in its own run (the caller guarantees
 *             0 <= d < rows_per_slot; skrample_amd.rolling.RollingBatch and skr_rolling_advance validate it), and its streams are those of
 *             draw d of a whole-batch generator: stream_base = d * stream_stride, stream_offset = stream_base + 1, or 1 (the first
 *             draw's) with static_offset != 0.
 * An active sample's slice of `out` has the bits skr_noise_offset writes for that sample alone (batch 1, its seed, those streams): the
 * same kernel code behind one scalar load, independent of the slot and of which other slots are active.  Covered: what the aligned
 * kernel of skr_noise_offset covers -- the innermost axis of unit_shape a multiple of 8, a unit below 2^31 elements, batch <= 65535,
 * `out` 16-byte aligned -- in bf16, fp16 or fp32; anything else, SKR_F64 included, is SKR_ERR_UNSUPPORTED.
 * Checked before the launch, without dereferencing device memory: rows_per_slot < 1, stream_stride == 0 or
 * batch * rows_per_slot > INT32_MAX is SKR_ERR_SHAPE; then the checks of skr_noise_offset in their order (batch == 0 or an empty unit
 * is SKR_OK with nothing launched); a NULL sample_index_dev is SKR_ERR_NULL.  Allocates nothing, never synchronises: capturable. */
int skr_noise_offset_rolling(void* out, int32_t out_dtype, const uint64_t* seeds_dev,
                             const int32_t* sample_index_dev /* device int32[batch], < 0: inactive */, int32_t rows_per_slot,
                             uint64_t stream_stride, int32_t static_offset, int64_t batch, const int64_t* unit_shape, int32_t ndim,
                             uint32_t keep_mask, double strength, void* stream);

/* Pyramid.generate (noise.py:146-207) over the last two dims (resize_h = 1) or the last dim (resize_h = 0,
 * h must be 1) of a [batch][lead][h][w] tensor:
 *   out = (N(base) + sum_{l >= skip} strength^l * upsample_bilinear(N(level l)))  /  per-sample unbiased std
 * The base normal is stream_base+0; the pyramid component uses stream_levels (= stream_base for a fresh pyramid
 * per draw, the first draw's id for PyramidProps.static): geometry uniforms = stream_levels+255, level l normals
 * (stream_levels+1+l, shape [lead][h_l][w_l]) are generated into LDS and sampled there; level 0 is full resolution;
 * skip = max(0, n_levels-1-depth).  Workspaces: scratch_f32 [batch*lead*h*w], partials_f64 [batch*lead*2],
 * level_ws int32 [batch*17] (receives the level table, readable for tests).  with_base = 0 returns the un-normalised
 * pyramid component alone (reference Pyramid.pyramid(), noise.py:146-200).  Limits: w % 4 == 0 and
 * about h*w <= 380*380 (the level stage must fit 152 KiB of LDS); returns SKR_ERR_UNSUPPORTED beyond them --
 * skr_noise_pyramid_any below covers every shape. */
int skr_noise_pyramid(void* out, int32_t out_dtype, float* scratch_f32, double* partials_f64, int32_t* level_ws,
                      const uint64_t* seeds_dev, uint64_t stream_base, uint64_t stream_levels, int64_t batch,
                      int64_t lead, int64_t h, int64_t w, int32_t resize_h, double strength, int32_t depth,
                      int32_t with_base, void* stream);

/* skr_noise_pyramid (with_base = 1) for a rolling batch, under the contract of skr_noise_offset_rolling: sample b is inactive when
 * sample_index_dev[b] < 0 -- its workgroups of pass 1 AND of the normalising pass return on a scalar branch before their first
 * vector-memory instruction and before any LDS or Philox work; neither its seed, nor level_ws, nor its partials are read, and `out`,
 * scratch_f32, partials_f64 and level_ws keep their bytes there -- else its draw number is d = sample_index_dev[b] - b * rows_per_slot
 * and its streams are stream_base = d * stream_stride, stream_levels = stream_base, or 0 (the first draw's) with static_levels != 0.
 * An active sample's slice of `out` has the bits skr_noise_pyramid writes for that sample alone (batch 1, its seed, those streams): the
 * same five pass-1 forms, picked by the same route decision, and the same normalising pass, behind one scalar load.  Workspaces as for
 * skr_noise_pyramid.  Covered: what skr_noise_pyramid covers, in bf16, fp16 or fp32; a shape its LDS route refuses and SKR_F64 are
 * SKR_ERR_UNSUPPORTED with nothing launched (there is no rolling form of the any-shape kernels).
 * Checked before any launch, without dereferencing device memory: rows_per_slot < 1, stream_stride == 0 or
 * batch * rows_per_slot > INT32_MAX is SKR_ERR_SHAPE; then the checks of skr_noise_pyramid in their order (batch == 0 is SKR_OK with
 * nothing launched; sample_index_dev is one of the pointers: NULL is SKR_ERR_NULL), then the output type.  Capturable. */
int skr_noise_pyramid_rolling(void* out, int32_t out_dtype, float* scratch_f32, double* partials_f64, int32_t* level_ws,
                              const uint64_t* seeds_dev, const int32_t* sample_index_dev /* device int32[batch], < 0: inactive */,
                              int32_t rows_per_slot, uint64_t stream_stride, int32_t static_levels, int64_t batch, int64_t lead,
                              int64_t h, int64_t w, int32_t resize_h, double strength, int32_t depth, void* stream);

/* What the two rolling entries answer for a batch of such units, with nothing launched and no pointer looked at: their own shape checks
 * and route decision (SKR_OK, SKR_ERR_SHAPE, or SKR_ERR_UNSUPPORTED for a unit outside the aligned Offset kernel / a plane the LDS route of
 * the Pyramid kernels refuses).  A caller that owns long-lived buffers (skrample_amd.rolling.RollingBatch) asks before it allocates them. */
int skr_noise_offset_rolling_covers(int64_t batch, const int64_t* unit_shape, int32_t ndim);
int skr_noise_pyramid_rolling_covers(int64_t batch, int64_t lead, int64_t h, int64_t w, int32_t resize_h);

/* Same generator for any plane size and width (no `w % 4`, no LDS limit): the level normals are generated into
 * levels_f32 ([batch * lead*h*w] fp32) and sampled from global memory.  partials_f64 = [batch * n_slots * 2],
 * n_slots (1..65535) = workgroups per sample of the main pass.  Same values as skr_noise_pyramid where both apply
 * (up to the summation order of the per-sample statistics). */
int skr_noise_pyramid_any(void* out, int32_t out_dtype, float* scratch_f32, float* levels_f32, double* partials_f64,
                          int32_t n_slots, int32_t* level_ws, const uint64_t* seeds_dev, uint64_t stream_base,
                          uint64_t stream_levels, int64_t batch, int64_t lead, int64_t h, int64_t w, int32_t resize_h,
                          double strength, int32_t depth, int32_t with_base, void* stream);

/* Pyramid over ANY one or two axes of the unit (reference noise.py:146-193: the resized axes are permuted to the end,
 * interpolated slice by slice and permuted back; level l normals are drawn in the unit's own axis order, reduced sizes on the
 * resized axes).  unit_shape[ndim] (ndim <= 4; merge adjacent untouched axes), axis_a < axis_b the resized axes (axis_a = -1:
 * only axis_b).  Same streams, level geometry, workspaces and normalisation as skr_noise_pyramid_any, which is the special
 * case unit_shape = (lead, h, w), axes (1, 2). */
int skr_noise_pyramid_nd(void* out, int32_t out_dtype, float* scratch_f32, float* levels_f32, double* partials_f64, int32_t n_slots,
                         int32_t* level_ws, const uint64_t* seeds_dev, uint64_t stream_base, uint64_t stream_levels, int64_t batch,
                         int32_t ndim, const int64_t* unit_shape, int32_t axis_a, int32_t axis_b, double strength, int32_t depth,
                         int32_t with_base, void* stream);

/* Colored.generate / colorize_noise (noise.py:337-425): white Philox noise shaped in the Fourier domain by
 * clamp(radial_frequency, eps)^(-exponent/2) and rescaled per sample to the white noise's std (or `energy`).
 * The per-sample transform is over (d1, d2, d3) (d1 = 1 for a 2-D unit).  Covered by the hand-written LDS transforms: every axis a
 * power of two <= 4096; or d1 a power of two <= 16 (or 1) over planes whose sides are 2^a * r, r odd <= 63, with d2 even and
 * d3 a multiple of 4 (every such side up to 126 / 252, then 96 * 2^k, 160 * 2^k ...: 90, 96, 104, 112, 144, 152, 160, 168, 192 ...) as long as one plane fits a CU's LDS (up to 192 x 192).  Other shapes:
 * SKR_ERR_UNSUPPORTED -- use skr_noise_colored_any.
 * Workspaces (caller-provided): spec_c64 = batch*d1*d2*(d3/2+1) complex64, scratch_f32 = batch*d1*d2*d3,
 * partials_f64 = 4*batch*partial_slots doubles with partial_slots >= max(d1, ceil(d1*d2 / max(1, 4096/d3))): the plane routes keep one
 * white-noise slot per plane of the outer axis (d1 of them; a Mixed unit given fewer is SKR_ERR_UNSUPPORTED, a power-of-two one
 * SKR_ERR_SHAPE), the route of separate passes one per workgroup of its last-axis pass (at most the second term).  The coloured
 * statistics and the bookkeeping of the 128 x 128 inverse share the same 4*batch*partial_slots doubles; nothing is written behind them.
 * That minimum guarantees that the draw is accepted, not its fastest route: a 2- or 4-channel unit over planes too large for the LDS takes
 * the fused mid-axes kernel only when its tiles of the half spectrum, ceil((d3/2+1) / 4) at most, fit the slots the white noise leaves
 * free, 2*partial_slots minus the workgroups of the last-axis pass (2 channels over 256 x 256: 33 <= 2*partial_slots - 16, i.e. 25 slots);
 * with fewer the separate passes run, with the same values to rounding.  The Python side passes max(256, ...) slots. */
int skr_noise_colored(void* out, int32_t out_dtype, void* spec_c64, float* scratch_f32, double* partials_f64,
                      int64_t partial_slots, const uint64_t* seeds_dev, uint64_t stream_id, int64_t batch,
                      int32_t d1, int32_t d2, int32_t d3, double exponent, int32_t has_energy, double energy,
                      void* stream);

/* Same generator for per-sample shapes that are not powers of two (rank 1-12 after dropping size-1 dims, any
 * sizes >= 2): identical pipeline; the real N-D transform of the inner (up to three) axes runs on the library's own
 * any-length kernels (skr_fft_own.hip): lengths 2^a r with r a product of at most three factors out of 3, 5, 7, 11, 13 directly
 * (up to 4096), every other length <= 2048 through Bluestein's chirp-z on the same LDS tile transform (its per-length tables are
 * allocated on first use, outside stream capture: SKR_ERR_CAPTURE), and a LAST axis of any even length n = 2 A B with A, B such
 * lengths (8192, 65536, 5000, 10010 ...) as a half-length complex transform in four steps over the same kernels.
 * hipFFT (dlopen'ed on first use) runs only when asked for (skr_set_tuning "hipfft" 1 / SKR_FFT_HIPFFT): a shape outside the above
 * is SKR_ERR_UNSUPPORTED otherwise.  More than three axes (e.g. channels x frames x height x width): every outer axis
 * (<= 128 long, at most nine of them) is a direct DFT kernel, the outermost one fused with the radial weights.
 * Workspaces: spec_c64 = batch*prod(dims[:-1])*(dims[-1]/2+1) complex64, scratch_f32 = batch*prod(dims), partials_f64 = 4*batch*256 doubles. */
int skr_noise_colored_any(void* out, int32_t out_dtype, void* spec_c64, float* scratch_f32, double* partials_f64,
                          const uint64_t* seeds_dev, uint64_t stream_id, int64_t batch, int32_t rank,
                          const int32_t* dims, double exponent, int32_t has_energy, double energy, void* stream);

/* mean(|a - b|^power), power 1 or 2 (FunctionalAdaptive.mae / .mse, skrample/sampling/functional.py:197-214);
 * a may be NULL (= zeros).  Deterministic two-stage reduction in double; the result lands in out_dev[0]
 * (the adaptive sampler reads it back: step-size control is a host decision).  partials_dev: 1024 doubles. */
int skr_error_mean(const void* a_or_null, const void* b, int32_t dtype, int64_t numel, int32_t power,
                   double* out_dev, double* partials_dev, void* stream);

/* raw generator outputs, for parity tests of the RNG itself */
int skr_philox_u32(uint32_t* out /* [n_blocks*4] device */, uint64_t seed, uint64_t stream_id,
                   uint64_t first_block, int64_t n_blocks, void* stream);
/* The Philox-to-normal transform on caller-provided words, one block of four words per thread.  parts = 0:
 * out[4i..4i+3] = the four normals the generators and step kernels make of words[4i..4i+3].  parts = 1: the factors of
 * the first pair, out[4i..] = (r(x), cos(y), sin(y), r(x) * cos(y)) with r = sqrt(-2 ln u), the angle 2 pi u and
 * u = fl32(x) * 2^-32 + 2^-33; words z and w are ignored.  Any other parts is SKR_ERR_UNSUPPORTED. */
int skr_normal_u32(float* out /* [n_blocks*4] device */, const uint32_t* words /* [n_blocks*4] device */,
                   int64_t n_blocks, int32_t parts, void* stream);

/* Colored.colorize_noise (noise.py:337-403) on a caller's white noise: white_f32 ([batch * prod(dims)] fp32, used as
 * the transform workspace and overwritten) is shaped exactly as skr_noise_colored_any shapes its own draws; same
 * workspaces and the same dims: the own any-length transforms, never the plane kernels; hipFFT only when asked for, a shape outside
 * the own transforms' lengths is SKR_ERR_UNSUPPORTED otherwise, refused before anything is written (white_f32 keeps the caller's
 * values).  exponent = 0 is the caller's fast path (plain rescale), not handled here. */
int skr_colorize(void* out, int32_t out_dtype, void* spec_c64, float* white_f32, double* partials_f64, int64_t batch,
                 int32_t rank, const int32_t* dims, double exponent, int32_t has_energy, double energy, void* stream);

/* SPC's signed-power blend (structured.py:568-572 with common.py:187-190), the one non-linear tensor op of the
 * samplers: out = spowf(p * spowf(a, P) + c * spowf(b, P), 1/P), spowf(x, f) = |x|^f * sign(x).  out is fp32 or
 * fp64 (the wrappers' compute_scale; fp64 uses double-precision pow); a and b may be any of the four dtypes.  P != 0. */
int skr_power_blend(void* out, int32_t out_dtype, const void* a, int32_t a_dtype, const void* b, int32_t b_dtype, double p,
                    double c, double power, int64_t numel, void* stream);

/* Backward of skr_power_blend: with u = p * spowf(a, P) + c * spowf(b, P) and g the incoming gradient (out_dtype of the forward,
 * fp32 or fp64, which is also the arithmetic),
 *     grad_a = g * p * |u|^(1/P - 1) * |a|^(P - 1),   grad_b likewise with c and b
 * evaluated as torch autograd evaluates the host expression spowf(x, f) = |x|^f * sign(x) -- the chain
 * ((g * sgn u) * (1/P) |u|^(1/P-1)) * sgn u, then (p * that * sgn a) * P |a|^(P-1) * sgn a, sgn(0) = 0 -- so that exact zeros give
 * what it gives (0, or NaN where a zero meets a negative exponent).  grad_a has a's dtype, grad_b b's; either may be NULL.
 * A 16-bit gradient is the arithmetic's value rounded once to nearest-even, from fp64 arithmetic too. */
int skr_power_blend_backward(void* grad_a, void* grad_b, const void* g, int32_t g_dtype, const void* a, int32_t a_dtype, const void* b,
                             int32_t b_dtype, double p, double c, double power, int64_t numel, void* stream);

/* Diagnostics counters of this process (tests assert that a shape did NOT go to the vendor FFT): "hipfft_plans" = hipFFT plan pairs
 * created so far, "hipfft_execs" = forward hipFFT transforms run so far, "own_fft_execs" = forward N-D transforms run by the library's
 * own any-length kernels so far, "colored_inv128_launches" = launches of the persistent 128 x 128 inverse kernel of Colored noise so far,
 * "colored_inv128_ticketed" = those of its launches in which at least one plane was claimed from the device ticket (more than two planes
 * per block, ticket not disabled), "channels_last_one_trip" / "channels_last_general" = launches of skr_step_launch_channels_last
 * (program launches included) that ran its one-trip / its general kernel so far, "masked_channels_last_one_trip" /
 * "masked_channels_last_general" = the same for skr_step_launch_masked_channels_last; -1 for an unknown key. */
int64_t skr_stat(const char* key);

int skr_abi_version(void);
const char* skr_strerror(int status);
int skr_last_hip_error(void); /* hipError_t of the most recent failed launch on this thread */
const char* skr_build_info(void);

/* Kernel-selection switches for tests and tuning tools (process-wide, not synchronised with launches in flight on
 * other threads; results are bit-identical under every setting -- only speed changes):
 *   "one_trip" 1|0  one-trip loads-first kernels for launches made of whole 2048-element chunks (default 1)
 *   "xmap"     n    XCD-aware chunk map of the one-trip kernels: every XCD takes runs of 2^n consecutive chunks
 *                   (0 = identity map)
 *   "tile"     1|0  whole-line tile layout when a 32-bit tensor takes part (default 1)
 *   "two_out"  2|1|0  compile-time one-trip kernel for two-output (UniPC / SPC) launches: 1 where it measured faster
 *                   (default), 2 wherever it is instantiated, 0 never
 *   "pace"     1|0  paced load issue in the one-trip kernels (default 1)
 *   "two_nt"   -1|0|1  stores of two-output launches without in-kernel noise and >= 9 operands: non-temporal (1), write-through (0),
 *                   by operand count where it measured faster (-1, the default)
 *   "rk_uv"    0|1|2|4  vectors per lane of the grid-stride Runge-Kutta stage kernel (0 = default)
 *   "rk_blk"   0|128|256  threads per workgroup of the one-trip Runge-Kutta stage kernel (0 = by operand count, the default:
 *                   128 for 4-6 operands, 256 otherwise)
 *   "tape_words" 0|1|2  skr_tape_launch: 16-byte words a lane carries per trip (0 = by tensor size, the default: two from 2 Mi elements up)
 *   "fft_rank" 0|1|2  skr_noise_colored_any / skr_colorize: trailing axes handed to the N-D transform (0 = up to three, the
 *                   default); the other axes run on the direct-DFT kernels (results agree to rounding, not bit for bit)
 *   "hipfft"   -1|0|1  the N-D transform of those axes: 0 the library's own kernels (skr_noise_colored_any's comment lists the lengths;
 *                   anything else is SKR_ERR_UNSUPPORTED), 1 hipFFT (dlopen'ed; any length), -1 = by the environment, the default: own
 *                   kernels unless SKR_FFT_HIPFFT is set
 *   "reset"    (value ignored) back to the defaults
 * Initial values can also be set by the environment: SKR_ONE_TRIP=0, SKR_XMAP=n, SKR_NO_TILE, SKR_NO_TWO_OUT, SKR_RK_UV=n, SKR_RK_BLK=n, SKR_TAPE_WORDS=n. */
int skr_set_tuning(const char* key, int32_t value);

#ifdef __cplusplus
}
#endif
#endif /* SKRAMPLE_HIP_H */
