"""Rolling batches (continuous batching): every sample of a batch at its own position of its own sampling loop, one launch per tick.

`capture_sampling_loop(..., per_sample=True)` gives every sample of a batch its own schedule, but all samples start together, run
the same number of steps and finish together.  A server's requests do not: they arrive one by one, and 20-step requests sit
beside 50-step ones.  `RollingBatch` keeps `capacity` slots; a request is admitted into a free slot at any tick, steps with
whatever else is resident, and leaves when its own run is over -- the slot is free for the next request at once:

    batch = RollingBatch(make_wrapper, example, capacity=B)
    batch.admit(slot, latents, wrapper, steps, seed=None)
    t = batch.timesteps                              # device tensor [B]
    done = batch.step(model(batch.latents, t))       # ONE skr_step_launch_rolling; the slots that just finished
    x = batch.take(slot)

In-painting requests (`SkrampleWrapperScheduler.set_inpaint`) join a batch built with the shape of one sample's mask; plain requests
share it, and a tick is still one launch (`skr_step_launch_masked_rolling`, csrc/skr_step_masked.hip):

    batch = RollingBatch(make_wrapper, example, capacity=B, inpaint_mask_shape=(1, H, W))
    batch.admit(slot, latents, wrapper, steps, seed=None, inpaint=(mask, original_samples, noise))   # one sample each
    batch.admit(other, latents, wrapper, steps)      # a plain request: its slot of `batch.mask` is ones

Classifier-free guidance: a batch built with `guided=True` takes the two halves of the network output and forms every request's guided
prediction inside the tick's one launch (`skr_step_launch_guided_rolling`, csrc/skr_step_guided.hip), each request under its own
scale -- or its own guidance schedule, one scale per step:

    batch = RollingBatch(make_wrapper, example, capacity=B, guided=True)
    batch.admit(slot, latents, wrapper, steps, seed=None, guidance_scale=7.5)          # or guidance_scale=[g_0, ..., g_{steps-1}]
    uncond, cond = model(batch.latents, batch.timesteps)                                # two contiguous [B, ...] tensors
    done = batch.step_guided(uncond, cond)

With `device_positions=True` the positions live on the device and a tick needs no host-to-device copy:

    batch.advance()                                  # ONE skr_rolling_advance: index and timesteps computed on the device
    done = batch.step(model(batch.latents, batch.timesteps))
    ticks = batch.capture(model)                     # or: the advance and the network of every ring phase in captured graphs
    done = ticks.tick()                              # one graph replay + one skr_step_launch_rolling

How it works.  The launch structure is the sampler's steady-state (widest) step, found by a dry run of `make_wrapper()` on one
sample.  Every operand of it has a ROLE (sampling/program.py: this tick's sample / model output, or the k-th last sample, model
output or state): the batch binds the roles to whole-batch tensors it rotates itself -- a ring of its own latents, a ring of the
caller's last model outputs, a ring of fp32 states (UniPC / SPC).  An admitted request's rows come from a dry run of ITS wrapper on
one sample (the mechanism of `CapturedLoop.retarget`); each row is placed into the wide structure by role, zeros elsewhere, and
uploaded into the slot's region of one device table.  Per tick the host publishes `index[b] = base[b] + position[b]`, or -1 for a
free or finished slot, with one small stream-ordered copy.  The kernels (csrc/skr_step_fast.hip, `RowForm::Rolling`) skip inactive samples
before their first vector-memory instruction, and neither load nor accumulate an operand whose coefficients are zero in the
sample's row: a sample in its multistep ramp-up has the bits of the narrower launch its lone run makes, whatever the slot's previous
occupant left in the history rings.

A masked batch (`inpaint_mask_shape`) owns three more whole-batch tensors -- `mask[capacity, *mask_shape]` (ones until a request brings
its own), `original` and `noise[capacity, *unit_shape]` -- and two more roles, ("orig",) and ("znoise",), bound to the last two.  Its
launch structure is the widest step of a dry run with in-painting set on scratch one-sample tensors, so both have slots; the launch is
always per slot (`batch_stride = mask_numel`), its mask descriptor built once.  `admit(..., inpaint=...)` copies the request's three
tensors into the slot's slices and dry-runs the wrapper with `set_inpaint` on one-sample views of them (the `retarget` mechanism): the
rows carry the step form in `coef0` and the re-noised known form in `coef1`; the last step's known form is the original alone, a row with
a zero in the `znoise` slot, which the kernel then does not load.  A plain request's rows come from the plain dry run -- every `coef1`
zero, `orig` / `znoise` absent -- under a mask of ones.  `step()`, `advance()`, `capture()` and `CapturedTicks.tick()` mean what they
mean on a plain batch.  Covered there: the samplers whose masked step is one single-output launch -- Euler, DPM 1-3, Adams 2-4, UniP
2-3.  UniPC and SPC blend with a second launch and are refused when the batch is built ("not one fused launch").

Structured noise.  A batch whose `make_wrapper()` has `noise_type` Offset or Pyramid (pytorch/noise.py) and a sampler that draws is
a structured-noise batch: the noise is a whole-batch TENSOR the batch owns, `[capacity, *unit_shape]` in the latents' dtype, and an
operand of the step like any other -- role ("n",) for this tick's draw and ("pn", k) for the draw of -k ticks ago (UniPC's corrector
re-evaluates the previous step with the previous draw), its coefficient in `coef0` / `coef1`; the plan's `noise_mode` is 0 and the step
launch gets no seeds.  A tick draws with ONE call of the generator's rolling entry (`skr_noise_offset_rolling` /
`skr_noise_pyramid_rolling`, csrc/skr_noise.hip) after the index is on the device and before the step launch: the kernels read the same
index vector, draw slot b at draw number `index[b] - b * max_steps` -- its position in its own run, the wrappers draw exactly once per
step -- with the streams its lone generator would use, and leave inactive slots alone.  Where a ("pn", k) occurs the noise tensors form a
ring as long as the latents ring (so that the phases of `CapturedTicks` close); the generator's workspaces for `capacity` samples are
allocated once, when the batch is built.  A new request never reads its slot's previous occupant's noise: its first row has zeros in
every ("pn", k) slot.  `admit()` refuses a wrapper whose `noise_props` differ from the batch's (strength, depth, dims and static are
launch arguments).  Refused when the batch is built: Colored, Brownian and custom generator classes, `prefetch_noise=True`, a unit
the rolling entry does not cover (asked of the library's route decision, nothing launched), and `inpaint_mask_shape` beside
structured noise.

Guided batches (`guided=True`).  The launch structure comes from a dry run through `wrapper.step_guided(u, c, 1.0, t, x)`: `uncond` is the
operand of role ("o",), whose place in the wide structure is the launch's `slot` -- fixed for the batch, checked against every request's
dry run --; `cond` and `guided_out` are launch arguments, not operands.  The history operands ("po", k) are the GUIDED predictions of
earlier ticks, which only the launch itself produces: the batch owns a ring of them, oldest first and as long as the latents ring (so
that the phases of `CapturedTicks` close); a tick's launch stores its prediction into the entry no operand reads.  Nothing of the caller
is held -- no alias guard, no snapshot (`alias_history` has no effect), `uncond` and `cond` may be overwritten once `step_guided` has
returned --, and a sampler without history (Euler) passes `guided_out = NULL` and owns no ring.  The scale of a request's step i is the
row's `convert_k[0]` (a guided plan has no rounded conversion, so the field is free): `admit(..., guidance_scale=g)` takes a float or a
sequence of exactly `steps` floats, requires it on a guided batch and refuses it on any other.  Rows are placed by role as ever, so the
first rows of a run have zeros in the history slots and a new request never reads its slot's previous occupant's predictions; an absent
operand of the guided kernel is one whose `coef0` is zero (`uncond` and `cond` are always read for an active slot).  An unguided request
shares the batch without a special case: hand it the same prediction in both halves -- cond - uncond is exactly 0 and the guided
prediction is `uncond` for finite values, whatever its scale.  `step()` on a guided batch and `step_guided()` on any other raise.
`advance()` and `device_positions=True` work unchanged; `capture(model)` takes a model that returns `(uncond, cond)`, and
`CapturedTicks.tick()` is one replay plus one eager guided launch whose operand array, `cond` and `guided_out` were bound per phase at
capture time.  Covered: Euler, DPM 1-3, Adams 2-4 and UniP 2-3, with or without stochasticity, `Random` noise or none, bf16 / fp16 / fp32
latents under the default compute scale.  Refused when the batch is built, each with its reason: a sampler whose guided step is not one
fused launch (UniPC, SPC, `compute_scale=None`), `guided` beside `inpaint_mask_shape`, `guided` beside Offset / Pyramid noise, and
whatever the one-trip guided kernel does not cover.  Not covered: changing a resident request's scale mid-run (admit it with a schedule),
channels-last, the Runge-Kutta wrappers, autograd.

Rescaled guidance (`guided=True, rescaled=True`): diffusers' `rescale_noise_cfg` with a `guidance_rescale` (phi) per request, or per step:

    batch = RollingBatch(make_wrapper, example, capacity=B, guided=True, rescaled=True)
    batch.admit(slot, latents, wrapper, steps, guidance_scale=7.5, guidance_rescale=0.7)   # or one phi per step; 0.0 (the default): not rescaled
    done = batch.step_guided(uncond, cond)

phi travels in the row's `convert_k[1]` beside the scale in `convert_k[0]` (zero in every other batch's rows).  A tick is two launches on
the current stream with the same index, rows and row offset: `skr_guidance_rescale_factor_rolling` (csrc/skr_guidance_stats_rows.hip)
writes std(cond) / std(prediction) of every active slot whose phi is not zero into the batch's `factor` tensor, `[capacity]` in the latents'
dtype, through a partial-sum workspace -- both allocated once, when the batch is built, the same in every phase of `CapturedTicks` --; then
`skr_step_launch_guided_rescaled_rolling` (csrc/skr_step_guided.hip) steps every active slot, with the rescaled prediction
where phi is not zero and with the plain guided one -- its factor unread -- where it is.  Free slots, finished slots and requests that do
not rescale cost no statistics traffic; the tick has the same two launches whether or not a resident request rescales.  Every request has
the bits of its lone `step_guided(uncond, cond, g, t, x, guidance_rescale=phi)` run, and a request with phi = 0 throughout those of a
guided batch built without `rescaled`.  Ring upkeep, `guided_out` (NULL for Euler), the returned slots, "nothing of the caller is held",
`advance()`, `device_positions=True`, `capture(model)` (`CapturedTicks.tick()`: one replay plus the two eager launches) and the refusals
of a guided batch are unchanged.  `rescaled=True` without `guided=True`, a negative, NaN or non-number `guidance_rescale`, a schedule of
the wrong length and a non-zero `guidance_rescale` on a batch built without `rescaled` are refused.  Not covered: changing a resident
request's phi mid-run (admit it with a schedule), skipping the statistics launch from the host when nobody rescales.

Sample sizes.  A unit (`example.shape[1:]`) of whole 2048-element chunks joins any batch.  A ragged unit -- at least 2048 elements and a
multiple of 8, not whole chunks: (4,144,112) and most other non-square SDXL latent buckets -- joins a plain batch: not `guided`, no
`inpaint_mask_shape`, `Random` noise or none, and a sampler whose step is one single-output launch (Euler, DPM 1-3, Adams, UniP).  The
entry takes the ragged form of the kernel by itself (csrc/skr_step_ragged.hip: a sample's last workgroup is partly empty), and `admit()`,
`step()`, `advance()`, `capture()` and `CapturedTicks.tick()` need nothing new.  Refused when the batch is built, each naming the reason:
UniPC and SPC, `guided`, `inpaint_mask_shape` and Offset / Pyramid noise on a ragged unit; units below 2048 elements or not a multiple of 8.

Covered: `SkrampleWrapperScheduler` with Euler, DPM 1-3, Adams 2-4, UniP / UniPC 2-3 and SPC, with or without stochasticity,
`Random` noise (drawn in the kernel), `Offset` / `Pyramid` noise (drawn per slot, above) or none, bf16 / fp16 / fp32 latents under the default compute scale -- what
`skr_step_launch_indexed` covers (UniPC on fp32 latents is refused, as by the captured loops); a device-resident position vector
(`device_positions=True`: csrc/skr_rolling.hip advances positions the host validated once at `admit()`, so the index the step
kernel reads is inside the slot's own run by construction) and graph capture of ticks (`capture()`: one graph per ring phase holds
the advance and the network; the step launch follows each replay eagerly, which is what lets the graphs' static outputs be the
model-output history, aliased and never copied).  Not covered: the Runge-Kutta wrapper classes (the kernel form exists, the stage
bookkeeping does not), Colored and Brownian noise (Colored's persistent plane kernels claim planes by ticket, Brownian's weights are a host
walk per step interval), Pyramid units of the any-shape / nd routes and Offset units outside the aligned kernel, structured noise in
masked batches, the draw inside the captured graph, autograd, runs longer than `max_steps`, the step launch inside the graph (its history
operands are the other graphs' outputs, which exist only once every graph is captured: it would force a snapshot of every model output).
"""

from __future__ import annotations

import ctypes
from typing import Callable, Sequence

import torch

from . import _hip
from ._hip import PER_SAMPLE_CHUNK, ROW_TERMS, SkrampleHipError, StepGuidanceC, StepMaskC, StepPlanC, StepRescaleC, StepRowC, upload_rows
from .sampling import lazy

Role = tuple  # ("x",) ("o",) ("pi", k) ("po", k) ("px", k), k < 0: see sampling/program.py; ("orig",) ("znoise",): a masked batch's original / re-noising tensor;
# ("n",) ("pn", k): a structured-noise batch's draw of this tick / of -k ticks ago

ALIAS_HELP = (
    "a model output passed to an earlier step() is still a history operand of this batch and {what}; RollingBatch aliases the caller's "
    "model outputs instead of copying them -- construct it with alias_history=False (one snapshot per tick) when the network reuses its output buffer"
)


def sampler_structure(wrapper) -> tuple:
    "what two requests must share to step in one launch (host only: read from the wrapper's configuration)"
    sampler = wrapper.sampler
    nested = tuple((type(s).__name__, getattr(s, "order", None)) for s in (getattr(sampler, "predictor", None), getattr(sampler, "corrector", None)) if s is not None)
    return (type(wrapper).__name__, type(sampler).__name__, getattr(sampler, "order", None), nested, type(wrapper.model).__name__,
            wrapper.compute_scale, getattr(wrapper.noise_type, "__name__", None), bool(wrapper.invert_prediction))  # fmt: skip


def place_row(wide_roles: Sequence[Role], plan: StepPlanC, roles: Sequence[Role], two_outputs: bool) -> StepRowC:
    """The row of a (possibly narrower) launch inside the wide structure: operand j goes to the slot of its role, the other slots
    stay zero -- absent operands for the kernel.  The operands present must keep their relative order (the kernels accumulate in
    slot order; any other order would not be the lone run's bits).  A single-output launch inside a two-output structure (the
    first step of a UniPC / SPC run) goes to the second output, the one that is the step's result: the state it leaves is zero
    and is never read, because the next step's row has a zero there."""
    row = StepRowC()
    last = -1
    single = two_outputs and plan.out1_dtype == _hip.NONE
    for j, role in enumerate(roles):
        if role not in wide_roles:
            raise SkrampleHipError(f"operand {role} of this step has no place in the batch's launch structure {list(wide_roles)}")
        behind = [at for at, wide in enumerate(wide_roles) if wide == role and at > last]  # (a role may have several slots: see RollingBatch._widest)
        if not behind:
            raise SkrampleHipError(f"operand {role} precedes its neighbours in this step but follows them in the batch's launch structure: the sums would differ in order")
        last = at = behind[0]
        if single:
            row.coef1[at] = plan.coef0[j]
        else:
            row.coef0[at], row.coef1[at] = plan.coef0[j], plan.coef1[j]
    if single:
        row.zeta1, row.stream1 = plan.zeta0, plan.stream0
    else:
        row.chain, row.zeta0, row.zeta1, row.stream0, row.stream1 = plan.chain, plan.zeta0, plan.zeta1, plan.stream0, plan.stream1
    return row


def advance_reference(position: list, length: list, times: list, max_steps: int) -> tuple[list, list, list]:
    """What `skr_rolling_advance` computes, in plain Python: (new position, sample index, timestep or None) per slot.  A slot is active
    iff 0 <= p < n <= max_steps; an inactive slot reads -1 and keeps its position and its timestep (None: the bytes stay)."""
    new_position, index, timestep = list(position), [], []
    for b, (p, n) in enumerate(zip(position, length)):
        if 0 <= p < n <= max_steps:
            index.append(b * max_steps + p)
            timestep.append(times[b * max_steps + p])
            new_position[b] = p + 1
        else:
            index.append(-1)
            timestep.append(None)
    return new_position, index, timestep


def draw_reference(index: list, max_steps: int, static: bool, stride: int = 256) -> list:
    """What the rolling generator entries derive from the index vector, in plain Python: per slot None (inactive: nothing drawn, nothing
    read) or (stream_base, auxiliary stream) -- the auxiliary stream is `stream_levels` of Pyramid; Offset's `stream_offset` is one more."""
    out = []
    for b, at in enumerate(index):
        if at < 0:
            out.append(None)
            continue
        base = (at - b * max_steps) * stride
        out.append((base, 0 if static else base))
    return out


class _Request:
    __slots__ = ("rows", "times", "position")

    def __init__(self, rows: list, times: list):
        self.rows, self.times, self.position = rows, times, 0


class RollingBatch:
    """`capacity` slots of samples shaped like `example[0]`, stepped together by one `skr_step_launch_rolling` per tick.

    `make_wrapper()` returns a fresh `SkrampleWrapperScheduler`: its sampler fixes the launch structure every admitted request must
    share.  `max_steps` bounds a request's run length (the device table holds `capacity * max_steps` rows of 328 bytes).
    `alias_history`: True keeps the caller's model outputs as history operands (0 bytes written; overwriting one that is still
    held raises), False snapshots each one.  `device_positions`: True keeps every slot's position, run length and timesteps on
    the device (`advance()` before each `step()`, or `capture()`); the host publishes nothing per tick.  `guided`: True makes a tick
    `step_guided(uncond, cond)`, one `skr_step_launch_guided_rolling` with every request's own guidance scale (module docstring).
    `rescaled` (with `guided`): True makes that tick two launches -- `skr_guidance_rescale_factor_rolling`, then
    `skr_step_launch_guided_rescaled_rolling` -- with every request's own `guidance_rescale` beside its scale (module docstring)."""

    def __init__(self, make_wrapper: Callable[[], object], example: torch.Tensor, capacity: int, max_steps: int = 128, alias_history: bool = True,
                 device_positions: bool = False, inpaint_mask_shape: Sequence[int] | None = None, guided: bool = False, rescaled: bool = False):  # fmt: skip
        if capacity < 1:
            raise ValueError("a rolling batch has at least one slot")
        self.masked = inpaint_mask_shape is not None
        self.guided = bool(guided)
        self.rescaled = bool(rescaled)
        if self.rescaled and not self.guided:
            raise ValueError("rescaled=True needs guided=True: guidance_rescale is applied to the guided prediction a guided batch forms")
        if self.guided and self.masked:
            raise ValueError("guided together with inpaint_mask_shape: a guided step under set_inpaint is not one fused launch (guided in-painting batches are not covered)")
        self.capacity, self.max_steps, self.alias_history = int(capacity), int(max_steps), bool(alias_history)
        self.device_positions = bool(device_positions)
        if self.device_positions and (self.max_steps < 1 or self.capacity * self.max_steps > 0x7FFFFFFF):
            raise ValueError(f"device-resident positions index {self.capacity} x {self.max_steps} rows with an int32")
        self.unit_shape = tuple(example.shape[1:])
        self.dtype, self.device = example.dtype, example.device
        self.sample_numel = 1
        for n in self.unit_shape:
            self.sample_numel *= int(n)
        # ragged samples (at least one chunk, a multiple of 8 elements, not whole chunks: most non-square SDXL buckets) join a plain batch
        self.ragged = _hip.ragged_sample(self.sample_numel)
        if self.sample_numel <= 0 or (self.sample_numel % PER_SAMPLE_CHUNK != 0 and not self.ragged):
            raise ValueError(f"per-sample rows need samples of whole {PER_SAMPLE_CHUNK}-element chunks, not {self.sample_numel} elements per sample "
                             f"(ragged samples are served from {PER_SAMPLE_CHUNK} elements on, in multiples of 8)")
        self.numel = self.capacity * self.sample_numel
        first = make_wrapper()
        if self.ragged:
            self._refuse_ragged(first)
        if self.guided:
            self._refuse_guided(first)
        self.draws_noise = bool(first.sampler.require_noise)
        self.structured = self.draws_noise and self._init_noise(first)
        if self.masked:
            self._init_inpaint(tuple(int(n) for n in inpaint_mask_shape), first)
        self.structure = sampler_structure(first)
        self.keep = int(first.sampler.require_previous)
        self.plan, self.roles = self._widest(self._trace(first, self.keep + 4, seed=0 if self.draws_noise else None))
        self.two_outputs = self.plan.out0_dtype != _hip.NONE and self.plan.out1_dtype != _hip.NONE
        if self.ragged and not _hip.single_output_plan(self.plan):  # (whatever else the dry run turned up: compute_scale=float64, a rounded conversion)
            raise SkrampleHipError(f"skr_step_launch_rolling: request outside kernel coverage ({_hip.RAGGED_SINGLE_OUTPUT})")
        if self.plan.n_terms > ROW_TERMS:
            raise SkrampleHipError(f"a launch with {self.plan.n_terms} operands does not fit a device-resident row ({ROW_TERMS})")
        shape = (self.capacity, *self.unit_shape)
        depth = self.keep + 1
        # rings, oldest first: [-1] is this tick's latents / the latest state; the model outputs are the caller's (or snapshots)
        self._x = [torch.zeros(shape, dtype=self.dtype, device=self.device) for _ in range(depth + 1)]
        state_dtype = _hip.CODE_DTYPE[self.plan.out0_dtype] if self.two_outputs else None
        self._state = [torch.zeros(shape, dtype=state_dtype, device=self.device) for _ in range(depth + 1)] if self.two_outputs else []
        self._blank = torch.zeros(shape, dtype=self.dtype, device=self.device)  # stands for a model output no tick has produced yet
        if self.structured:
            # the noise tensors, oldest first: [-1] is the latest draw; a ring as long as the latents ring where a step reads an earlier draw
            self._n = [torch.zeros(shape, dtype=self.dtype, device=self.device) for _ in range(depth + 1 if any(r[0] == "pn" for r in self.roles) else 1)]
            self._noise_ws = self.noise_type.rolling_workspace(self.unit_shape, self.noise_props, self.capacity, self.device)
        # a guided batch: the guided predictions of the last ticks, oldest first, as long as the latents ring (so that the phases of
        # CapturedTicks close); [-1] is the tensor this tick's launch stores into, ("po", k) the one of -k ticks ago.  Euler keeps none.
        self._g = [torch.zeros(shape, dtype=self.dtype, device=self.device) for _ in range(depth + 1)] if self.guided and self.keep else []
        if self.rescaled:
            # a rescaled batch: every slot's factor std(cond) / std(p) and the partial sums behind it, written by the tick's statistics
            # launch and read by its step launch; allocated once, the same in every phase of CapturedTicks
            self.factor = torch.zeros(self.capacity, dtype=self.dtype, device=self.device)
            self._partials = torch.zeros(_hip.guidance_partials(self.numel, self.sample_numel), dtype=torch.float64, device=self.device)
            self._rescale_desc = StepRescaleC(self.factor.data_ptr(), 0.0, self.sample_numel, 0)
        self._outputs: list[torch.Tensor] = []
        self._stamps: list[tuple[torch.Tensor, int, int]] = []
        self._results: dict[int, torch.Tensor] = {}
        self._requests: list[_Request | None] = [None] * self.capacity
        self._finished: set[int] = set()
        self.row_bytes = ctypes.sizeof(StepRowC)
        self.rows_dev = torch.zeros(self.capacity * self.max_steps * self.row_bytes, dtype=torch.uint8, device=self.device)
        self.index_dev = torch.full((self.capacity,), -1, dtype=torch.int32, device=self.device)
        self.seeds_dev = torch.zeros(self.capacity, dtype=torch.int64, device=self.device)
        self._times_host = torch.zeros(self.capacity, dtype=torch.float32)
        self.timesteps = torch.zeros(self.capacity, dtype=torch.float32, device=self.device)
        self.ticks = 0
        self._advanced = False  # device positions: advance() ran and step() has not consumed it yet
        self._captured: "CapturedTicks | None" = None
        if self.device_positions:
            self.position_dev = torch.zeros(self.capacity, dtype=torch.int32, device=self.device)
            self.length_dev = torch.zeros(self.capacity, dtype=torch.int32, device=self.device)
            self.times_dev = torch.zeros(self.capacity * self.max_steps, dtype=torch.float32, device=self.device)
        self._fixed = self._fixed_arguments()

    def _init_noise(self, first) -> bool:
        "a wrapper whose sampler draws: False for `Random` (drawn in the step kernel), True for a generator the batch draws per slot, or the refusal"
        from .pytorch import noise as generators

        kind = first.noise_type
        if kind is generators.Random:
            return False
        defaults = {generators.Offset: generators.OffsetProps(), generators.Pyramid: generators.PyramidProps()}
        if kind not in defaults:
            why = {generators.Colored: "its persistent plane kernels claim planes by ticket and have no per-slot form",
                   generators.Brownian: "its weights are a host walk per step interval"}.get(kind, "a custom generator class has no per-slot kernel form")  # fmt: skip
            raise SkrampleHipError(f"{getattr(kind, '__name__', kind)} noise cannot join a rolling batch ({why}): a rolling batch draws Random, Offset or Pyramid noise")
        if self.masked:
            raise ValueError(f"inpaint_mask_shape together with {kind.__name__} noise: a masked rolling batch draws Random noise or none")
        if getattr(first, "prefetch_noise", False):
            raise ValueError("prefetch_noise=True draws a step's noise ahead on a side stream of the wrapper: a rolling batch draws every slot's noise itself, per tick")
        self.noise_type = kind
        self.noise_props = first.noise_props if first.noise_props is not None else defaults[kind]
        refused = kind.rolling_refusal(self.unit_shape, self.noise_props, self.capacity)
        if refused is not None:
            raise SkrampleHipError(f"{kind.__name__} noise on samples {self.unit_shape}: {refused}")
        return True

    def _refuse_ragged(self, first) -> None:
        """ragged samples (not whole 2048-element chunks): only the single-output rolling step has a ragged kernel form
        (csrc/skr_step_ragged.hip); everything else is refused by name before anything is allocated or traced"""
        from .pytorch import noise as generators
        from .sampling import structured as sampling

        what = f"ragged samples ({self.sample_numel} elements, not whole {PER_SAMPLE_CHUNK}-element chunks)"
        if self.guided:
            raise ValueError(f"guided together with {what}: the guided row kernels need samples of whole chunks")
        if self.masked:
            raise ValueError(f"inpaint_mask_shape together with {what}: the masked row kernels need samples of whole chunks")
        sampler = first.sampler
        if type(sampler).sample_packed is not sampling.StatedSampler.sample_packed:
            raise SkrampleHipError(f"{type(sampler).__name__} on {what}: its step is a two-output launch, whose row kernel needs samples of whole chunks; "
                                   "a rolling batch of ragged samples takes Euler, DPM 1-3, Adams and UniP")  # fmt: skip
        if bool(sampler.require_noise) and first.noise_type in (generators.Offset, generators.Pyramid):
            raise ValueError(f"{first.noise_type.__name__} noise on {what}: the rolling draws need samples of whole chunks; a rolling batch of ragged samples draws Random noise or none")

    def _refuse_guided(self, first) -> None:
        "a guided batch: what its one launch per tick does not cover, refused by name before anything is allocated or traced"
        from .pytorch import noise as generators
        from .sampling import structured as sampling

        sampler = first.sampler
        if type(sampler).sample_packed is not sampling.StatedSampler.sample_packed:
            raise SkrampleHipError(f"a guided step of {type(sampler).__name__} is not one fused launch (its two-output step forms the guided prediction with a "
                                   "guidance-only launch of its own): a guided rolling batch takes Euler, DPM 1-3, Adams 2-4 and UniP 2-3")  # fmt: skip
        if first.compute_scale is None:
            raise SkrampleHipError("a guided step under compute_scale=None is not one fused launch (the guidance-only launch, then the reference's rounded tensor ops)")
        if getattr(first, "_inpaint", None) is not None:
            raise SkrampleHipError("a guided step under set_inpaint is not one fused launch: guided in-painting batches are not covered")
        if bool(sampler.require_noise) and first.noise_type in (generators.Offset, generators.Pyramid):
            raise ValueError(f"guided together with {first.noise_type.__name__} noise: a guided rolling batch draws Random noise or none (structured noise is not covered)")
        if self.dtype not in (torch.bfloat16, torch.float16, torch.float32):
            raise SkrampleHipError(f"guided rows need one 16- or 32-bit dtype for operands, cond and both outputs, not {self.dtype}")

    def _init_inpaint(self, mask_shape: tuple, first) -> None:
        """A masked batch: the three whole-batch in-paint tensors (every slot's mask starts as ones: generate everything), the mask
        descriptor of every tick's launch -- one mask per slot, always -- and in-painting set on the wrapper whose dry run gives the
        launch structure, on scratch one-sample tensors, so that `orig` and `znoise` get their slots."""
        unit = (1, *self.unit_shape)
        try:
            self.mask_numel, _ = lazy.mask_layout((1, *mask_shape), unit)
        except SkrampleHipError as refused:
            raise ValueError(f"inpaint_mask_shape {mask_shape} is not the mask of one {self.unit_shape} sample: {refused}") from None
        if self.mask_numel % 8 != 0:
            raise ValueError(f"masked rows need a mask of a multiple of 8 elements per sample, not {self.mask_numel}")
        if self.dtype not in (torch.bfloat16, torch.float16, torch.float32):
            raise ValueError(f"masked rows need one 16- or 32-bit dtype for operands, mask and output, not {self.dtype}")
        self.mask_shape = mask_shape
        self.mask = torch.ones((self.capacity, *mask_shape), dtype=self.dtype, device=self.device)
        self.original = torch.zeros((self.capacity, *self.unit_shape), dtype=self.dtype, device=self.device)
        self.noise = torch.zeros((self.capacity, *self.unit_shape), dtype=self.dtype, device=self.device)
        self._mask_desc = StepMaskC(self.mask.data_ptr(), _hip.DTYPE_CODE[self.dtype], 0, self.mask_numel, self.mask_numel)
        scratch = [torch.ones((1, *mask_shape), dtype=self.dtype, device=self.device)] + [torch.zeros(unit, dtype=self.dtype, device=self.device) for _ in range(2)]
        first.set_inpaint(*scratch)

    # ---- what a test replaces to run the bookkeeping without a device ---------------------------------------------------
    def _trace(self, wrapper, steps: int, seed: int | None) -> list[tuple[StepPlanC, list[Role], float]]:
        """Dry run of `wrapper` for `steps` steps on one sample: (plan, operand roles, timestep) of every step's single launch.
        Coefficients depend on the schedule and the step alone, never on tensor contents, so the model outputs are zeros.
        A wrapper with `set_inpaint` in force (a masked batch's in-painting request) must issue masked launches -- a `_hip.StepCall`
        of kind "masked" -- and one without it plain ones.  A guided batch steps the wrapper with `step_guided(uncond, cond, 1.0, ...)`
        and must see one of kind "guided": `uncond` is the operand of role ("o",) -- the call's `slot` --, `cond` and `guided_out` are
        not operands, and the history operands are the wrapper's stored guided predictions, role ("po", k)."""
        inpaint = getattr(wrapper, "_inpaint", None)
        if inpaint is not None and not self.masked:
            raise SkrampleHipError("this wrapper has set_inpaint in force and the batch was built without inpaint_mask_shape")
        wrapper.set_timesteps(steps)
        x = torch.zeros((1, *self.unit_shape), dtype=self.dtype, device=self.device)
        found = []
        draws = self.structured and bool(wrapper.sampler.require_noise)
        for t in wrapper.timesteps.tolist():
            out = torch.zeros_like(x)
            cond = torch.zeros_like(x) if self.guided else None
            known: dict[int, Role] = {}
            if draws:
                # the step's realised noise: handed to the wrapper in place of a draw of its generator (the wrapper consumes one draw per
                # step either way, and the coefficient of the operand does not depend on its contents)
                wrapper._predrawn_noise = torch.zeros_like(x)
                known[wrapper._predrawn_noise.data_ptr()] = ("n",)
            for k in range(-len(wrapper._previous), 0):
                state = wrapper._previous[k].sample
                if isinstance(state, torch.Tensor):
                    known[state.data_ptr()] = ("px", k)
                if draws and isinstance(wrapper._previous[k].noise, torch.Tensor):
                    known[wrapper._previous[k].noise.data_ptr()] = ("pn", k)
                known[wrapper._raw_outputs[k].data_ptr()] = ("po", k)
                known[wrapper._raw_samples[k].data_ptr()] = ("pi", k)
            held = _hip.trace
            _hip.trace = []
            try:
                if self.guided:
                    new = wrapper.step_guided(out, cond, 1.0, t, x, generator=[seed] if seed is not None else None, return_dict=False)[0]
                else:
                    new = wrapper.step(out, t, x, generator=[seed] if seed is not None else None, return_dict=False)[0]
                launches = _hip.trace
            finally:
                _hip.trace = held
            if len(launches) != 1:
                raise SkrampleHipError(f"a step of this wrapper is {len(launches)} launches, not one fused launch: it cannot join a rolling batch")
            call = launches[0]
            if self.guided and call.kind != "guided":
                raise SkrampleHipError("a guided step of this wrapper is not one fused guided launch: it cannot join a guided rolling batch")
            if (call.kind == "masked") != (inpaint is not None):
                raise SkrampleHipError("a step of this wrapper is not the masked launch its in-painting asks for" if inpaint is not None else "a step of this wrapper is a masked launch although no in-painting is set")
            plan, inputs = StepPlanC.from_buffer_copy(call.plan), call.inputs
            known[x.data_ptr()], known[out.data_ptr()] = ("x",), ("o",)
            if inpaint is not None:
                known[inpaint[1].data_ptr()], known[inpaint[2].data_ptr()] = ("orig",), ("znoise",)
            if wrapper._raw_samples:  # (a wrapper that snapshots its history stepped on its own copies of this call's tensors)
                known[wrapper._raw_samples[-1].data_ptr()], known[wrapper._raw_outputs[-1].data_ptr()] = ("x",), ("o",)
            roles = [known.get(tensor.data_ptr()) for tensor in inputs]
            if any(r is None for r in roles):
                raise SkrampleHipError("a step of this wrapper reads a temporary tensor (a cast, a copy, realised noise): it cannot join a rolling batch")
            if self.guided and (inputs[call.slot] is not out or roles.count(("o",)) != 1):
                raise SkrampleHipError("the guided launch of this wrapper does not replace its `uncond` operand: it cannot join a guided rolling batch")
            found.append((plan, roles, float(t)))
            x = new
        torch.cuda.synchronize(self.device)
        return found

    def _fixed_arguments(self) -> list:
        """Per batch, once: [(C entry name, its arguments laid out by the launch table, name -> position of those a tick fills in)] of the
        tick's launches -- the statistics launch of a rescaled batch, then the step launch.  Everything else in them is the batch's own --
        plan, descriptors, and the addresses of rows_dev, index_dev, seeds_dev, factor and _partials, which are allocated in __init__ and
        never reassigned."""
        kind = "guided_rescaled" if self.rescaled else "guided" if self.guided else "masked" if self.masked else "plain"
        # structured noise is an operand, drawn by a launch of its own: no seeds (masked and guided batches refuse structured noise when built)
        seeds = self.seeds_dev.data_ptr() if self.draws_noise and not self.structured else None
        values = dict(plan=self.plan, seeds=seeds, numel=self.numel, rows=self.rows_dev.data_ptr(), index=self.index_dev.data_ptr(), row_offset=0,
                      operands=None, out0=None, out1=None, stream=None, uncond=None, cond=None, guide=StepGuidanceC())  # fmt: skip
        if self.masked:  # (one output: a masked step is one single-output launch)
            values["mask"] = self._mask_desc
        if self.rescaled:  # (the statistics launch reads the same index, rows and row_offset, and writes the factor the step's descriptor names)
            values.update(rescale=self._rescale_desc, dtype=_hip.DTYPE_CODE[self.dtype], sample_numel=self.sample_numel, factor=self.factor.data_ptr(), stats=None,
                          partials=self._partials.data_ptr())  # fmt: skip
        launches = []
        for each in (_hip.FACTOR, kind) if self.rescaled else (kind,):
            name, names = _hip.ENTRIES[each, "rolling"]
            launches.append((name, _hip.entry_args(each, "rolling", **values), {n: i for i, n in enumerate(names)}))
        return launches

    def _launch(self, arr, out0: torch.Tensor | None, out1: torch.Tensor | None, cond: torch.Tensor | None = None, guided_out: torch.Tensor | None = None) -> None:
        """the tick's step launch through the rolling form of the launch table (_hip.ENTRIES); a rescaled batch: behind the statistics
        launch, on the same stream.  Only what changes from tick to tick is filled in."""
        lib, stream = _hip.load(), _hip.current_stream_ptr(self.device)
        given = {"operands": arr, "out0": _hip._ptr(out0), "out1": _hip._ptr(out1), "stream": stream}
        if self.guided:  # (one output; `cond` and `guided_out` -- None: not stored -- are launch arguments, the scale each slot's row value)
            given["guide"] = ctypes.byref(StepGuidanceC(cond.data_ptr(), _hip._ptr(guided_out), 0.0, self.slot, 0))
            if self.rescaled:  # (what the statistics launch reads)
                given["uncond"], given["cond"] = arr[self.slot], cond.data_ptr()
        for name, fixed, at in self._fixed:
            args = list(fixed)
            for what, value in given.items():
                if what in at:
                    args[at[what]] = value
            _hip.check(getattr(lib, name)(*args), name)

    def _draw(self, out: torch.Tensor) -> None:
        "a structured-noise batch: ONE launch of the generator's rolling entry draws, into `out`, every slot the index on the device names"
        self.noise_type._rolling(out, self._noise_ws, self.seeds_dev, self.index_dev, self.max_steps, self.noise_props)

    def _advance(self) -> None:
        lib = _hip.load()
        status = lib.skr_rolling_advance(self.position_dev.data_ptr(), self.length_dev.data_ptr(), self.times_dev.data_ptr(), self.index_dev.data_ptr(),
                                         self.timesteps.data_ptr(), self.capacity, self.max_steps, _hip.current_stream_ptr(self.device))  # fmt: skip
        _hip.check(status, "skr_rolling_advance")

    # ---- structure ---------------------------------------------------------------------------------------------------------
    def _widest(self, traced) -> tuple[StepPlanC, list[Role]]:
        """The launch structure: the widest step of the dry run.  The kernels accumulate in slot order, so every narrower step's
        operands must appear in it in THEIR order.  Where a ramp-up step orders two roles the other way round (SPC's second step
        reads sample, previous sample, model output; its steady state sample, model output, previous sample, ...) the role gets a
        second slot at the place that step needs it: a slot whose coefficients are zero costs a kernel argument and no bytes.  Two-output
        launches are then padded with never-present slots up to an operand count the table kernels are instantiated for."""
        plan, roles, _ = max(traced, key=lambda entry: entry[0].n_terms)
        wide = StepPlanC.from_buffer_copy(plan)
        roles = list(roles)
        two = wide.out0_dtype != _hip.NONE and wide.out1_dtype != _hip.NONE
        for _, narrow, _ in traced:
            at = 0
            for role in narrow:
                if role[0] == "px":
                    continue  # (the fp32 group stays last)
                found = [i for i in range(at, wide.n_group_a) if roles[i] == role]
                if found:
                    at = found[0] + 1
                else:
                    roles.insert(at, role)
                    wide.n_group_a += 1
                    wide.n_terms += 1
                    at += 1
        if two and wide.n_terms > wide.n_group_a:
            while wide.n_group_a not in (4, 6, 7, 8, 10, 12, 14) and wide.n_group_a < 14:
                roles.insert(wide.n_group_a, ("none",))
                wide.n_group_a += 1
                wide.n_terms += 1
        wide.sample_numel = self.sample_numel
        if self.draws_noise and not self.structured:  # (structured noise is an operand, drawn by a launch of its own)
            wide.noise_mode = 1
        if self.dtype == torch.float32 and wide.out0_dtype != _hip.NONE and wide.out1_dtype != _hip.NONE:
            raise SkrampleHipError("skr_step_launch_rolling: request outside kernel coverage (the two-output table kernels take 16-bit operands)")
        # (the batch's dtype is a 16- or 32-bit one: _init_inpaint and _refuse_guided have seen to it)
        if self.masked and not _hip.one_group_launch(wide, _hip.DTYPE_CODE[self.dtype]):
            raise SkrampleHipError("skr_step_launch_masked_rolling: request outside kernel coverage (one single-output launch of one 16- or 32-bit dtype, evaluated in float32)")
        if self.guided:
            if not _hip.one_group_launch(wide, _hip.DTYPE_CODE[self.dtype]) or wide.convert_to or wide.convert_from:
                raise SkrampleHipError("skr_step_launch_guided_rolling: request outside kernel coverage (one single-output launch of one 16- or 32-bit dtype, evaluated in float32)")
            if roles.count(("o",)) != 1:
                raise SkrampleHipError("the guided launch structure has no single `uncond` operand for the guided value to replace")
            self.slot = roles.index(("o",))
        return wide, list(roles)

    def _rows_of(self, traced, scales: Sequence[float] | None = None, rescales: Sequence[float] | None = None) -> list[StepRowC]:
        """`scales` (a guided batch): the guidance scale of every step, carried in the row's convert_k[0] (a guided plan has no rounded
        conversion); `rescales` (a rescaled batch): guidance_rescale of every step, in convert_k[1] -- zero in every other batch's rows"""
        rows = []
        for step, (plan, roles, _) in enumerate(traced):
            if (plan.dtype_a, plan.acc_f64, plan.convert_to, plan.convert_from) != (self.plan.dtype_a, self.plan.acc_f64, self.plan.convert_to, self.plan.convert_from):
                raise SkrampleHipError("a step of this request differs in dtype or conversion from the batch's launch structure")
            if self.masked and not _hip.one_group_launch(plan):  # (dtype and arithmetic are the batch's by the check above)
                raise SkrampleHipError("a step of this request is not one single-output launch of the masked batch's dtype")
            row = place_row(self.roles, plan, roles, self.two_outputs)
            if self.guided:
                if not _hip.one_group_launch(plan) or list(roles).count(("o",)) != 1:
                    raise SkrampleHipError("a step of this request is not one single-output guided launch of the batch's dtype with one `uncond` operand")
                if row.coef0[self.slot] != plan.coef0[list(roles).index(("o",))]:  # (place_row put `uncond` where the batch's launches replace it)
                    raise SkrampleHipError(f"the `uncond` operand of this step is not at the batch's slot {self.slot}")
                row.convert_k[0] = float(scales[step])
                if self.rescaled and rescales is not None:
                    row.convert_k[1] = float(rescales[step])
            rows.append(row)
        return rows

    # ---- slots ---------------------------------------------------------------------------------------------------------------
    def _check_slot(self, slot: int) -> int:
        if not isinstance(slot, int) or isinstance(slot, bool) or not 0 <= slot < self.capacity:
            raise ValueError(f"slot {slot} outside 0..{self.capacity - 1}")
        return slot

    @property
    def latents(self) -> torch.Tensor:
        "this tick's samples, [capacity, ...]: what the network reads (free slots hold finite leftovers)"
        return self._x[-1]

    @property
    def active(self) -> list[int]:
        return [b for b, r in enumerate(self._requests) if r is not None and b not in self._finished]

    def free(self, slot: int) -> bool:
        return self._requests[self._check_slot(slot)] is None

    def ring_tensors(self) -> list[torch.Tensor]:
        "every whole-batch tensor a history operand may be bound to: the batch's own latents and states, snapshots of model outputs"
        owned = self._x[:-1] + list(self._state) + [self._blank] + (list(self._n) if self.structured else []) + list(self._g)
        return owned + ([] if self.alias_history else list(self._outputs))

    def _running(self) -> list[tuple[int, _Request]]:
        "host: (slot, request) of every active slot, validated -- nothing outside a slot's own run; THE scan every tick starts with"
        live, finished, max_steps = [], self._finished, self.max_steps
        for b, req in enumerate(self._requests):
            if req is None or b in finished:
                continue
            if not 0 <= req.position < len(req.rows) <= max_steps:
                raise ValueError(f"slot {b} is at position {req.position} of a run of {len(req.rows)} steps")
            live.append((b, req))
        return live

    def index_vector(self, live: list | None = None) -> list[int]:
        "host: the row every slot reads this tick, -1 for a free or finished slot (validated: nothing outside a slot's own run)"
        out, max_steps = [-1] * self.capacity, self.max_steps
        for b, req in self._running() if live is None else live:
            out[b] = b * max_steps + req.position
        return out

    def admit(self, slot: int, latents: torch.Tensor, wrapper, steps: int, seed: int | None = None, inpaint: Sequence[torch.Tensor] | None = None,
              guidance_scale: "float | Sequence[float] | None" = None, guidance_rescale: "float | Sequence[float]" = 0.0) -> None:  # fmt: skip
        """Start a request in a free slot: `latents` of one sample, `wrapper` with this request's schedule / stochasticity (same
        sampler structure as the batch; it is consumed by the dry run that produces the rows), `steps` its run length.
        `inpaint` (a batch built with `inpaint_mask_shape` only): (mask, original_samples, noise) of ONE sample -- the request is an
        in-painting one, stepped as `wrapper.set_inpaint` would step it alone; the batch copies the three into the slot's slices of
        its own tensors (the mask cast to the latents' dtype, as set_inpaint casts it).  None there: a plain request sharing the
        batch -- its mask is ones and its rows name neither the original nor the re-noising tensor.
        `guidance_scale` (a batch built with `guided=True` only, and required there): the request's classifier-free-guidance scale, a
        float, or a sequence of exactly `steps` floats -- a guidance schedule: the row of step i carries guidance_scale[i].
        `guidance_rescale` (non-zero on a batch built with `rescaled=True` only): the request's phi of diffusers' rescale_noise_cfg, a
        Python number >= 0, or a sequence of exactly `steps` of them -- a rescale schedule; a step whose phi is zero is not rescaled."""
        self._check_slot(slot)
        if self._requests[slot] is not None:
            raise ValueError(f"slot {slot} is busy: take() its result first" if slot in self._finished else f"slot {slot} is busy")
        steps = int(steps)
        if not 1 <= steps <= self.max_steps:
            raise ValueError(f"a request runs 1..{self.max_steps} steps (max_steps), not {steps}")
        if sampler_structure(wrapper) != self.structure:
            raise ValueError(f"this wrapper's sampler structure {sampler_structure(wrapper)} is not the batch's {self.structure}")
        scales = None
        if self.guided:
            if guidance_scale is None:
                raise ValueError("guidance_scale is required on a guided batch: a float, or one float per step (an unguided request hands step_guided the same prediction twice)")
            if isinstance(guidance_scale, (int, float)) and not isinstance(guidance_scale, bool):
                scales = [float(guidance_scale)] * steps
            else:
                try:
                    scales = [float(g) for g in guidance_scale]
                except TypeError:
                    raise ValueError(f"guidance_scale is a float or a sequence of {steps} floats, not {type(guidance_scale).__name__}") from None
                if len(scales) != steps:
                    raise ValueError(f"a guidance schedule has one scale per step: {len(scales)} scales for {steps} steps")
        elif guidance_scale is not None:
            raise ValueError("guidance_scale= needs a batch built with guided=True: this one steps with step(model_output)")
        rescales = self._rescales_of(guidance_rescale, steps)
        noisy = bool(wrapper.sampler.require_noise)
        if noisy and not self.draws_noise:
            raise ValueError("this wrapper draws noise and the batch's sampler structure does not")
        if noisy and self.structured:
            if (wrapper.noise_props if wrapper.noise_props is not None else type(self.noise_props)()) != self.noise_props:
                raise ValueError(f"this wrapper's noise_props {wrapper.noise_props} are not the batch's {self.noise_props}: they are arguments of the one draw launch")
            if getattr(wrapper, "prefetch_noise", False):
                raise ValueError("prefetch_noise=True: a rolling batch draws every slot's noise itself")
        if noisy and seed is None:
            raise ValueError("a request that draws noise needs a seed")
        if tuple(latents.shape) not in (self.unit_shape, (1, *self.unit_shape)) or latents.dtype != self.dtype:
            raise ValueError(f"latents of shape {tuple(latents.shape)} / {latents.dtype} in a batch of samples {self.unit_shape} / {self.dtype}")
        if self._advanced:
            raise ValueError("admit() between advance() and step(): this tick's index is already on the device; admit between ticks")
        if inpaint is not None:
            if not self.masked:
                raise ValueError("inpaint= needs a batch built with inpaint_mask_shape: this one steps with skr_step_launch_rolling")
            given = tuple(inpaint)
            if len(given) != 3 or any(not isinstance(t, torch.Tensor) for t in given):
                raise ValueError("inpaint is (mask, original_samples, noise): three tensors for one sample")
            if tuple(given[0].shape) not in (self.mask_shape, (1, *self.mask_shape)):
                raise ValueError(f"a mask of shape {tuple(given[0].shape)} in a batch of masks {self.mask_shape}")
            for name, t in (("original_samples", given[1]), ("noise", given[2])):
                if tuple(t.shape) not in (self.unit_shape, (1, *self.unit_shape)) or t.dtype != self.dtype:
                    raise ValueError(f"{name} of shape {tuple(t.shape)} / {t.dtype} in a batch of samples {self.unit_shape} / {self.dtype}")
        if self.masked:
            if inpaint is None:
                if getattr(wrapper, "_inpaint", None) is not None:
                    raise ValueError("this wrapper has set_inpaint in force: hand its tensors to admit(inpaint=...), the batch steps on its own copies")
                self.mask[slot].fill_(1.0)
            else:
                self.mask[slot].copy_(given[0].reshape(self.mask_shape))
                self.original[slot].copy_(given[1].reshape(self.unit_shape))
                self.noise[slot].copy_(given[2].reshape(self.unit_shape))
                # (the dry run steps on one-sample views of the batch's own tensors: the mechanism of CapturedLoop.retarget)
                wrapper.set_inpaint(self.mask[slot : slot + 1], self.original[slot : slot + 1], self.noise[slot : slot + 1])
        traced = self._trace(wrapper, steps, seed if noisy else None)
        if len(traced) != steps:
            raise SkrampleHipError(f"the schedule issued {len(traced)} launches for {steps} steps")
        request = _Request(self._rows_of(traced, scales, rescales) if self.guided else self._rows_of(traced), [t for _, _, t in traced])
        upload_rows(self.rows_dev, slot * self.max_steps, request.rows)
        self._x[-1][slot].copy_(latents.reshape(self.unit_shape))
        if noisy:
            value = int(seed) & 0xFFFFFFFFFFFFFFFF
            self.seeds_dev[slot : slot + 1].copy_(torch.tensor([value - (1 << 64) if value >= (1 << 63) else value], dtype=torch.int64))
        self._requests[slot] = request
        if self.device_positions:
            # stream-ordered, behind the rows: the slot's timesteps, then its run length and position (the next advance reads them)
            self.times_dev[slot * self.max_steps : slot * self.max_steps + steps].copy_(torch.tensor(request.times, dtype=torch.float32))
            self.length_dev[slot : slot + 1].fill_(steps)
            self.position_dev[slot : slot + 1].zero_()
            return
        self._times_host[slot] = request.times[0]
        self.timesteps.copy_(self._times_host)

    def _rescales_of(self, guidance_rescale, steps: int) -> list[float]:
        "guidance_rescale of every step of a request: a Python number >= 0 or exactly `steps` of them, non-zero on a rescaled batch only"

        def one(phi) -> float:
            if isinstance(phi, bool) or not isinstance(phi, lazy.NUMBER):
                raise ValueError(f"guidance_rescale is a Python number, not {type(phi).__name__}")
            if not phi >= 0.0:
                raise ValueError(f"guidance_rescale must be >= 0, not {phi}")
            return float(phi)

        if isinstance(guidance_rescale, (str, bytes, torch.Tensor)) or isinstance(guidance_rescale, lazy.NUMBER):
            rescales = [one(guidance_rescale)] * steps
        else:
            try:
                given = list(guidance_rescale)
            except TypeError:
                raise ValueError(f"guidance_rescale is a Python number, not {type(guidance_rescale).__name__}") from None
            rescales = [one(phi) for phi in given]
            if len(rescales) != steps:
                raise ValueError(f"a rescale schedule has one guidance_rescale per step: {len(rescales)} values for {steps} steps")
        if not self.rescaled and any(phi != 0.0 for phi in rescales):
            raise ValueError("guidance_rescale= needs a batch built with guided=True, rescaled=True: this one's tick has no statistics launch")
        return rescales

    def take(self, slot: int) -> torch.Tensor:
        "the result of a finished slot; the slot is free again"
        self._check_slot(slot)
        if slot not in self._finished:
            raise ValueError(f"slot {slot} holds no request" if self._requests[slot] is None else f"slot {slot} has not finished: {self._requests[slot].position} of {len(self._requests[slot].rows)} steps done")
        self._finished.discard(slot)
        self._requests[slot] = None
        if self.device_positions:
            self.length_dev[slot : slot + 1].zero_()  # free: inactive whatever its position holds
        return self._results.pop(slot)

    # ---- one tick --------------------------------------------------------------------------------------------------------------
    def _guard(self, model_output: torch.Tensor) -> None:
        for held, ptr, version in self._stamps:
            if held._version != version or held.data_ptr() != ptr:
                raise SkrampleHipError(ALIAS_HELP.format(what="was modified in place since"))
            if ptr == model_output.data_ptr():
                raise SkrampleHipError(ALIAS_HELP.format(what="its buffer now holds this tick's model output"))

    def _bind(self, role: Role, model_output: torch.Tensor, p: int = 0, outputs: Sequence[torch.Tensor] | None = None) -> torch.Tensor:
        """THE rule that turns a role into a tensor, for the eager tick (p = 0) and for phase p of CapturedTicks alike.  Every ring is read
        as it stands BEFORE the tick's rotation (_ticked), oldest first, p rotations on: the tick reads its latents from _x[P - 1 + p]
        and writes its results into entry p of every ring -- new latents, new state, this tick's draw, this tick's guided prediction --
        and the entry of -k ticks ago lies k places before either.  `outputs` (CapturedTicks): the graphs' static outputs, the
        model-output ring there; None: the caller's last model outputs, or `_blank` for one no tick has produced yet."""
        kind, P = role[0], len(self._x)
        if kind == "x":
            return self._x[(P - 1 + p) % P]
        if kind == "o":
            return model_output
        if kind == "none":
            return self._blank
        if kind in ("orig", "znoise") and self.masked:  # the batch's own in-paint tensors: the same in every phase
            return self.original if kind == "orig" else self.noise
        if kind in ("n", "pn") and self.structured:
            return self._n[(p + (role[1] if kind == "pn" else 0)) % len(self._n)]
        if len(role) < 2:
            raise SkrampleHipError(f"operand role {role} is not one a rolling batch binds (noise tensors of a batch built without structured noise, or an unknown role)")
        k = role[1]
        if kind == "pi":
            return self._x[(P - 1 + p + k) % P]
        if kind == "px":
            return self._state[(p + k) % P]
        if kind == "po" and self.guided:  # the batch's own guided prediction of -k ticks ago
            return self._g[(p + k) % P]
        if kind == "po" and outputs is not None:  # the static output of the graph replayed -k ticks ago
            return outputs[(p + k) % P]
        if kind == "po":
            return self._outputs[k] if -k <= len(self._outputs) else self._blank
        raise SkrampleHipError(f"operand role {role} is not one a rolling batch binds (noise tensors of a batch built without structured noise, or an unknown role)")

    def _operands(self, model_output: torch.Tensor, p: int = 0, outputs: Sequence[torch.Tensor] | None = None) -> tuple:
        "(operand pointer array, out0, out1) of the step launch of the eager tick, or of phase p: entry p of the rings takes the results"
        bind = self._bind
        arr = (ctypes.c_void_p * max(len(self.roles), 1))(*[bind(role, model_output, p, outputs).data_ptr() for role in self.roles])
        new_x = self._x[p]  # the oldest entries take this tick's results: no operand of the structure reaches that far back
        if self.two_outputs:
            return arr, self._state[p], new_x
        return (arr, new_x, None) if self.plan.out0_dtype != _hip.NONE else (arr, None, new_x)

    def _tick_begins(self, what: str, **tensors: torch.Tensor) -> list:
        "the refusals shared by step() and step_guided(), in their order; returns this tick's active (slot, request) pairs"
        if self._captured is not None:
            raise ValueError("this batch's ticks are captured: the rings' phase belongs to CapturedTicks.tick()")
        live = self._running()
        if not live:
            raise ValueError(f"no active slot: admit() a request before {what}()")
        if self.device_positions and not self._advanced:
            raise ValueError(f"device-resident positions: advance() publishes this tick's index and timesteps; call it before the network and {what}()")
        for name, t in tensors.items():
            if tuple(t.shape) != tuple(self._x[-1].shape) or t.dtype != self.dtype or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"{name} of a tick is a contiguous {tuple(self._x[-1].shape)} {self.dtype} tensor on {self.device}")
        return live

    def _publish(self, live: list) -> None:
        "host-published positions: one small stream-ordered copy of this tick's index, ahead of every launch of the tick"
        if not self.device_positions:
            self.index_dev.copy_(torch.tensor(self.index_vector(live), dtype=torch.int32))

    def step(self, model_output: torch.Tensor) -> list[int]:
        "advance every active slot by one step of its own run with ONE launch; returns the slots that finished with this tick"
        if self.guided:
            raise ValueError("this batch was built with guided=True: a tick is step_guided(uncond, cond), the guided prediction is formed inside its launch")
        live = self._tick_begins("step", **{"the model output": model_output})
        if self.alias_history:
            self._guard(model_output)
        elif self.keep:
            model_output = model_output.clone()
        self._publish(live)
        if self.structured:
            self._draw(self._n[0])  # behind the index, ahead of the step launch that reads it: the oldest draw's tensor takes this tick's
        self._launch(*self._operands(model_output))
        if self.keep:
            self._outputs.append(model_output)
            del self._outputs[: max(len(self._outputs) - self.keep, 0)]
            if self.alias_history:
                self._stamps.append((model_output, model_output.data_ptr(), model_output._version))
                del self._stamps[: max(len(self._stamps) - self.keep, 0)]
        return self._ticked(live)

    def step_guided(self, uncond: torch.Tensor, cond: torch.Tensor) -> list[int]:
        """A tick of a guided batch: ONE skr_step_launch_guided_rolling forms every active slot's guided prediction
        uncond + g * (cond - uncond) -- g the slot's own scale for its own step, from its row --, steps the slot with it and stores it
        into the batch's ring of guided predictions; returns the slots that finished with this tick.  Nothing of the caller is held: both
        tensors may be overwritten as soon as the launch is enqueued.  An unguided request sharing the batch gets the same prediction in
        both halves: cond - uncond is exactly 0 and the guided prediction is uncond (for finite values), whatever its scale."""
        if not self.guided:
            raise ValueError("step_guided() needs a batch built with guided=True: this one steps with step(model_output)")
        live = self._tick_begins("step_guided", uncond=uncond, cond=cond)
        self._publish(live)
        self._launch(*self._operands(uncond), cond, self._g[0] if self._g else None)  # (the oldest guided prediction's tensor takes this tick's)
        return self._ticked(live)

    def _ticked(self, live: list) -> list[int]:
        """THE host bookkeeping behind a tick's launches, for step(), step_guided() and CapturedTicks.tick(): every ring rotates -- the oldest
        entry, which took this tick's result, becomes the newest, so that `latents` is where admit() must write --, then positions, finished
        slots, the result clones and the next timesteps"""
        for ring in (self._x, self._state, self._n if self.structured else (), self._g):
            if ring:
                ring.append(ring.pop(0))
        new_x = self._x[-1]
        self.ticks += 1
        self._advanced = False
        done, on_host = [], not self.device_positions
        for b, req in live:
            req.position += 1
            if req.position == len(req.rows):
                done.append(b)
                self._finished.add(b)
                self._results[b] = new_x[b].clone()
            elif on_host:
                self._times_host[b] = req.times[req.position]
        # (the slices of free slots are not touched, by the kernel or here: they hold what an older tick left there)
        if not self.device_positions:
            self.timesteps.copy_(self._times_host)
        return done

    # ---- device-resident positions -------------------------------------------------------------------------------------------
    def advance(self) -> None:
        """Device-resident positions: ONE skr_rolling_advance computes this tick's `index_dev` and `timesteps` from the slots' device
        state and moves the running slots on.  Call it once per tick, before the network reads `timesteps`; `step()` consumes it."""
        if not self.device_positions:
            raise ValueError("advance() needs device_positions=True: this batch publishes its index from the host in step()")
        if self._captured is not None:
            raise ValueError("this batch's ticks are captured: the rings' phase belongs to CapturedTicks.tick()")
        if self._advanced:
            raise ValueError("advance() ran for this tick already: step() comes next")
        if not self._running():
            raise ValueError("no active slot: admit() a request before advance()")
        self._advance()
        self._advanced = True

    def capture(self, model: Callable[[torch.Tensor, torch.Tensor], torch.Tensor], warmup: int = 2) -> "CapturedTicks":
        "graphs of the advance and the network for every ring phase: see CapturedTicks"
        if not self.device_positions:
            raise ValueError("capture() needs device_positions=True: a tick that copies its index from the host cannot be captured")
        if self._captured is not None:
            raise ValueError("this batch's ticks are captured already")
        if any(r is not None for r in self._requests) or self._advanced:
            raise ValueError("capture() with a resident request: take() every result first (the warm-up runs the network on the rings)")
        self._captured = CapturedTicks(self, model, warmup)
        return self._captured


class CapturedTicks:
    """The ticks of a `RollingBatch(device_positions=True)` with the network in captured graphs.

    The latents and states rotate through rings of P = keep + 2 tensors, so a tick has one of P operand bindings: graph p holds, on
    one stream, the advance launch and `out_p = model(latents of phase p, timesteps)`.  `tick()` replays graph `ticks mod P` and
    follows it with one eager skr_step_launch_rolling whose operand array was built at capture time (a structured-noise batch: with the
    one draw launch of the phase's noise tensor between the two, eager for the same reason).  The step stays outside the
    graphs because its history operand ("po", k) is the static output of graph (p + k) mod P, which exists only once every graph
    is captured -- and that is why no model output is ever copied: the P static outputs ARE the model-output ring (it needs
    keep + 1 of them), they belong to the graphs, and nobody else can overwrite them (no alias guard).  `admit()` / `take()` of
    the batch work between ticks.  A guided batch: `model` returns `(uncond, cond)`; the uncond halves are `outputs`, the cond halves and
    the batch's own ring of guided predictions -- the ("po", k) history there -- are bound per phase beside the operand array, and the
    eager launch is one skr_step_launch_guided_rolling."""

    def __init__(self, batch: RollingBatch, model, warmup: int):
        self.batch = batch
        dev = batch.device
        self.phases = P = len(batch._x)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(max(int(warmup), 1)):
                model(batch._x[-1], batch.timesteps)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        # phase p reads the ring as it stands after p rotations; P rotations bring it back
        latents = [batch._x[(P - 1 + p) % P] for p in range(P)]
        self.graphs: list[torch.cuda.CUDAGraph] = []
        self.outputs: list[torch.Tensor] = []  # referenced here so that the graphs' pool keeps them alive
        self.conds: list[torch.Tensor] = []  # a guided batch: the cond halves, launch arguments of the phases' step launches
        pool = torch.cuda.graph_pool_handle()
        for p in range(P):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, pool=pool):
                batch._advance()
                out = model(latents[p], batch.timesteps)
            if batch.guided:  # the network returns (uncond, cond): `outputs` holds the uncond halves, the operand of role ("o",)
                if not isinstance(out, (tuple, list)) or len(out) != 2:
                    raise ValueError("the model of a guided batch returns (uncond, cond)")
                out, cond = out
                if tuple(cond.shape) != tuple(latents[p].shape) or cond.dtype != batch.dtype or cond.device != dev or not cond.is_contiguous():
                    raise ValueError(f"cond of a tick is a contiguous {tuple(latents[p].shape)} {batch.dtype} tensor on {dev}")
                self.conds.append(cond)
            if tuple(out.shape) != tuple(latents[p].shape) or out.dtype != batch.dtype or out.device != dev or not out.is_contiguous():
                raise ValueError(f"the model output of a tick is a contiguous {tuple(latents[p].shape)} {batch.dtype} tensor on {dev}")
            self.graphs.append(graph)
            self.outputs.append(out)
        self._bind_phases()
        self.ticks = 0
        self.replays = [0] * P

    def _bind_phases(self) -> None:
        """the step launch of every phase -- (operand pointers, out0, out1) --, the tensor its draw goes to and its guided arguments, from the
        rings as they stand and the graphs' outputs: RollingBatch._bind, the eager tick's rule, p rotations on"""
        batch, phases = self.batch, range(self.phases)
        self._launches = [batch._operands(self.outputs[p], p, self.outputs) for p in phases]
        # a structured-noise batch: the tick of phase p draws into entry p of the noise ring -- one tensor, or a ring of P
        self._draws = [batch._bind(("n",), None, p) for p in phases] if batch.structured else None
        # a guided batch: the tick of phase p stores its guided prediction into entry p of that ring; Euler stores none
        self._guides = [(self.conds[p], batch._g[p] if batch._g else None) for p in phases] if batch.guided else None

    def tick(self) -> list[int]:
        "one graph replay (advance + network), the draw of a structured-noise batch, and ONE step launch; returns the slots that finished with this tick"
        batch = self.batch
        live = batch._running()  # (validated before anything is enqueued)
        if not live:
            raise ValueError("no active slot: admit() a request before tick()")
        phase = self.ticks % self.phases
        self.graphs[phase].replay()
        if self._draws is not None:  # eager like the step launch, between the advance (in the graph) and the step that reads the draw
            batch._draw(self._draws[phase])
        batch._launch(*self._launches[phase], *(self._guides[phase] if self._guides is not None else ()))
        self.replays[phase] += 1
        self.ticks += 1
        return batch._ticked(live)  # the batch's rings follow the phase
