"""Whole-loop capture: record an N-step sampling loop (network + fused sampler steps) into one HIP graph.

Every launch of this engine is capture-safe by construction (`skr_step_launch` only enqueues a kernel on the
caller's stream: no allocation, no synchronisation, no host read-back; per-sample seeds and all operands are
read from device memory at run time), so a sampling loop whose network is itself capturable can be recorded
with `torch.cuda.graph` and replayed with new inputs / new seeds at ~10 us of host cost for the whole loop.
This removes the per-step Python + launch overhead that dominates small batches.

`indexed=True` additionally moves every step's scalars (coefficients, zeta, Philox stream ids, conversion constants) out
of the frozen kernel arguments into a device-resident table (`skr_step_launch_indexed`, include/skrample_hip.h): the kernels
read row `index + k` when they run.  The captured loop then serves ANY schedule of its length -- other sigmas, flow shift
(`mu`), begin index, stochasticity -- by rewriting the table (`CapturedLoop.retarget`, a dry run of the new scheduler on one
sample plus one small copy; no re-capture), and keeps several schedules resident at once, selected per replay by moving the
device-resident index (`loop(latents, slot=k)`).  The network's timestep argument is data as well: with `device_timesteps`
(the default of an indexed capture) `model(x, t)` receives 0-d elements of ONE device tensor, as a diffusers pipeline's
`for t in scheduler.timesteps` does, and re-targeting / switching slots rewrites that tensor -- a host float would be frozen into
the captured network.  The reference redoes this work on the host every step, with a device sync
(skrample/diffusers.py:565-567, skrample/scheduling.py:51-62, skrample/sampling/interface.py:34-59).

`per_sample=True` (with `indexed=True`) makes the schedule per SAMPLE: the index becomes an int32 vector with one entry per sample
(`skr_step_launch_indexed_per_sample`), and `loop(latents, slot=[2, 0, 1, ...])` lets every sample of one replay follow its own
resident schedule -- a batch of requests with different shifts, sigma families, stochasticities or begin indices in one launch per
step.  With `device_timesteps` the network's `t` is then a 1-D tensor of shape `[batch]` (row i of one `[steps, batch]` device
tensor), the per-sample form diffusers models accept.  A sample's result is bit-identical to the one the whole-batch `slot=k` gives it.

In-painting (`wrapper.set_inpaint(mask, original_samples, noise)` in force when the loop is captured) goes through all of this: the
masked steps of an indexed capture are `skr_step_launch_masked_indexed[_per_sample]` launches whose blend coefficients -- the alpha
and sigma of each step's target -- sit in the rows beside the step's own, so strength (begin index), shift and schedule are data.
The wrapper's three in-paint tensors are the loop's static buffers (`loop.inpaint`); `loop(latents, inpaint=(mask, original,
noise))` copies a new request's into them ahead of the replay.

Classifier-free guidance (`guidance_scale=`): `model(x, t)` returns `(uncond, cond)` and the loop body is `wrapper.step_guided(uncond,
cond, guidance_scale, t, x)`, whose guidance runs inside the step launch.  A plain capture freezes the scale into the graph; an indexed
one keeps it in the rows (`skr_step_launch_guided_indexed[_per_sample]`), so `retarget(wrapper, slot, guidance_scale=...)` loads another
scale beside another schedule, several scales stay resident, and with `per_sample=True` every sample of a replay follows its own.

Rescaled guidance (`guidance_rescale=`, diffusers' `rescale_noise_cfg`): a plain capture freezes phi into the graph.  An indexed capture
made with `rescaled=True` keeps it in the rows beside the scale (`convert_k[1]`): every guided step of the graph is the statistics row
launch and the rescaled row step (`skr_guidance_rescale_factor_indexed[_per_sample]`, `skr_step_launch_guided_rescaled_indexed[_per_sample]`)
on one factor tensor and one workspace the loop owns, `retarget(wrapper, slot, guidance_rescale=...)` loads another phi -- 0.0 included,
which makes the first launch return at once and the second the plain guided step -- and with `per_sample=True` every sample follows its
own.  Without `rescaled=True` an indexed capture refuses a non-zero `guidance_rescale`, as before.
"""

from __future__ import annotations

import contextlib
import gc
from collections import OrderedDict
from typing import Callable, Sequence

import torch


@contextlib.contextmanager
def _no_collection():
    """No cyclic garbage collection while a stream captures.  A dead reference cycle may hold a CapturedLoop (an exception kept with its
    traceback is enough), and the collector runs wherever an allocation tips its counters -- inside a step of the loop being captured, for
    one.  Destroying a graph there ends the process: on ROCm torch's graph destructor synchronises the device, which a capturing stream
    forbids, and the error leaves a destructor.  The cycle is collected after the capture instead."""
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_enabled:
            gc.enable()


class CapturedLoop:
    "replayable sampling loop: `out = loop(initial_latents, seeds=None)`"

    def __init__(self, graph: torch.cuda.CUDAGraph, static_in: torch.Tensor, static_out: torch.Tensor, seeds_dev: torch.Tensor | None, rows=None, runner=None,
                 static_times: torch.Tensor | None = None, sample_times: torch.Tensor | None = None, inpaint: tuple | None = None,
                 guidance_scale: float | None = None, guidance_rescale: float = 0.0, rescaled: bool = False):
        self.guidance_scale = guidance_scale  # the scale the loop was captured with, or None: a loop captured without guidance
        # the phi the loop was captured with, and whether it is a row value (captured with rescaled=True) that retarget may replace
        self.guidance_rescale, self.rescaled = guidance_rescale, rescaled
        self.inpaint = inpaint  # (mask, original_samples, noise) the captured masked steps read, or None: a loop captured without in-painting
        self.graph, self.static_in, self.static_out, self.seeds_dev = graph, static_in, static_out, seeds_dev
        self.rows, self._runner = rows, runner  # _hip.IndexedRows of an indexed capture; runner(wrapper, x) = the captured loop body
        self._filled = {0}  # table slots that hold a schedule (the capture itself fills slot 0; the others start as zero rows)
        # device_timesteps: the tensor whose elements the captured network reads as `t`, and each slot's values for it
        self.static_times = static_times
        self._times = {0: static_times.detach().cpu().clone()} if static_times is not None else {}
        self._times_slot = 0
        # per-sample capture: the [steps, batch] tensor whose rows the network reads as `t`, and the slot every sample follows now
        self.sample_times = sample_times
        self._sample_slots = [0] * self.batch if self.per_sample else None

    @property
    def slots(self) -> int:
        return self.rows.slots if self.rows is not None else 1

    @property
    def per_sample(self) -> bool:
        "captured with per_sample=True: `slot` may name a schedule slot for every sample"
        return self.rows is not None and getattr(self.rows, "sample_index_dev", None) is not None

    @property
    def batch(self) -> int:
        return int(self.static_in.shape[0])

    def _check_slots(self, slot) -> list[int]:
        "a per-sample slot argument as a validated list (host only: nothing is enqueued before every entry is known to be good)"
        if isinstance(slot, torch.Tensor):
            if slot.device.type != "cpu" or slot.dtype.is_floating_point or slot.dtype in (torch.bool, torch.complex64, torch.complex128) or slot.dim() != 1:
                raise ValueError("per-sample slots are a host sequence or a 1-D CPU integer tensor (a device tensor could not be validated without a sync)")
            slot = slot.tolist()
        chosen = [int(k) for k in slot]
        if len(chosen) != self.batch:
            raise ValueError(f"{len(chosen)} slots for a captured batch of {self.batch}")
        for k in chosen:
            if not 0 <= k < self.rows.slots:
                raise ValueError(f"slot {k} outside 0..{self.rows.slots - 1}")
            if k not in self._filled:
                raise ValueError(f"schedule slot {k} has never been loaded: call retarget(wrapper, slot={k}) first (its rows are all zero)")
        return chosen

    def _assemble_times(self, chosen: Sequence[int]) -> torch.Tensor:
        "host [steps, batch]: column b holds the timesteps of the slot sample b follows (from the per-slot copies in `_times`)"
        return torch.stack([self._times[k] for k in chosen], dim=1)

    def _publish_sample_times(self) -> None:
        if self.sample_times is not None:
            self.sample_times.copy_(self._assemble_times(self._sample_slots))  # one copy, stream-ordered ahead of the replay

    def retarget(self, wrapper, slot: int = 0, guidance_scale: float | None = None, guidance_rescale: float | None = None) -> None:
        """Load the step scalars of `wrapper` (same sampler structure and number of steps as the captured one, any schedule /
        shift / begin index / stochasticity) into table slot `slot`: a dry run of its loop on one sample fills the rows, one
        small host-to-device copy publishes them.  The graph itself is untouched.
        A loop captured with `guidance_scale` loads a scale into the slot as well: `guidance_scale`, or the captured one when None.
        A loop captured with `rescaled=True` loads a phi too: `guidance_rescale`, or the captured one when None; 0.0 turns the rescale
        off for that slot.  On any other loop a `guidance_rescale` is refused: its phi, if any, is frozen into the graph.
        A loop captured with in-painting takes a wrapper that has `set_inpaint(...)` in force itself (the dry run steps on one-sample
        views of ITS tensors); only its scalars reach the graph, which goes on reading `loop.inpaint`."""
        from . import _hip

        if self.rows is None:
            raise ValueError("capture the loop with indexed=True to re-target it")
        if not 0 <= slot < self.rows.slots:
            raise ValueError(f"slot {slot} outside 0..{self.rows.slots - 1}")
        if guidance_scale is not None and self.guidance_scale is None:
            raise ValueError("this loop was captured without guidance: pass guidance_scale= to capture_sampling_loop")
        if guidance_rescale is not None and not self.rescaled:
            raise ValueError("this loop was captured without rescaled=True: its guidance_rescale is not a row value; pass rescaled=True to capture_sampling_loop")
        if self.guidance_scale is not None:
            from .sampling import lazy

            scale = guidance_scale if guidance_scale is not None else self.guidance_scale
            phi = guidance_rescale if guidance_rescale is not None else self.guidance_rescale
            lazy.check_guidance_numbers(scale, phi)  # (before anything of the slot changes)
        self.rows.begin("refill", slot)
        _hip.indexed = self.rows
        try:
            if self.guidance_scale is None:
                self._runner(wrapper, self.static_in[:1].clone())
            else:
                self._runner(wrapper, self.static_in[:1].clone(), scale, phi)
        finally:
            _hip.indexed = None
        if self.rows.cursor != self.rows.length:
            raise _hip.SkrampleHipError(f"the new schedule issued {self.rows.cursor} launches, the captured loop has {self.rows.length}: re-capture")
        self.rows.upload(slot)
        self._filled.add(slot)
        if self.static_times is not None:
            times = wrapper.timesteps.detach().to("cpu", self.static_times.dtype)
            if times.shape != self.static_times.shape:
                raise _hip.SkrampleHipError(f"the new schedule has {times.numel()} timesteps, the captured loop {self.static_times.numel()}: re-capture")
            self._times[slot] = times.clone()
            if slot == self._times_slot:
                self.static_times.copy_(self._times[slot])
            if self.sample_times is not None and slot in self._sample_slots:
                self._publish_sample_times()  # the columns of the samples that follow this slot

    def __call__(self, latents: torch.Tensor, seeds: Sequence[int] | None = None, slot: int | Sequence[int] | torch.Tensor | None = None,
                 inpaint: Sequence[torch.Tensor] | None = None) -> torch.Tensor:
        """Replay on `latents`.  `slot`: the resident schedule to follow -- an int for the whole batch; on a loop captured with
        `per_sample=True` also a host sequence or 1-D CPU integer tensor with one slot per sample.  `inpaint`: (mask, original_samples,
        noise) of the captured shapes, copied into `loop.inpaint` ahead of the replay (a loop captured with in-painting only)."""
        if inpaint is not None:
            if self.inpaint is None:
                raise ValueError("this loop was captured without in-painting: call wrapper.set_inpaint(...) before capture_sampling_loop")
            given = tuple(inpaint)
            if len(given) != 3 or any(not isinstance(t, torch.Tensor) or t.shape != held.shape for t, held in zip(given, self.inpaint)):
                raise ValueError(f"inpaint is (mask, original_samples, noise) of shapes {[tuple(t.shape) for t in self.inpaint]}")
        chosen = None
        if slot is not None and not isinstance(slot, int):
            if not self.per_sample:
                raise ValueError("one slot per sample needs a loop captured with capture_sampling_loop(..., indexed=True, per_sample=True)")
            chosen = self._check_slots(slot)
        self.static_in.copy_(latents)
        if inpaint is not None:
            for held, new in zip(self.inpaint, given):
                held.copy_(new)  # (stream-ordered ahead of the replay; a bool / uint8 mask is cast as set_inpaint casts it)
        if chosen is not None:
            self.rows.select(chosen)  # sample b reads row slot[b] * length + position in the loop
            if self.sample_times is not None and chosen != self._sample_slots:
                self._sample_slots = chosen
                self._publish_sample_times()
            self._sample_slots = chosen
        elif slot is not None:
            if self.rows is None or not 0 <= slot < self.rows.slots:
                raise ValueError("no such schedule slot")
            if slot not in self._filled:
                raise ValueError(f"schedule slot {slot} has never been loaded: call retarget(wrapper, slot={slot}) first (its rows are all zero)")
            self.rows.index_dev.fill_(slot * self.rows.length)  # the device-resident step index: row = index + position in the loop
            if self.per_sample:
                self.rows.sample_index_dev.fill_(slot * self.rows.length)
                if self.sample_times is not None and self._sample_slots != [slot] * self.batch:
                    self._sample_slots = [slot] * self.batch
                    self._publish_sample_times()
                self._sample_slots = [slot] * self.batch
            if self.static_times is not None and slot != self._times_slot:
                self.static_times.copy_(self._times[slot])  # what the network reads as `t` (stream-ordered ahead of the replay)
                self._times_slot = slot
        if seeds is not None:
            if self.seeds_dev is None:
                raise ValueError("this loop draws no noise")
            from .pytorch.noise import seeds_tensor

            self.seeds_dev.copy_(seeds_tensor([int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds], self.seeds_dev.device))
        self.graph.replay()
        return self.static_out.clone()


class CapturedLoops:
    """Captured sampling loops for ANY run length: `out = loops(latents, steps, seeds=None)`.

    A run's length shapes the loop itself (number of launches, the multistep ramp-up, the operands of every step), so a graph
    serves one length; the reference's loop takes `steps` per call (skrample/sampling/interface.py:34-59).  This keeps one
    `CapturedLoop` per length, recorded the first time that length is asked for (one eager warm-up + one capture, tens of
    milliseconds) and replayed afterwards; the `keep` most recently used lengths stay resident, the oldest graph and its static
    buffers are dropped beyond that.  `make_wrapper()` returns a fresh scheduler wrapper per capture (a graph reads its wrapper's
    device buffers, so lengths cannot share one); the other arguments are `capture_sampling_loop`'s."""

    def __init__(self, make_wrapper: Callable[[], object], model: Callable[[torch.Tensor, torch.Tensor], torch.Tensor], example: torch.Tensor, seeds: Sequence[int] | None = None,
                 keep: int = 8, **capture_options):
        if keep < 1:
            raise ValueError("keep at least one captured length")
        self._make, self._model, self._example, self._seeds, self._options = make_wrapper, model, example, seeds, capture_options
        self.keep = keep
        self._loops: OrderedDict[int, CapturedLoop] = OrderedDict()
        self.captures = 0  # how many graphs were recorded so far (a replay of a resident length adds none)

    def loop(self, steps: int) -> CapturedLoop:
        "the captured loop of this run length (recorded now if it is not resident)"
        steps = int(steps)
        if steps < 1:
            raise ValueError(f"a sampling loop has at least one step, not {steps}")
        found = self._loops.get(steps)
        if found is None:
            found = capture_sampling_loop(self._make(), self._model, self._example, steps, seeds=self._seeds, **self._options)
            self.captures += 1
            self._loops[steps] = found
            while len(self._loops) > self.keep:
                self._loops.popitem(last=False)
        self._loops.move_to_end(steps)
        return found

    @property
    def resident(self) -> tuple[int, ...]:
        "run lengths whose graphs are resident, least recently used first"
        return tuple(self._loops)

    def __call__(self, latents: torch.Tensor, steps: int, seeds: Sequence[int] | None = None, slot: int | Sequence[int] | torch.Tensor | None = None,
                 inpaint: Sequence[torch.Tensor] | None = None) -> torch.Tensor:
        return self.loop(steps)(latents, seeds, slot, inpaint)


def capture_sampling_loop(wrapper, model: Callable[[torch.Tensor, torch.Tensor], torch.Tensor], example: torch.Tensor, steps: int, seeds: Sequence[int] | None = None, warmup: int = 2,
                          indexed: bool = False, slots: int = 4, device_timesteps: bool | None = None, per_sample: bool = False,
                          guidance_scale: float | None = None, rescaled: bool = False, guidance_rescale: float = 0.0) -> CapturedLoop:
    """Capture `for t in wrapper.timesteps: x = wrapper.step(model(x, t), t, x)` for `steps` steps.

    `wrapper` is any scheduler wrapper of skrample_amd.diffusers; `model(x, t)` must be capturable (pure device
    work); `example` fixes shape/dtype/device.  Warm-up passes run eagerly first so that every step program is
    lowered and every allocation pattern is known before capture.

    `device_timesteps` (default: the value of `indexed`): `t` is a 0-d element of the scheduler's device-resident `timesteps`
    tensor -- located by the wrapper through its storage offset, no read-back -- instead of a host float; the network then
    follows a re-targeted schedule, because the tensor's contents are replaced with the rows.

    `per_sample` (needs `indexed=True`; off by default, and then nothing changes): every sample of a replay may follow its own slot,
    `loop(latents, slot=[...])`; with `device_timesteps` the network receives a 1-D `t` of shape `[batch]`.  Needs samples of at least
    2048 elements and a multiple of 8 (below).  `slots` may be as large as the batch (one schedule per request): the table is
    `slots * launches per loop * 328 bytes` of device memory -- 256 slots of a 30-launch loop are 2.5 MB.

    Sample sizes of an indexed capture.  Samples of whole 2048-element chunks are served for every sampler the row kernels cover.
    Ragged samples -- at least 2048 elements, a multiple of 8, not whole chunks: most non-square SDXL latent buckets, (4,144,112) for
    one -- are served, with or without `per_sample`, for the samplers whose step is one single-output launch (Euler, DPM 1-3, Adams,
    UniP) in one 16- or 32-bit dtype under the default compute scale, with `Random` noise or none.  UniPC and SPC, the Runge-Kutta
    wrappers, in-painting, guidance and `compute_scale=float64` on ragged samples are refused during the recording pass, before the
    stream captures; so are samples below 2048 elements or not a multiple of 8 wherever a row kernel needs a sample size.

    A wrapper with `set_inpaint(...)` in force is captured with its masked steps; its three in-paint tensors become static buffers of
    the loop (`loop.inpaint`).  With `indexed=True` the masked row kernel must cover the launches -- samples of whole 2048-element
    chunks, one 16- or 32-bit dtype for latents and mask, a mask of a multiple of 8 elements per sample, no `compute_scale=float64`
    -- and anything else is refused during the recording pass, before the stream captures.

    `guidance_scale` (None: nothing changes): `model(x, t)` returns `(uncond, cond)` and the loop body is
    `x = wrapper.step_guided(uncond, cond, guidance_scale, t, x)`.  With `indexed=False` the scale is frozen into the graph, and every
    sampler `step_guided` serves is captured.  With `indexed=True` the scale is a row value beside the step's scalars
    (`loop.retarget(wrapper, slot, guidance_scale=...)`; per sample with `per_sample=True`), and the guided row kernel must cover the
    launches: a sampler whose step is one single-output launch (Euler, DPM, Adams, UniP), contiguous latents of whole 2048-element chunks
    in one 16- or 32-bit dtype, no `set_inpaint`, no `compute_scale=None` / `float64`.  Anything else -- UniPC and SPC among them, whose
    guidance is a launch of its own -- is refused during the recording pass, before the stream captures.

    `guidance_rescale` (with `guidance_scale`; 0.0: nothing changes): the loop body is `wrapper.step_guided(..., guidance_rescale=...)`.
    With `indexed=False` the statistics launch and the rescaled step are captured, guidance_rescale frozen into the graph.  A loop
    captured without `rescaled` has no row form of rescaled guidance: `indexed=True` (and so `per_sample`) with a non-zero
    guidance_rescale is refused during the recording pass, before the stream captures.

    `rescaled` (a keyword, like its neighbours; needs `indexed=True` and `guidance_scale`; off by default, and then nothing changes): guidance_rescale -- 0.0 allowed --
    is a row value beside the scale.  Every guided step of the graph is two launches, the statistics row launch and the rescaled row
    step, on one factor tensor `[batch]` and one workspace the loop owns; `loop.retarget(wrapper, slot, guidance_rescale=...)` loads
    another phi, zero included, and with `per_sample=True` every sample follows its own.  On top of what a guided indexed capture needs,
    every sample must be made of whole 2048-element chunks.  Anything else is refused during the recording pass, before the stream
    captures.
    """
    if per_sample and not indexed:
        raise ValueError("per_sample=True needs indexed=True: only device-resident rows can differ by sample")
    if guidance_rescale != 0.0 and guidance_scale is None:
        raise ValueError("guidance_rescale belongs to a guided loop: pass guidance_scale= as well")
    if rescaled and not indexed:
        raise ValueError("rescaled=True needs indexed=True: it makes guidance_rescale a value of the device-resident rows (a plain capture freezes it into the graph)")
    if rescaled and guidance_scale is None:
        raise ValueError("rescaled=True belongs to a guided loop: pass guidance_scale= as well")
    from .pytorch import noise as _noise

    _noise._private_vectors[0] += 1  # the loop's seed vector is overwritten in place by replays with new seeds: it is this loop's alone
    try:
        return _capture(wrapper, model, example, steps, seeds, warmup, indexed, slots, device_timesteps, per_sample, guidance_scale, guidance_rescale, rescaled)
    finally:
        _noise._private_vectors[0] -= 1


def _capture(wrapper, model, example: torch.Tensor, steps: int, seeds, warmup: int, indexed: bool, slots: int, device_timesteps, per_sample: bool = False,
             guidance_scale: float | None = None, guidance_rescale: float = 0.0, rescaled: bool = False) -> CapturedLoop:
    dev = example.device
    static_in = example.clone()
    gen = list(seeds) if seeds is not None else None
    if device_timesteps is None:
        device_timesteps = indexed

    wrapper.set_timesteps(steps)
    static_times = None
    if device_timesteps:
        if wrapper.timesteps.device != dev:
            wrapper.set_timesteps(steps, device=dev)
        static_times = wrapper.timesteps  # (the scheduler remembers what it handed out for as long as this tensor lives)
        times = [static_times[i] for i in range(static_times.numel())]
    else:
        times = wrapper.timesteps.tolist()
    # per-sample: the network's `t` is row i of one [steps, batch] device tensor; the wrapper keeps its own 0-d timesteps[i]
    sample_times = static_times.detach().clone().unsqueeze(1).repeat(1, example.shape[0]).contiguous() if per_sample and device_timesteps else None
    model_times = [sample_times[i] for i in range(sample_times.shape[0])] if sample_times is not None else times

    def step_of(w, x, t, tm, generator, scale, rescale=guidance_rescale):  # the loop body: a guided capture's network returns (uncond, cond)
        if scale is None:
            return w.step(model(x, tm), t, x, generator=generator, return_dict=False)[0]
        uncond, cond = model(x, tm)
        return w.step_guided(uncond, cond, scale, t, x, generator=generator, return_dict=False, guidance_rescale=rescale)[0]

    def run(x):
        wrapper.reset_run()  # same schedule, same device seed vector; history and draw counter rewound
        for t, tm in zip(times, model_times):
            x = step_of(wrapper, x, t, tm, gen, guidance_scale)
        return x

    def run_other(other, x, scale=None, rescale=guidance_rescale):  # the same loop body on another scheduler instance (re-targeting dry run, one sample) under its own scale and phi
        other.set_timesteps(steps, device=dev) if device_timesteps else other.set_timesteps(steps)
        sub = gen[: x.shape[0]] if gen is not None else None
        ts = other.timesteps
        held = getattr(other, "_inpaint", None)
        if held is not None:  # in-painting: the dry run's samples of the new wrapper's own tensors (views; only its scalars reach the rows)
            mask, original, noise = held
            n = x.shape[0]
            other._inpaint = (mask[:n] if mask.dim() == original.dim() and mask.shape[0] > n else mask, original[:n], noise[:n])
        try:
            for t in ([ts[i] for i in range(ts.numel())] if device_timesteps else ts.tolist()):
                tm = t.reshape(1).expand(x.shape[0]) if sample_times is not None else t  # (the dry run's samples: `t` of shape [1])
                x = step_of(other, x, t, tm, sub, scale, rescale)
        finally:
            if held is not None:
                other._inpaint = held
        return x

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(max(warmup, 1)):
            run(static_in)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    if hasattr(wrapper, "noise_quiesced"):
        wrapper.noise_quiesced()  # the warm-up may have drawn noise ahead on the wrapper's side stream; the device is idle now

    rows = None
    if indexed:
        from . import _hip

        rows = _hip.IndexedRows(dev, slots=slots, batch=int(example.shape[0]) if per_sample else None, guided=guidance_scale is not None,
                                rescaled=rescaled, samples=int(example.shape[0]))  # (samples: the factor's size, and the sample size of a ragged launch without noise)
        _hip.indexed = rows
        try:
            rows.begin("record")
            run(static_in)  # recording pass: one row per launch, in launch order
            torch.cuda.synchronize(dev)
            rows.finish_recording()
            rows.begin("emit")
            graph = torch.cuda.CUDAGraph()
            with _no_collection(), torch.cuda.graph(graph):
                static_out = run(static_in)
        finally:
            _hip.indexed = None
        if rows.cursor != rows.length:
            raise _hip.SkrampleHipError("the captured loop issued a different number of launches than the recording pass")
    else:
        graph = torch.cuda.CUDAGraph()
        with _no_collection(), torch.cuda.graph(graph):
            static_out = run(static_in)
    seeds_dev = getattr(getattr(wrapper, "_noise_generator", None), "_seeds", None)
    from .pytorch.noise import forget_seed_vector

    forget_seed_vector(seeds_dev)  # the graph reads this very buffer and replays may overwrite it: no other run may share it from now on
    return CapturedLoop(graph, static_in, static_out, seeds_dev, rows, run_other, static_times, sample_times, getattr(wrapper, "_inpaint", None), guidance_scale, guidance_rescale, rescaled)
