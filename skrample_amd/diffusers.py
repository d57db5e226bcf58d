"""Scheduler-shaped wrappers: the outer drop-in boundary (what a diffusers pipeline calls).

Same classes, dataclass fields, properties and methods as reference `skrample/diffusers.py`
(parse_diffusers_config :112-196, as_diffusers_config :206-230, SkrampleWrapperCore :233-388,
SkrampleWrapperScheduler :390-599, RKWrapperCore :602-873, RKUltraWrapperScheduler :876-963,
DynasauRKWrapperScheduler :966-1041).  Like the reference, `diffusers` itself is never imported.

What `step()` does differently from the reference (diffusers.py:550-599):
  * no `.to(compute_scale)` / `.to(out dtype)` passes: bf16/fp16 inputs are widened in registers and
    the result is rounded once inside the single fused kernel;
  * history holds aliases of the caller's tensors, not deep copies (structured.py:113-125 deep-copies
    every tensor field through dataclasses.asdict);
  * white noise is drawn inside the step kernel (Philox), other noise types by one batched launch;
  * a device-resident `timestep` tensor is not `.item()`-synchronised: steps are assumed to arrive in
    schedule order from `set_begin_index` (host numbers / CPU tensors are looked up by value exactly
    as in the reference, raising ValueError when absent).
"""

from __future__ import annotations

import abc
import contextlib
import ctypes
import dataclasses
import functools
import math
import weakref
from collections import OrderedDict
from collections.abc import Hashable, Mapping, Sequence
from types import MappingProxyType
from typing import Any

import numpy as np
import torch
from torch import Tensor

from . import scheduling
from .common import DeltaPoint, MergeStrategy, Point, Step
from .pytorch.noise import SUBSTREAMS, BatchTensorNoise, HostRandomBatch, Offset, Pyramid, Random, TensorNoiseCommon, TensorNoiseProps
from . import _hip
from .sampling import functional, interface, lazy, models, program, tableaux, traits
from .sampling import structured as sampling
from .sampling.lazy import LazyTensor, Lin, PhiloxNoise, SkrampleHipError, empty_output, lift
from .sampling.models import DataModel, DiffusionModel, FlowModel, NoiseModel, VelocityModel
from .sampling.structured import SampleInput, SKSamples, StructuredSampler
from .scheduling import ScheduleCommon, ScheduleModifier, SkrampleSchedule, SubSchedule

DIFFUSERS_CLASS_MAP: dict[str, tuple[type[StructuredSampler], dict[str, Any]]] = {
    "DDIMScheduler": (sampling.Euler, {}),
    "DDPMScheduler": (sampling.Euler, {"stochasticity": True}),
    "DPMSolverMultistepScheduler": (sampling.DPM, {}),
    "DPMSolverSDEScheduler": (sampling.DPM, {"stochasticity": True, "order": 1}),
    "EulerAncestralDiscreteScheduler": (sampling.Euler, {"stochasticity": True}),
    "EulerDiscreteScheduler": (sampling.Euler, {}),
    "FlowMatchEulerDiscreteScheduler": (sampling.Euler, {}),
    "IPNDMScheduler": (sampling.Adams, {"order": 4}),
    "MiniMaxH3Scheduler": (sampling.Euler, {}),
    "UniPCMultistepScheduler": (sampling.UniPC, {}),
}

DIFFUSERS_KEY_MAP: dict[str, str] = {
    "shift": "shift",
    "flow_shift": "shift",
    "solver_order": "order",
    "num_train_timesteps": "base_timesteps",
}
DIFFUSERS_KEY_MAP_REV: dict[str, str] = {v: k for k, v in DIFFUSERS_KEY_MAP.items()}

DIFFUSERS_VALUE_MAP: dict[tuple[str, Any], tuple[str, Any]] = {
    ("beta_schedule", "linear"): ("beta_scale", 1),
    ("beta_schedule", "scaled_linear"): ("beta_scale", 2),
    ("algorithm_type", "dpmsolver"): ("stochasticity", False),
    ("algorithm_type", "dpmsolver++"): ("stochasticity", False),
    ("algorithm_type", "sde-dpmsolver"): ("stochasticity", True),
    ("algorithm_type", "sde-dpmsolver++"): ("stochasticity", True),
    ("prediction_type", "epsilon"): ("skrample_predictor", NoiseModel()),
    ("prediction_type", "flow"): ("skrample_predictor", FlowModel()),
    ("prediction_type", "sample"): ("skrample_predictor", DataModel()),
    ("prediction_type", "v_prediction"): ("skrample_predictor", VelocityModel()),
    # later entries win
    ("use_flow_sigmas", True): ("skrample_subschedule", None),
    ("use_beta_sigmas", True): ("skrample_subschedule", scheduling.Beta),
    ("use_exponential_sigmas", True): ("skrample_subschedule", scheduling.Exponential),
    ("use_karras_sigmas", True): ("skrample_subschedule", scheduling.Karras),
}
DIFFUSERS_VALUE_MAP_REV: dict[tuple[str, Any], tuple[str, Any]] = {v: k for k, v in DIFFUSERS_VALUE_MAP.items()}

DEFAULT_FAKE_CONFIG = {
    "base_image_seq_len": 256,
    "base_shift": 0.5,
    "max_image_seq_len": 4096,
    "max_shift": 1.15,
    "use_dynamic_shifting": True,
}


@dataclasses.dataclass(frozen=True)
class ParsedDiffusersConfig:
    sampler: type[StructuredSampler]
    sampler_props: dict[str, Any]
    schedule: type[SkrampleSchedule]
    schedule_props: dict[str, Any]
    subschedule: type[SubSchedule] | None
    subschedule_props: dict[str, Any]
    schedule_modifiers: list[tuple[type[ScheduleModifier], dict[str, Any]]]
    model: DiffusionModel
    invert_prediction: bool


def _field_names(cls) -> list[str]:
    return [f.name for f in dataclasses.fields(cls)]


def parse_diffusers_config(config, sampler: type[StructuredSampler] | None = None, schedule: type[SkrampleSchedule] | None = None) -> ParsedDiffusersConfig:
    "translate a diffusers scheduler (or its config dict) into skrample classes + keyword props"
    class_name = config.get("_class_name", "") if isinstance(config, dict) else type(config).__name__
    if not isinstance(config, dict):
        config = dict(config.config)

    mapped: dict[str, Any] = {dst: config[src] for src, dst in DIFFUSERS_KEY_MAP.items() if src in config}
    for (src, src_value), (dst, dst_value) in DIFFUSERS_VALUE_MAP.items():
        if src in config and config[src] == src_value:
            mapped[dst] = dst_value

    if "skrample_predictor" in mapped:
        model: DiffusionModel = mapped.pop("skrample_predictor")
    elif "shift" in mapped:
        model = FlowModel()
    else:
        model = NoiseModel()

    sampler_props: dict[str, Any] = {}
    if not sampler:
        sampler, sampler_props = DIFFUSERS_CLASS_MAP.get(class_name, (sampling.DPM, {}))

    if not schedule:
        if isinstance(model, FlowModel):
            schedule = scheduling.Linear
        elif config.get("rescale_betas_zero_snr", False):
            schedule = scheduling.ZSNR
        else:
            schedule = scheduling.Scaled

    # a Linear schedule for a non-flow model starts at the sigma the beta schedule would reach
    if "sigma_start" not in mapped and not isinstance(model, FlowModel) and issubclass(schedule, scheduling.Linear):
        beta = scheduling.Scaled(**{k: v for k, v in mapped.items() if k in _field_names(scheduling.Scaled)})
        mapped["sigma_start"] = beta.space.regularize(beta.point_1.sigma).item()

    modifiers: list[tuple[type[ScheduleModifier], dict[str, Any]]] = []
    subschedule: type[SubSchedule] | None = None
    subschedule_props: dict[str, Any] = {}
    if "skrample_subschedule" in mapped:
        subschedule = mapped.pop("skrample_subschedule")
        if config.get("use_flow_sigmas", False) is True and subschedule in (scheduling.Karras, scheduling.Exponential):
            subschedule = None  # flow sigmas + karras/exponential flags: flow wins
        if subschedule:
            subschedule_props = {k: v for k, v in mapped.items() if k in _field_names(subschedule)}

    if isinstance(model, FlowModel) and not subschedule:
        modifiers.append((scheduling.FlowShift, {k: v for k, v in mapped.items() if k in _field_names(scheduling.FlowShift)}))

    invert = class_name == "MiniMaxH3Scheduler"
    if invert and "base_timesteps" not in mapped:
        mapped["base_timesteps"] = -1

    return ParsedDiffusersConfig(
        sampler=sampler,
        sampler_props=sampler_props | {k: v for k, v in mapped.items() if k in _field_names(sampler)},
        schedule=schedule,
        schedule_props={k: v for k, v in mapped.items() if k in _field_names(schedule)},
        subschedule=subschedule,
        subschedule_props=subschedule_props,
        schedule_modifiers=modifiers,
        model=model,
        invert_prediction=invert,
    )


def attr_dict(**kwargs) -> OrderedDict:
    "OrderedDict whose items are also attributes (what diffusers' BaseOutput looks like to callers)"
    od = OrderedDict(**kwargs)
    for k, v in od.items():
        setattr(od, k, v)
    return od


def as_diffusers_config(sampler: StructuredSampler, schedule: SkrampleSchedule, model: DiffusionModel) -> dict[str, Any]:
    "best-effort inverse of parse_diffusers_config"
    cfg = dataclasses.asdict(sampler)
    cfg["skrample_predictor"] = model
    if isinstance(schedule, ScheduleModifier):
        sub = schedule.all_split[1]
        if sub is not None:
            cfg["skrample_subschedule"] = type(sub)
    else:
        cfg |= dataclasses.asdict(schedule)
    renamed = {DIFFUSERS_KEY_MAP_REV[k]: v for k, v in cfg.items() if k in DIFFUSERS_KEY_MAP_REV}
    revalued = {}
    for k, v in cfg.items():
        if isinstance(v, Hashable) and (k, v) in DIFFUSERS_VALUE_MAP_REV:
            dk, dv = DIFFUSERS_VALUE_MAP_REV[(k, v)]
            revalued[dk] = dv
    return cfg | renamed | revalued


def _build_schedule(parsed: ParsedDiffusersConfig, schedule, subschedule, schedule_modifiers, schedule_props, subschedule_props, merge: MergeStrategy):
    built = (schedule or parsed.schedule)(**parsed.schedule_props | schedule_props)
    sub = subschedule or parsed.subschedule
    if sub is not None and isinstance(built, ScheduleCommon):
        built = sub(built, **parsed.subschedule_props | subschedule_props)
    if isinstance(built, (ScheduleCommon, SubSchedule, ScheduleModifier)):
        for modifier, props in merge.merge(ours=schedule_modifiers, theirs=parsed.schedule_modifiers, cmp=lambda a, b: a[0] is b[0]):
            built = modifier(base=built, **props)
    return built


def _apply_dynamic(schedule: SkrampleSchedule, steps: int, mu: float | None) -> SkrampleSchedule:
    "per-run schedule tweaks: FlowShift.shift = exp(mu); Karras/Exponential.steps = steps"
    if mu is not None and isinstance(schedule, ScheduleModifier):
        found = schedule.find_split(scheduling.FlowShift)
        if found is not None:
            before, flow, after, sub, base = found
            schedule = schedule.stack([*before, dataclasses.replace(flow, shift=math.exp(mu)), *after], sub, base)
    ramped = (scheduling.Karras, scheduling.Exponential)
    if isinstance(schedule, ramped):
        schedule = dataclasses.replace(schedule, steps=steps)
    elif isinstance(schedule, ScheduleModifier):
        mods, sub, base = schedule.all_split
        if isinstance(sub, ramped):
            schedule = schedule.stack(mods, dataclasses.replace(sub, steps=steps), base)
    return schedule


def _host_number(timestep) -> float | None:
    "python number for host scalars / CPU tensors; None for device tensors (no sync)"
    if isinstance(timestep, (int, float)):
        return timestep
    if isinstance(timestep, Tensor):
        return None if timestep.is_cuda else timestep.item()
    return float(timestep)


@dataclasses.dataclass
class SkrampleWrapperCore(abc.ABC):
    def __post_init__(self) -> None:
        self._steps: int = 50
        self._index: int = 0
        self._device: torch.device = torch.device("cpu")
        self._noise_generator: BatchTensorNoise | None = None
        self._noise_ahead = None  # (step, tensor, event, draws before, draws after): the next step's noise, drawn on the side stream
        self._noise_done = None  # event behind the latest generator launch, whichever stream it ran on (workspaces are shared)
        self._noise_side = None
        self._noise_wanted = None  # (next step, sample): drawn ahead once this call's own launch has been issued
        self._alias_stamps: list[tuple[Tensor, int, int]] = []  # (caller tensor aliased by history, data_ptr, _version)
        self._alias_auto = None  # alias_history="auto": None before a run's first call, (model_output, sample) of that call, then "alias" / "snapshot"

    # ---- copies (copy.deepcopy / pickle of a scheduler, also in the middle of a run: a plain dataclass in the reference) ------------------
    # What a copy must not inherit: pointer-bound replay entries and lowered programs (ctypes structures naming THIS object's buffers), stream
    # and event handles, weak references -- and the alias stamps, which record the addresses of the ORIGINAL's tensors: the copy's own tensors
    # are stamped afresh, so its guard keeps guarding.
    _COPY_RESET = {
        "_noise_ahead": None, "_noise_done": None, "_noise_side": None, "_noise_wanted": None, "_predrawn_noise": None, "_fast": {}, "_fast_ids": None, "_fast_hits": 0,
        "_programs": {}, "_programs_for": None, "_rk_programs": {}, "_rk_programs_for": None, "_issued_timesteps": [], "_foreign_timesteps": {},
    }  # fmt: skip

    def __getstate__(self):
        self._drain_noise_ahead()
        if self._noise_ahead is not None and self._noise_generator is not None and self._noise_generator._draws == self._noise_ahead[4]:
            self._noise_generator._draws = self._noise_ahead[3]  # (a guess drawn ahead is not part of the state: the copy draws it itself)
            self._noise_ahead = None
        state = dict(self.__dict__)
        for key, fresh in self._COPY_RESET.items():
            if key in state:
                state[key] = type(fresh)() if isinstance(fresh, (dict, list)) else fresh
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        self._alias_stamps = [(t, t.data_ptr(), t._version) for t, _ptr, _version in self._alias_stamps]
        if getattr(self, "_hist_ptrs", None):
            raws = zip(getattr(self, "_raw_samples", []), getattr(self, "_raw_outputs", []), getattr(self, "_previous", []))
            self._hist_ptrs = [
                (smp.data_ptr(), out.data_ptr(), rec.sample.data_ptr() if isinstance(rec.sample, Tensor) else 0) if old is not None else None
                for old, (smp, out, rec) in zip(self._hist_ptrs, raws)
            ]

    # ---- guard of the aliased history (alias_history=True) -------------------------------------------------------
    # The reference deep-copies every record (structured.py:113-125); this engine keeps the caller's own tensors as
    # history operands instead (0 bytes written, 4 B/element read per entry).  That is only sound while the caller
    # leaves them alone, so every aliased tensor is stamped with (data_ptr, _version) when it enters the history and
    # checked before it is read again: an in-place write (version bump), a re-bound storage, or a new network output
    # that occupies a held buffer (a graphed / compiled network with static outputs replays without bumping versions)
    # raises instead of stepping on overwritten data.
    _ALIAS_HELP = (
        "a tensor passed to an earlier step() is still a history operand of this sampler and {what}; the default wrapper "
        "aliases the caller's `sample` / `model_output` instead of copying them -- construct it with alias_history=False "
        "(snapshots both tensors per step) when buffers are reused between steps"
    )

    def _alias_check(self, model_output: Tensor, sample: Tensor) -> None:
        stamps = self._alias_stamps
        if not stamps:
            return
        for t, ptr, version in stamps:
            if t._version != version or t.data_ptr() != ptr:
                raise SkrampleHipError(self._ALIAS_HELP.format(what="was modified in place since"))
        out_ptr = model_output.data_ptr()
        for t, ptr, _ in stamps:
            if ptr == out_ptr:  # same buffer handed back as a new network output (static-output network)
                raise SkrampleHipError(self._ALIAS_HELP.format(what="its buffer now holds this step's model_output"))
            if ptr == sample.data_ptr() and t is not sample:
                raise SkrampleHipError(self._ALIAS_HELP.format(what="its buffer now holds this step's sample"))

    def _alias_now(self, model_output: Tensor, sample: Tensor) -> bool:
        """True: this call keeps the caller's tensors as history operands; False: it snapshots them.
        alias_history="auto" (the default) finds out which kind of caller it has: the run's first call snapshots and HOLDS the
        caller's two tensors, which pins their addresses -- a network that allocates its output afresh (eager PyTorch) cannot
        hand the next output back at the same address, a network with static output memory (HIP-graphed, torch.compile
        mode="reduce-overhead", an in-place `buf.copy_()` loop) does exactly that.  The second call compares and settles the
        mode for the rest of the run: aliasing (0 bytes written, guarded as before) or snapshots (+8 B/element/step)."""
        setting = self.alias_history
        if setting is True or setting is False:
            return setting
        state = self._alias_auto
        if state is None:
            self._alias_auto = (model_output, sample)
            return False
        if isinstance(state, tuple):
            static = model_output.data_ptr() == state[0].data_ptr() or sample.data_ptr() == state[1].data_ptr()
            self._alias_auto = state = "snapshot" if static else "alias"
        return state == "alias"

    def _alias_hold(self, tensors, keep: int) -> None:
        "stamp this call's caller-owned tensors; `keep` = how many of the most recent stamps stay live"
        for t in tensors:
            if isinstance(t, Tensor) and t.numel() > 0:  # (empty tensors own no buffer: their data_ptr says nothing)
                self._alias_stamps.append((t, t.data_ptr(), t._version))
        self._alias_stamps = self._alias_stamps[max(len(self._alias_stamps) - keep, 0):] if keep > 0 else []

    @property
    @abc.abstractmethod
    def sigma_space(self) -> scheduling.SigmaSpace: ...

    @property
    @abc.abstractmethod
    def schedule_np(self) -> np.ndarray: ...

    @property
    @abc.abstractmethod
    def config(self) -> OrderedDict: ...

    @property
    def schedule_pt(self) -> Tensor:
        return torch.from_numpy(self.schedule_np).to(self._device)

    @property
    def timesteps(self) -> Tensor:
        out = torch.from_numpy(self.schedule_np[:, 0]).to(self._device)
        if out.is_cuda:
            # remember what was handed out: a 0-d slice of it (`for t in scheduler.timesteps`) is then recognised by its storage
            # offset -- the index without the reference's .item() synchronisation (diffusers.py:565-567)
            issued = [ref for ref in getattr(self, "_issued_timesteps", []) if ref() is not None][-3:]
            issued.append(weakref.ref(out))
            self._issued_timesteps = issued
        return out

    def _device_timestep_index(self, timestep: Tensor) -> int | None:
        "index of a device-resident timestep that is an element of a `timesteps` tensor this scheduler handed out; else None"
        if timestep.numel() != 1:
            return None
        ptr = timestep.data_ptr()
        for ref in getattr(self, "_issued_timesteps", ()):
            base = ref()
            if base is not None and base.dtype == timestep.dtype and base.device == timestep.device:
                off = ptr - base.data_ptr()
                if 0 <= off < base.numel() * base.element_size() and off % base.element_size() == 0:
                    return off // base.element_size()
        return None

    @property
    def sigmas(self) -> Tensor:
        regular = torch.from_numpy(self.sigma_space.regularize(self.schedule_np[:, 1])).to(self._device)
        return torch.cat([regular, torch.zeros([1], device=regular.device, dtype=regular.dtype)])  # diffusers wants the trailing 0

    @property
    def init_noise_sigma(self) -> float:
        return 1

    @property
    def order(self) -> int:
        return 1

    @abc.abstractmethod
    def functional_interface(self): ...

    def functional_sample_model(self, sample, model, steps: int, include: slice = slice(None), rng=None, callback=None):
        sampler, schedule, transform = self.functional_interface()
        return sampler.sample_model(sample, model, transform, schedule, steps, include, rng, callback)

    def functional_generate_model(self, model, rng, steps: int, include: slice = slice(None), initial=None, callback=None):
        sampler, schedule, transform = self.functional_interface()
        return sampler.generate_model(model, transform, schedule, rng, steps, include, initial, callback)

    def _make_noise_generator(self, step: Step, sample: Tensor, noise_type, noise_props, generator) -> BatchTensorNoise:
        if isinstance(generator, list) and len(generator) == sample.shape[0]:
            seeds: list = generator
        elif isinstance(generator, torch.Generator) and sample.shape[0] == 1:
            seeds = [generator]
        else:
            # fallback: seed from each item's middle element (one small gather + sync, first step only)
            per_item = math.prod(sample.shape[1:])
            flat = sample.reshape(sample.shape[0], per_item)
            mids = flat[:, per_item // 2].to(torch.float64).cpu().tolist() if per_item else [0.0] * sample.shape[0]
            seeds = [int(v * 1e4 * (step.position() + 1)) for v in mids]
        from .pytorch import noise as _noise_mod

        if sample.is_cuda and noise_type is Random and _noise_mod._private_vectors[0] == 0 and all(type(v) is int for v in seeds):
            # white noise keyed by plain ints has no state but its draw counter: a run with the same seeds reuses the generator
            # object (and its device seed vector) of the previous run instead of rebuilding both
            key = (tuple(seeds), tuple(sample.shape[1:]), sample.dtype, sample.device)
            hit = getattr(self, "_white_generator", None)
            if hit is not None and hit[0] == key and not torch.cuda.is_current_stream_capturing():
                hit[1]._draws = 0
                return hit[1]
            made = BatchTensorNoise.from_batch_inputs(noise_type, unit_shape=tuple(sample.shape[1:]), seeds=seeds, props=noise_props, dtype=sample.dtype)
            self._white_generator = (key, made)
            return made
        if not sample.is_cuda:  # host-resident latents (the reference's CPU path): torch's own generators, drawn as the reference draws them
            if noise_type is Random:
                return HostRandomBatch(tuple(sample.shape[1:]), seeds, torch.float32)
            from .pytorch.host_noise import HostStructuredBatch

            return HostStructuredBatch(noise_type, tuple(sample.shape[1:]), seeds, noise_props, torch.float32)
        return BatchTensorNoise.from_batch_inputs(noise_type, unit_shape=tuple(sample.shape[1:]), seeds=seeds, props=noise_props, dtype=sample.dtype)

    def get_step_noise(self, step: Step, sample: Tensor, noise_type, noise_props, generator=None, dtype: torch.dtype | None = None, lazy_ok: bool = False):
        """noise for this step: [B, *unit].  With `lazy_ok` plain white noise comes back symbolic
        (drawn inside the step kernel); otherwise a tensor of `dtype or sample.dtype`."""
        handed = getattr(self, "_predrawn_noise", None)
        if handed is not None:  # drawn by a stage replay that then fell back to the normal path
            self._predrawn_noise = None
            if lazy_ok or not isinstance(handed, lazy.PhiloxNoise):
                return handed if lazy_ok else lazy.cast(handed, dtype or sample.dtype)
            return lazy.cast(handed.realize(torch.float32), dtype or sample.dtype)
        if isinstance(sample, Tensor) and sample.numel() == 0:  # an empty batch draws nothing (and has no items to seed generators from)
            return torch.empty(sample.shape, dtype=dtype or sample.dtype, device=sample.device)
        if self._noise_generator is None:
            self._retire_noise_generator()
            self._noise_generator = self._make_noise_generator(step, sample, noise_type, noise_props, generator)
        gen = self._noise_generator
        noise = self._take_noise_ahead(step, sample, lazy_ok)
        if noise is None:
            if self._noise_done is not None:  # the generator's workspaces were last used on the side stream
                if torch.cuda.is_current_stream_capturing():
                    # an event from outside a capture can be neither waited on nor queried inside it
                    raise SkrampleHipError("this wrapper has drawn noise ahead on its side stream: synchronize the device and call noise_quiesced() before capturing (skrample_amd.graphs.capture_sampling_loop does)")
                else:
                    torch.cuda.current_stream(sample.device).wait_event(self._noise_done)
                self._noise_done = None
            noise = gen.generate_lazy(step) if lazy_ok else gen.generate(step)
            if self._noise_side is not None and isinstance(gen, BatchTensorNoise) and isinstance(sample, Tensor) and sample.is_cuda:
                gen.used_on(torch.cuda.current_stream(sample.device))  # (workspaces may have been allocated under the side stream)
        if not lazy_ok:
            return lazy.cast(noise, dtype or sample.dtype)
        # The reference casts whatever its generator returns to the compute scale (diffusers.py:346).  The step kernel widens a tensor of the SAMPLE's dtype
        # in registers (exact, so the same values: the built-in generators draw in that dtype) and symbolic white noise is drawn inside it; only a generator
        # object that returns some third dtype -- fp32 noise beside fp16 latents under a float64 compute scale -- is cast here, as there
        if isinstance(noise, Tensor) and noise.dtype not in (sample.dtype, dtype or sample.dtype):
            return lazy.cast(noise, dtype or sample.dtype)
        return noise

    # ---- next step's noise, drawn ahead on a side stream ----------------------------------------------------------------
    # Pyramid / Offset noise is a chain of VALU-bound kernels that depends on nothing but (seeds, draw counter, step);
    # the step kernel is HBM-bound.  While step i's kernel (and, in a pipeline, the network call behind it) runs on the caller's
    # stream, the noise of step i+1 is generated on a side stream and handed over with an event.  Values and draw numbering are
    # exactly those of generating at the moment of use: a guess that does not match the next request is dropped and the counter
    # rewound.  Not under stream capture, not for Brownian (its cache makes queries order-dependent), not for white noise (drawn
    # inside the step kernel anyway).
    _AHEAD_KINDS = (Pyramid, Offset)
    # ^ generators drawn ahead when prefetch_noise=True.  Round 2 measured RKUltra-6 + Pyramid (BASELINE config 5 shard) 51.4 -> 47.9 us per
    # stage call with it; round 3's alternating A/B (tools/ab_prefetch.py) finds it 5 % slower there and only DPM-2 + Pyramid faster, so it is
    # off by default.  Colored is left out -- its plane kernels hold 134 KiB of LDS and most of the vector registers of every CU, the
    # step kernel cannot co-reside, and UniPC-3 + Colored (config 3) went 702 -> 736 us per call with it drawn ahead.

    def _drain_noise_ahead(self) -> None:
        """run boundary (reset_run): wait on the host for whatever the side stream still draws, so that the new run -- which may be
        recorded into a HIP graph, where an event from outside the capture can be neither waited on nor queried -- starts
        with no cross-stream fence pending.  One event wait per run, at most one noise generation long."""
        if self._noise_done is not None and not torch.cuda.is_current_stream_capturing():
            self._noise_done.synchronize()
            self._noise_done = None

    def noise_quiesced(self) -> None:
        "(not in the reference) tell the wrapper that the device has been synchronized: nothing drawn ahead is in flight any more"
        if self._noise_ahead is not None and self._noise_generator is not None and self._noise_generator._draws == self._noise_ahead[4]:
            self._noise_generator._draws = self._noise_ahead[3]
        self._noise_ahead = self._noise_done = None

    def _forget_issued_timesteps(self) -> None:
        "a new schedule: elements of `timesteps` tensors handed out for the previous one no longer name a step (the reference's list.index raises there)"
        self._issued_timesteps = []
        self._foreign_timesteps = {}

    def _retire_noise_generator(self) -> None:
        "drop the generator: its workspaces go back to the allocator, so whatever the side stream still runs on them must be ordered first"
        if self._noise_done is not None and torch.cuda.is_available():
            torch.cuda.current_stream(self._noise_side.device).wait_event(self._noise_done)
        self._noise_generator = None
        self._noise_ahead = self._noise_done = None

    def _noise_ahead_ok(self, sample) -> bool:
        gen = self._noise_generator
        return (
            getattr(self, "prefetch_noise", False)
            and isinstance(gen, BatchTensorNoise)
            and gen._kind in self._AHEAD_KINDS
            and isinstance(sample, Tensor)
            and sample.is_cuda
            and not torch.cuda.is_current_stream_capturing()
        )

    def _take_noise_ahead(self, step: Step, sample, lazy_ok: bool):
        ahead, self._noise_ahead = self._noise_ahead, None
        if ahead is None:
            return None
        a_step, item, event, before, after = ahead
        gen = self._noise_generator
        if gen._draws != after:  # someone drew in between: the guess no longer sits where an in-order draw would
            return None
        symbolic = not isinstance(item, Tensor)  # white noise stays symbolic (drawn inside the step kernel): only the counter moved
        if a_step != step or item.device != sample.device or torch.cuda.is_current_stream_capturing() or (symbolic and not lazy_ok):
            gen._draws = before  # as if it had never been drawn
            return None
        if not symbolic:
            main = torch.cuda.current_stream(sample.device)
            main.wait_event(event)
            item.record_stream(main)
        return item

    def _issue_noise_ahead(self) -> None:
        wanted, self._noise_wanted = self._noise_wanted, None
        if wanted is not None:
            self._draw_noise_ahead(*wanted)

    def _draw_noise_ahead(self, next_step: Step | None, sample) -> None:
        "enqueue the generation of `next_step`'s noise on the side stream (call after this step's noise exists, before its kernel)"
        if next_step is None or not self._noise_ahead_ok(sample):
            return
        gen, dev = self._noise_generator, sample.device
        if self._noise_side is None or self._noise_side.device != dev:
            self._noise_side = torch.cuda.Stream(device=dev)  # (a high-priority side stream measured 4 us per stage call WORSE on BASELINE config 5)
        side, main = self._noise_side, torch.cuda.current_stream(dev)
        if self._noise_done is None:  # the latest generation ran on the caller's stream: order the shared workspaces behind it
            fence = torch.cuda.Event()
            fence.record(main)
            side.wait_event(fence)
        before = gen._draws
        with torch.cuda.stream(side):
            item = gen.generate_lazy(next_step)  # what the wrappers ask for (lazy_ok): a tensor, or symbolic white noise
            event = None
            if isinstance(item, Tensor):
                event = torch.cuda.Event()
                event.record(side)
        gen.used_on(side)  # (workspaces allocated under the caller's stream: a later re-allocation must not recycle them under the side stream's feet)
        self._noise_ahead = (next_step, item, event, before, gen._draws)
        if event is not None:
            self._noise_done = event

    @abc.abstractmethod
    def scale_noise(self, sample: Tensor, timestep: Tensor, noise: Tensor) -> Tensor: ...

    @abc.abstractmethod
    def set_timesteps(self, num_inference_steps=None, device=None, timesteps=None, sigmas=None, mu=None) -> None: ...

    @abc.abstractmethod
    def step(self, model_output, timestep, sample, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0, generator=None, return_dict=True): ...

    def set_begin_index(self, begin_index: int = 0) -> None:
        self._index = begin_index

    def add_noise(self, original_samples: Tensor, noise: Tensor, timesteps: Tensor) -> Tensor:
        if len(timesteps) == 0:
            return original_samples
        return self.scale_noise(original_samples, timesteps[0], noise)

    def scale_model_input(self, sample: Tensor, timestep) -> Tensor:
        return sample

    def time_shift(self, mu: float, sigma: float, t: Tensor) -> Tensor:
        return math.exp(mu) / (math.exp(mu) + (1 / t - 1) ** sigma)

    # ---- shared helpers ---------------------------------------------------------------------------
    def _resolve_steps(self, num_inference_steps, timesteps, sigmas) -> int | None:
        if num_inference_steps is not None:
            return num_inference_steps
        if timesteps is not None:
            return len(timesteps)
        if sigmas is not None:
            return len(sigmas)
        return None

    def _lookup(self, table: Sequence[float], timestep, expected: int) -> int:
        value = _host_number(timestep)
        if value is None:
            # device tensor.  An element of the `timesteps` tensor this scheduler handed out is located by its storage
            # offset (no sync).  A foreign device scalar is read back once, as the reference does (diffusers.py:566) --
            # except under stream capture, where a read-back is impossible and the schedule order is authoritative.
            idx = self._device_timestep_index(timestep)
            if idx is not None:
                if not 0 <= idx < len(table):
                    raise ValueError(f"timestep index {idx} is outside the {len(table)}-step schedule")
                return idx
            if torch.cuda.is_current_stream_capturing():
                if not 0 <= expected < len(table):
                    raise ValueError(f"step {expected} is outside the {len(table)}-step schedule")
                return expected
            # a foreign device scalar: one read-back per tensor OBJECT (remembered by identity + version, never by address: a
            # recycled allocation would otherwise be mistaken for an earlier timestep)
            known = getattr(self, "_foreign_timesteps", None)
            if known is None:
                known = self._foreign_timesteps = {}
            hit = known.get(id(timestep))
            if hit is not None and hit[0]() is timestep and hit[1] == timestep._version:
                return hit[2]
            idx = table.index(timestep.item())
            if len(known) > 4096:
                known.clear()
            known[id(timestep)] = (weakref.ref(timestep), timestep._version, idx)
            return idx
        return table.index(value)

    @staticmethod
    def _finish(prev, pred, like: Tensor, return_dict: bool):
        def conv(v):
            if isinstance(v, LazyTensor):
                return v if v.dtype == like.dtype else LazyTensor(v.form, like.dtype, acc_f64=v._acc_f64)
            return lazy.cast(v, like.dtype) if isinstance(v, Tensor) else v

        prev, pred = conv(prev), conv(pred)
        return attr_dict(prev_sample=prev, pred_original_sample=pred) if return_dict else (prev, pred)


@dataclasses.dataclass
class SkrampleWrapperScheduler(SkrampleWrapperCore):
    sampler: StructuredSampler
    schedule: SkrampleSchedule
    model: DiffusionModel = NoiseModel()  # noqa: RUF009
    noise_type: type[TensorNoiseCommon] = Random
    noise_props: TensorNoiseProps | None = None
    compute_scale: torch.dtype | None = torch.float32
    allow_dynamic: bool = True
    invert_prediction: bool = False
    fake_config: dict[str, Any] = dataclasses.field(default_factory=DEFAULT_FAKE_CONFIG.copy)
    prefetch_noise: bool = False
    """(not in the reference) draw the next step's Pyramid / Offset noise ahead on a side HIP stream while this step's kernels run (same
    values, same draw numbering).  Opt-in since round 3: measured A/B/A/B in one process (tools/ab_prefetch.py) it gains 8 % for
    DPM-2 + Pyramid at 256x4x128x128 (108 vs 118 us per call) but LOSES 5 % on BASELINE config 5's shard (RKUltra-6 + Pyramid, 55.2 vs
    52.6 us per stage call: the generator's blocks take CU slots from the stage kernels on the critical path) and 37 % with Offset
    (77 vs 56 us: the cross-stream event hand-over costs more than the 19 us kernel it hides)."""
    alias_history: bool | str = "auto"
    """(not in the reference) True: keep history entries as aliases of the caller's `sample` / `model_output` tensors (0 bytes
    written; guarded: reusing a held buffer raises).  False: snapshot both tensors every step (+8 B/element/step), safe for callers
    that overwrite those buffers between steps (a HIP-graphed network with static output memory).  "auto" (default): the first
    call of a run snapshots and pins the caller's tensors, the second call sees whether the caller hands back the same memory and
    the run continues with snapshots (static buffers) or aliases (fresh tensors) -- see `_alias_now`."""

    def __post_init__(self) -> None:
        super().__post_init__()
        self._previous: list[SKSamples] = []
        self._raw_outputs: list[Tensor] = []  # model outputs / inputs of the records in _previous (for step programs)
        self._raw_samples: list[Tensor] = []
        self._programs: dict = {}
        self._programs_for = None
        self._schedule = self.schedule  # pristine copy restored by set_timesteps
        self._calls = 0
        # replayed steps of a run that walks the schedule in order (see _fast_step)
        self._fast: dict = {}  # (first index of the run, index) -> _FastEntry
        self._fast_ids = None  # the configuration objects the entries were learned under
        self._hist_ptrs: list = []  # per history record: (sample ptr, model_output ptr, record.sample ptr)
        self._hist_sigs: list = []  # per history record: (sample dtype, model_output dtype, record.sample dtype, shape, device) -- what a replayed step binds blind
        self._run_seq = False  # every call of this run so far took the next schedule index
        self._fast_hits = 0  # steps served by _fast_step (diagnostics / tests)
        self._inpaint = None  # (mask, original_samples, noise) while in-painting is set (set_inpaint)

    @classmethod
    def from_diffusers_config(
        cls,
        config,
        sampler: type[StructuredSampler] | None = None,
        schedule: type[SkrampleSchedule] | None = None,
        subschedule: type[SubSchedule] | None = None,
        schedule_modifiers: list[tuple[type[ScheduleModifier], dict[str, Any]]] = [],  # noqa: B006
        model: DiffusionModel | None = None,
        noise_type: type[TensorNoiseCommon] = Random,
        compute_scale: torch.dtype | None = torch.float32,
        sampler_props: dict[str, Any] = {},  # noqa: B006
        noise_props: TensorNoiseProps | None = None,
        schedule_props: dict[str, Any] = {},  # noqa: B006
        subschedule_props: dict[str, Any] = {},  # noqa: B006
        modifier_merge_strategy: MergeStrategy = MergeStrategy.UniqueBefore,
        allow_dynamic: bool = True,
        invert_prediction: bool | None = None,
    ) -> "SkrampleWrapperScheduler":
        parsed = parse_diffusers_config(config=config, sampler=sampler, schedule=schedule)
        return cls(
            (sampler or parsed.sampler)(**parsed.sampler_props | sampler_props),
            _build_schedule(parsed, schedule, subschedule, schedule_modifiers, schedule_props, subschedule_props, modifier_merge_strategy),
            model or parsed.model,
            noise_type=noise_type,
            noise_props=noise_props,
            compute_scale=compute_scale,
            fake_config=config.copy() if isinstance(config, dict) else dict(config.config),
            allow_dynamic=allow_dynamic,
            invert_prediction=parsed.invert_prediction if invert_prediction is None else invert_prediction,
        )

    def functional_interface(self):
        return interface.StructuredFunctionalAdapter(self.sampler), self._schedule, self.model

    @property
    def sigma_space(self) -> scheduling.SigmaSpace:
        return self.schedule.space

    @property
    def schedule_np(self) -> np.ndarray:
        return scheduling.np_schedule_lru(self.schedule, self._steps)

    @property
    def init_noise_sigma(self) -> float:
        return self.sampler.scale_input(1, Point(*self.schedule_np[0]))

    @property
    def order(self) -> int:
        return 1

    @property
    def config(self) -> OrderedDict:
        return attr_dict(**(self.fake_config | as_diffusers_config(self.sampler, self._schedule, self.model)))

    def set_begin_index(self, begin_index: int = 0) -> None:
        super().set_begin_index(begin_index)
        self._calls = 0
        self._run_seq = False
        self.fake_config["begin_index"] = begin_index

    def set_timesteps(self, num_inference_steps=None, device=None, timesteps=None, sigmas=None, mu=None) -> None:
        self._index = 0
        self._calls = 0
        self.schedule = self._schedule
        steps = self._resolve_steps(num_inference_steps, timesteps, sigmas)
        if steps is None:
            return
        self._steps = steps
        if self.allow_dynamic:
            self.schedule = _apply_dynamic(self.schedule, steps, mu)
        self._previous = []
        self._raw_outputs = []
        self._raw_samples = []
        self._hist_ptrs = []
        self._hist_sigs = []
        self._run_seq = False
        self._alias_stamps = []
        self._alias_auto = None
        self._retire_noise_generator()
        self._forget_issued_timesteps()
        self._timestep_list = None
        if device is not None:
            self._device = torch.device(device)

    def reset_run(self) -> None:
        """(not in the reference) rewind to the first step of the current schedule WITHOUT touching device state:
        history is dropped and the noise generator's draw counter restarts, but its device seed vector and the
        lowered step programs stay.  Used by skrample_amd.graphs to re-run a loop inside a HIP-graph capture."""
        self._calls = 0
        self._previous, self._raw_outputs, self._raw_samples = [], [], []
        self._hist_ptrs = []
        self._hist_sigs = []
        self._run_seq = False
        self._alias_stamps = []
        self._alias_auto = None
        self._noise_ahead = None
        self._drain_noise_ahead()
        if self._noise_generator is not None:
            self._noise_generator._draws = 0

    def _timestep_table(self) -> list[float]:
        key = (self.schedule, self._steps)
        if getattr(self, "_timestep_list", None) is None or self._timestep_key != key:
            self._timestep_list = self.schedule_np[:, 0].tolist()
            self._timestep_key = key
        return self._timestep_list

    def scale_noise(self, sample: Tensor, timestep: Tensor, noise: Tensor) -> Tensor:
        idx = self._lookup(self._timestep_table(), timestep, self._index)
        return self.sampler.add_noise(sample, noise, Point(*self.schedule_np[idx]))

    def scale_model_input(self, sample: Tensor, timestep) -> Tensor:
        idx = self._lookup(self._timestep_table(), timestep, self._index + self._calls)
        return self.sampler.scale_input(sample, Point(*self.schedule_np[idx]))

    # ---- in-painting / masked image-to-image (not in the reference) ---------------------------------------------------------------
    # The loop around a diffusers-shaped scheduler re-imposes the kept region after every step:
    #     known  = scheduler.add_noise(original_samples, noise, next timestep);   latents = mask * prev_sample + (1 - mask) * known
    # While a mask is set, step() returns prev_sample with that blend already applied, from the step's own launch
    # (lazy.evaluate_masked / skr_step_launch_masked) for the samplers whose step is one single-output launch, and from one more
    # launch behind the step for the two-output samplers (UniPC, SPC), whose state and history stay what they are.
    # Channels-last latents: when sample, model output, history, `original_samples` and `noise` all share one dense channels-last layout
    # the masked launch runs on them as they are (skr_step_launch_masked_channels_last): no copy, a channels-last prev_sample with the
    # bits of the contiguous run.  The mask is kept contiguous, in logical order.  A mixed layout takes the copying path as before.
    def set_inpaint(self, mask: Tensor, original_samples: Tensor, noise: Tensor) -> None:
        """blend every following step(): mask == 1 is generated, mask == 0 keeps `original_samples`, re-noised with `noise` to the
        level of the step's target (after the last step: `original_samples` itself).  `mask` broadcasts over leading axes of the
        latents -- (B,1,H,W), (1,1,H,W), (B,C,H,W) or (H,W) -- and is cast once to the latents' dtype (bool / uint8 accepted)."""
        for name, t in (("mask", mask), ("original_samples", original_samples), ("noise", noise)):
            if not isinstance(t, Tensor):
                raise lazy.SkrampleHipError(f"set_inpaint: {name} must be a torch tensor, not {type(t).__name__}")
        lazy._check_tensor(original_samples), lazy._check_tensor(noise)
        if original_samples.shape != noise.shape:
            raise lazy.SkrampleHipError(f"set_inpaint: original_samples {tuple(original_samples.shape)} and noise {tuple(noise.shape)} differ in shape")
        lazy.mask_layout(mask.shape, original_samples.shape)  # (refused here, not at the first step)
        mask = mask.to(device=original_samples.device, dtype=original_samples.dtype).contiguous()
        self._inpaint = (mask, original_samples, noise)

    def clear_inpaint(self) -> None:
        "steps are plain steps again (and take the replayed fast path where they did)"
        self._inpaint = None

    def _inpaint_blend(self, idx: int, steps: int):
        "the pending blend of the step at schedule index `idx`: the kept region at the noise level of index idx + 1 (Point.add_noise's algebra, host fp64)"
        mask, original, noise = self._inpaint
        if idx + 1 < steps:
            point = Point(*self.schedule_np[idx + 1])
            known = Lin.leaf(original) * float(point.alpha) + Lin.leaf(noise) * float(point.sigma)
        else:
            known = Lin.leaf(original) * 1.0
        return lazy.MaskedBlend(known, mask)

    def step(self, model_output: Tensor, timestep, sample: Tensor, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0, generator=None, return_dict: bool = True):
        inpaint = getattr(self, "_inpaint", None)
        if model_output is sample:  # one tensor in both roles: a view object per role (lazy.distinct), or the form would hold ONE operand
            model_output, sample = lazy.distinct(model_output, sample)
        # a step autograd records takes the general path: the replayed steps and step programs bind raw pointers (no autograd node)
        recorded = lazy.grad_recorded(model_output, sample, *self._raw_outputs, *self._raw_samples, *(rec.sample for rec in self._previous))
        if type(timestep) is float and self._fast_ids is not None and not recorded and inpaint is None:
            done = self._fast_step(model_output, timestep, sample, generator, return_dict)
            if done is not None:
                return done
        return self._step_general(model_output, timestep, sample, generator, return_dict, recorded, None)

    # ---- classifier-free guidance (not in the reference) --------------------------------------------------------------------------
    # The loop around a diffusers-shaped scheduler evaluates the network on a doubled batch and forms, with three tensor ops,
    #     noise_pred = uncond + guidance_scale * (cond - uncond)
    # before step() reads it.  step_guided() takes the two halves and the scale instead: for the samplers whose step is one
    # single-output launch (Euler, DPM, Adams, UniP) the three ops run inside that launch (lazy.evaluate_guided /
    # skr_step_launch_guided), which also stores the guided prediction that history, pred_original_sample and callbacks read.
    # Everything else -- the two-output samplers (UniPC, SPC), a step under set_inpaint, compute_scale=None, channels-last or strided
    # operands -- forms the prediction in one guidance-only launch and steps as ever; host-resident operands and operands that autograd
    # records form it with torch's own three lines.  Either way prev_sample and pred_original_sample have the bits of
    # step(uncond + guidance_scale * (cond - uncond), ...) on a wrapper in the same state, and calls of both kinds may be mixed in a run.
    # guidance_rescale (diffusers' rescale_noise_cfg, the line SDXL-style, v-prediction and zero-terminal-SNR pipelines put behind the three;
    # 0.0 -- diffusers' own `if guidance_rescale > 0` -- changes nothing): one statistics launch over uncond and cond
    # (skr_guidance_rescale_factor: per sample std(cond) / std(prediction)), then the same routes with the rescaled prediction
    # (skr_step_launch_guided_rescaled), which is what history and pred_original_sample read.
    def step_guided(self, model_output_uncond: Tensor, model_output_cond: Tensor, guidance_scale: float, timestep, sample: Tensor, generator=None, return_dict: bool = True,
                    guidance_rescale: float = 0.0):
        model_output_uncond, model_output_cond, sample = lazy.distinct(model_output_uncond, model_output_cond, sample)
        guidance = lazy.Guidance(model_output_uncond, model_output_cond, guidance_scale, guidance_rescale)
        recorded = lazy.grad_recorded(model_output_uncond, model_output_cond, sample, *self._raw_outputs, *self._raw_samples, *(rec.sample for rec in self._previous))
        return self._step_general(model_output_uncond, timestep, sample, generator, return_dict, recorded, guidance)

    def _step_general(self, model_output: Tensor, timestep, sample: Tensor, generator, return_dict: bool, recorded: bool, guidance):
        """the general path of step() and step_guided(): index lookup, alias guard, noise, the sampler's step, history upkeep.
        `guidance` (step_guided: a lazy.Guidance, and `model_output` is its uncond half, which stands in for the network output
        wherever only its address, dtype or layout is asked): the prediction is engine-owned -- never cloned -- and the call builds no
        step program and learns no replayed entry."""
        inpaint = getattr(self, "_inpaint", None)
        guided_call = guidance is not None
        if guided_call:
            # one launch: a sampler that settles one form through StatedSampler.sample_packed, over contiguous device tensors
            fused = (type(self.sampler).sample_packed is sampling.StatedSampler.sample_packed and inpaint is None and self.compute_scale is not None
                          and not recorded and isinstance(sample, Tensor) and sample.is_cuda and sample.is_contiguous()
                          and model_output.is_contiguous() and guidance.cond.is_contiguous())  # fmt: skip
            if not fused:
                guidance, model_output = None, lazy.guide_only(guidance)
        table = self._timestep_table()
        idx = self._lookup(table, timestep, self._index + self._calls)
        if self._calls == 0:
            self._run_seq = idx == self._index
        elif idx != self._index + self._calls:
            self._run_seq = False
        self._calls += 1
        step = Step.from_int(idx, len(table))
        keep = self.sampler.require_previous  # (a computed property: read once per step)
        aliasing = keep > 0 and self._alias_now(model_output, sample)
        if keep > 0 and not aliasing:
            sample = lazy.snapshot(sample)
            if not guided_call:  # (a guided prediction is the engine's own tensor)
                model_output = lazy.snapshot(model_output)
        elif aliasing:
            self._alias_check(model_output, sample)

        if guidance is not None:  # the guided prediction as a leaf of the sampler's form; under invert_prediction just a sign
            prediction = LazyTensor(-guidance.node() if self.invert_prediction else guidance.node(), model_output.dtype)
        else:
            prediction = LazyTensor(-Lin.leaf(model_output), model_output.dtype) if self.invert_prediction else model_output
        if self.invert_prediction and self.compute_scale is None and isinstance(model_output, Tensor) and isinstance(sample, Tensor):
            # no compute scale: the sampler runs the reference's rounded tensor ops on what it is handed (sampling/native.py), and the
            # reference hands it the negated TENSOR (diffusers.py:563-564) -- an exact op, one launch
            from .sampling import native

            if native._eligible(sample, model_output):  # (a view is copied by the tape: Tape.leaf)
                prediction = native._express(model_output, lambda o: -o, model_output)
        noise = None
        if self.sampler.require_noise:
            noise = self.get_step_noise(step, sample, self.noise_type, self.noise_props, generator, self.compute_scale, lazy_ok=True)
            self._noise_wanted = (Step.from_int(idx + 1, len(table)) if idx + 1 < len(table) else None, sample)

        # step programs (sampling/program.py): lower each distinct step once, then replay by pointer binding
        owner = (self.sampler, self.model, self.schedule, self._steps, self.compute_scale)
        if self._programs_for != owner:  # frozen dataclasses: equal configuration <=> equal coefficients
            self._programs, self._programs_for = {}, owner
            self._fast = {}
        self._fast_ids = (self.sampler, self.model, self.schedule, self.compute_scale, self.noise_type, self.noise_props, self._steps)
        roles = program.Roles(sample, model_output, noise, self._previous, self._raw_outputs, self._raw_samples)
        # (a record's `sample` is the caller's own tensor for the first step of a run and a state tensor -- UniPC's corrected, SPC's blended sample, in
        #  the compute dtype -- afterwards: a program lowered where the two coincide has ONE operand for both, so which records coincide is part of the
        #  key.  The step index alone does not say: a run may start anywhere, and a schedule may hand out one timestep several times -- Exponential over
        #  ZSNR repeats 1000.0, and a repeated value resolves to its first index, here as in the reference)
        key = (
            idx, tuple(rec.step for rec in self._previous), sample.dtype, model_output.dtype, tuple(sample.shape),
            type(noise), getattr(noise, "dtype", None), tuple(type(rec.noise) for rec in self._previous),
            tuple((rec.sample is raw, getattr(rec.sample, "dtype", None)) for rec, raw in zip(self._previous, self._raw_samples)),
        )  # fmt: skip
        record = None
        prog = self._programs.get(key) if not recorded and inpaint is None and not guided_call else False  # (a masked or guided step: no program, no tracing)
        blend = self._inpaint_blend(idx, len(table)) if inpaint is not None else None
        guide = lazy.GuidedStep(guidance) if guidance is not None else None
        if prog is not None and prog is not False:
            record = prog.run(roles, step, prediction, sample.device)
            if record is not None and self._run_seq and (self._index, idx) not in self._fast:
                self._fast_learn(prog, idx, step, table, sample, model_output, noise, keep)
        if record is None:
            tracing = prog is None and _hip.trace is None and isinstance(sample, Tensor) and sample.is_cuda
            if tracing:
                _hip.trace = []
            try:
                # (a pending blend is taken up by a sampler whose step is one single-output launch; anything else steps as ever and its result is blended below)
                one_launch = blend is not None and type(self.sampler).sample_packed is sampling.StatedSampler.sample_packed
                with lazy.compute_scale(self.compute_scale), (blend if one_launch else contextlib.nullcontext()), (guide if guide is not None else contextlib.nullcontext()):
                    record = self.sampler.sample_packed(
                        SampleInput(sample=sample, prediction=prediction, step=step, noise=noise),
                        model_transform=self.model,
                        schedule=self.schedule,
                        previous=self._previous,
                    )
                    if blend is not None and not blend.used:
                        record = dataclasses.replace(record, final=blend.settle(lift(record.final), getattr(record.final, "dtype", None)))
                if guide is not None:
                    # the record that goes into history holds the stored tensor, as the unfused run's does (negated lazily under invert_prediction)
                    model_output = guide.guided if guide.used else lazy.guide_only(guidance)
                    record = dataclasses.replace(record, prediction=LazyTensor(-Lin.leaf(model_output), model_output.dtype) if self.invert_prediction else model_output)
                if tracing:
                    built = program.StepProgram.build(_hip.trace[0], roles, record, prediction) if len(_hip.trace) == 1 else None
                    self._programs[key] = built if built is not None else False
                    if built is not None and self._run_seq and (self._index, idx) not in self._fast:
                        self._fast_learn(built, idx, step, table, sample, model_output, noise, keep)
            finally:
                if tracing:
                    _hip.trace = None
        self._previous.append(record)
        self._raw_outputs.append(model_output)
        self._raw_samples.append(sample)
        on_device = isinstance(sample, Tensor) and sample.is_cuda and isinstance(model_output, Tensor)
        self._hist_ptrs.append((sample.data_ptr(), model_output.data_ptr(), record.sample.data_ptr() if isinstance(record.sample, Tensor) else 0) if on_device else None)
        # what the pointers point at: a replayed step binds them without looking (its kernel was built for ONE dtype / size per operand), so
        # the signature of every record is compared against the one the entry was learned under (_fast_step)
        self._hist_sigs.append((sample.dtype, model_output.dtype, record.sample.dtype if isinstance(record.sample, Tensor) else None, tuple(sample.shape), sample.device,
                                _memory_format(sample), _memory_format(model_output), _memory_format(record.sample)) if on_device else None)
        self._previous = self._previous[max(len(self._previous) - keep, 0) :]
        self._raw_outputs = self._raw_outputs[max(len(self._raw_outputs) - keep, 0) :]
        self._raw_samples = self._raw_samples[max(len(self._raw_samples) - keep, 0) :]
        self._hist_ptrs = self._hist_ptrs[max(len(self._hist_ptrs) - keep, 0) :]
        self._hist_sigs = self._hist_sigs[max(len(self._hist_sigs) - keep, 0) :]
        if aliasing:
            self._alias_hold((sample, model_output), 2 * keep)
        self._issue_noise_ahead()  # behind this step's launch in host order: the step kernel is never kept waiting for it
        return self._finish(record.final, record.prediction, model_output, return_dict)


    # ---- replayed steps of an in-order run: the fast path -----------------------------------------------------------------
    # The step programs (sampling/program.py) already replace the step algebra by pointer binding; what is left per step is
    # bookkeeping -- index lookup, program key, role resolution, operand checks, alias stamps, record and history upkeep --
    # which at BASELINE config 2's size (a 7 us kernel) costs three times the kernel.  For a run that walks the schedule in
    # order, everything but the tensors is a function of (first index of the run, index): `_fast_learn` keeps, per such pair, the
    # program as a LIBRARY-side handle (skr_program_create), where each operand comes from (this call's sample / model_output, or
    # a pointer remembered with a history record) and which Philox draws feed it; `_fast_step` then validates this call's two
    # tensors, runs the alias guard, binds pointers and launches through skr_program_launch.  Anything out of the ordinary --
    # another timestep than the next one, a tensor timestep, other dtypes / shapes / devices, noise drawn ahead, a launch hook
    # (graph capture, tracing), structured noise, alias mode not settled -- returns None and the general path above runs.
    # Results are the general path's bit for bit (tests/test_step_gpu.py::test_fast_steps_equal_the_general_path).
    fast_steps = True  # class-level switch (tests compare both paths)

    def _fast_learn(self, prog, idx: int, step: Step, table, sample: Tensor, model_output: Tensor, noise, keep: int) -> None:
        key = (self._index, idx)
        self._fast[key] = False  # (decided once per key)
        if not self.fast_steps or _hip._raw_stream is None or self.invert_prediction or len(set(table)) != len(table) or not sample.is_cuda:
            return
        nprev = len(self._previous)
        srcs = []
        for role in prog.roles:
            kind = role[0]
            if kind == "x":
                srcs.append((0, 0, 0))
            elif kind == "o":
                srcs.append((1, 0, 0))
            elif kind in ("pi", "po", "px"):
                if self._hist_ptrs[role[1]] is None or (kind == "px" and self._hist_ptrs[role[1]][2] == 0):
                    return
                srcs.append((2, role[1], {"pi": 0, "po": 1, "px": 2}[kind]))
            else:
                return  # a noise TENSOR among the operands (Offset / Pyramid / Colored / Brownian): general path
        draws = []
        for role in prog.noise_roles:
            if role is None:
                draws.append(None)
            elif role == ("n",):
                draws.append(0)
            elif role[0] == "pn":
                draws.append(role[1])
            else:
                return
        uses_noise = noise is not None
        if uses_noise and not (isinstance(noise, PhiloxNoise) and type(self._noise_generator) is BatchTensorNoise and self._noise_generator._kind is Random):
            return
        final_dtype = prog.out_dtypes[prog.final_out]
        if final_dtype != model_output.dtype:
            return
        layout = prog.layout  # channels-last operands: the handle remembers the layout, and this call's two tensors must have it
        if layout is not None and (tuple(sample.stride()) != prog.strides or tuple(model_output.stride()) != prog.strides):
            return
        lib = _hip.load()
        handle = ctypes.c_void_p()
        if layout is None:
            status = lib.skr_program_create(ctypes.byref(prog.plan), prog.numel, ctypes.byref(handle))
        else:
            status = lib.skr_program_create_channels_last(ctypes.byref(prog.plan), prog.numel, ctypes.byref(_hip.StepLayoutC(*layout)), ctypes.byref(handle))
        if status != 0 or not handle.value:
            return
        entry = _FastEntry()
        weakref.finalize(entry, lib.skr_program_destroy, handle.value)
        entry.handle, entry.prog, entry.srcs, entry.draws, entry.noise = handle.value, prog, tuple(srcs), tuple(draws), uses_noise
        entry.arr = (ctypes.c_void_p * max(len(srcs), 1))()
        entry.sdt, entry.odt, entry.shape, entry.device, entry.dev_index = sample.dtype, model_output.dtype, sample.shape, sample.device, sample.device.index
        entry.step, entry.keep, entry.hist = step, keep, nprev
        entry.hist_sigs = list(self._hist_sigs)  # the records this step's history operands were lowered against
        entry.layout, entry.strides = layout, (sample.stride() if layout is not None else None)
        entry.sig = (sample.dtype, model_output.dtype, prog.out_dtypes[0] if prog.state_out is not None else sample.dtype, tuple(sample.shape), sample.device,
                     layout, layout, layout)
        entry.o0dt, entry.o1dt = prog.out_dtypes
        small = sample.numel() * sample.element_size() < (16 << 20)  # (larger results get lazy.empty_output's staggered placement)
        entry.like0, entry.like1 = small and entry.o0dt == sample.dtype, small and entry.o1dt == sample.dtype
        entry.final_out, entry.state_out, entry.pred = prog.final_out, prog.state_out, prog.pred
        entry.stream0, entry.stream1 = prog.plan.stream0, prog.plan.stream1
        entry.launch = lib.skr_program_launch
        self._fast[key] = entry

    def _fast_step(self, model_output, timestep: float, sample, generator, return_dict: bool):
        ids = self._fast_ids
        sched = self.schedule
        if (self.sampler is not ids[0] or self.model is not ids[1] or self.compute_scale is not ids[3] or self.noise_type is not ids[4]
                or self.noise_props is not ids[5] or self._steps != ids[6] or self.prefetch_noise):  # fmt: skip
            return None
        if sched is not ids[2]:
            if sched != ids[2]:
                return None
            self._fast_ids = ids = (ids[0], ids[1], sched, ids[3], ids[4], ids[5], ids[6])
        calls = self._calls
        start = self._index
        if calls and not self._run_seq:
            return None
        idx = start + calls
        entry = self._fast.get((start, idx))
        if not entry:
            return None
        table = self._timestep_list
        if table is None or self._timestep_key[0] is not sched or self._timestep_key[1] != ids[6]:
            table = self._timestep_table()
        hooks = _hip._hooks
        if idx >= len(table) or table[idx] != timestep or getattr(hooks, "indexed", None) is not None or getattr(hooks, "trace", None) is not None:
            return None
        shape = entry.shape
        if (type(sample) is not Tensor or type(model_output) is not Tensor or sample.dtype is not entry.sdt or model_output.dtype is not entry.odt
                or sample.shape != shape or model_output.shape != shape):  # fmt: skip
            return None
        strides = entry.strides  # None: a contiguous entry; else the dense channels-last strides it was learned on
        if (not sample.is_contiguous() or not model_output.is_contiguous()) if strides is None else (sample.stride() != strides or model_output.stride() != strides):
            return None
        sp, op = sample.data_ptr(), model_output.data_ptr()
        device = entry.device
        if (sp | op) & 15 or sample.device != device or model_output.device != device:
            return None
        keep = entry.keep
        hp = self._hist_ptrs
        if len(hp) != entry.hist or self._hist_sigs != entry.hist_sigs:  # (a record left by a general-path call of another shape / dtype: not this entry's history)
            return None
        stamps = self._alias_stamps
        if keep:
            if self.alias_history is not True and self._alias_auto != "alias":
                return None
            for t, ptr, version in stamps:  # the guard of the aliased history, as _alias_check
                if t._version != version or t.data_ptr() != ptr:
                    raise SkrampleHipError(self._ALIAS_HELP.format(what="was modified in place since"))
                if ptr == op:
                    raise SkrampleHipError(self._ALIAS_HELP.format(what="its buffer now holds this step's model_output"))
                if ptr == sp and t is not sample:
                    raise SkrampleHipError(self._ALIAS_HELP.format(what="its buffer now holds this step's sample"))
        previous = self._previous
        noise = None
        seeds_ptr = None
        s0, s1 = entry.stream0, entry.stream1
        if entry.noise:
            gen = self._noise_generator
            if self._noise_ahead is not None or self._noise_done is not None or getattr(self, "_predrawn_noise", None) is not None:
                return None
            if gen is None:
                gen = self._noise_generator = self._make_noise_generator(entry.step, sample, self.noise_type, self.noise_props, generator)
            if type(gen) is not BatchTensorNoise or gen._kind is not Random:
                return None
            seeds = gen._seeds
            if gen.batch_shape != shape:
                return None
            for d in entry.draws:  # history draws must be this generator's
                if d is not None and d != 0:
                    hn = previous[d].noise
                    if type(hn) is not PhiloxNoise or hn.seeds is not seeds:
                        return None
            # ---- nothing below can refuse: the draw counter may move now
            n = gen._draws
            gen._draws = n + 1
            noise = PhiloxNoise.quick(seeds, n * SUBSTREAMS, shape, device)
            seeds_ptr = gen.seeds_ptr
            d0, d1 = entry.draws
            if d0 is not None:
                s0 = noise.stream if d0 == 0 else previous[d0].noise.stream
            if d1 is not None:
                s1 = noise.stream if d1 == 0 else previous[d1].noise.stream
        arr = entry.arr
        j = 0
        for code, k, f in entry.srcs:
            arr[j] = sp if code == 0 else op if code == 1 else hp[k][f]
            j += 1
        # (results below the staggering size that share the sample's dtype: empty_like skips the shape / dtype / device argument parsing)
        out0 = torch.empty_like(sample) if entry.like0 else lazy.empty_output(shape, entry.o0dt, device, strides is not None)
        p0 = out0.data_ptr()
        if entry.o1dt is not None:
            out1 = torch.empty_like(sample) if entry.like1 else lazy.empty_output(shape, entry.o1dt, device, strides is not None)
            status = entry.launch(entry.handle, arr, p0, out1.data_ptr(), seeds_ptr, s0, s1, _hip._raw_stream(entry.dev_index))
            final = out1 if entry.final_out else out0
        else:
            status = entry.launch(entry.handle, arr, p0, None, seeds_ptr, s0, s1, _hip._raw_stream(entry.dev_index))
            final = out0
        if status:
            _hip.check(status, "skr_program_launch")
        if entry.state_out is None:
            rec_sample, rp = sample, sp
        else:
            rec_sample, rp = out0, p0
        raw_outputs, raw_samples = self._raw_outputs, self._raw_samples
        if entry.pred is None:
            prediction = model_output
        else:  # UniPC / SPC: the record's prediction is a form over this call's operands, materialised only if read
            roles = program.Roles(sample, model_output, noise, previous, raw_outputs, raw_samples)
            prediction = entry.prog.lazy_prediction(roles, shape, device)
        record = object.__new__(SKSamples)
        object.__setattr__(record, "__dict__", {"sample": rec_sample, "prediction": prediction, "step": entry.step, "noise": noise, "final": final})
        if keep:
            previous.append(record)
            raw_outputs.append(model_output)
            raw_samples.append(sample)
            hp.append((sp, op, rp))
            sigs = self._hist_sigs
            sigs.append(entry.sig)
            if len(previous) > keep:
                del previous[0], raw_outputs[0], raw_samples[0], hp[0], sigs[0]
            stamps.append((sample, sp, sample._version))
            stamps.append((model_output, op, model_output._version))
            extra = len(stamps) - 2 * keep
            if extra > 0:
                del stamps[:extra]
        self._calls = calls + 1
        if not calls:
            self._run_seq = True  # (the run's first call took the run's first index)
        self._fast_hits += 1
        if entry.pred is not None:
            return self._finish(final, prediction, model_output, return_dict)
        return attr_dict(prev_sample=final, pred_original_sample=prediction) if return_dict else (final, prediction)


def _memory_format(t):
    """what a history record's signature says of a tensor's storage: None contiguous, (channels, plane) dense channels-last, else "strided";
    "unaligned" for either dense form at an address that is no multiple of 16 -- a replayed step binds the addresses of its history blind,
    and the launch refuses such a pointer (the general path copies the operand instead)"""
    if not isinstance(t, Tensor):
        return None
    if t.is_contiguous():
        return "unaligned" if t.data_ptr() & 15 else None
    layout = lazy.layout_of(t)
    return "strided" if layout is None else "unaligned" if t.data_ptr() & 15 else layout


class _FastEntry:
    "what a replayed step of an in-order run needs besides today's tensors (SkrampleWrapperScheduler._fast_learn)"

    __slots__ = ("handle", "prog", "srcs", "draws", "noise", "arr", "sdt", "odt", "shape", "device", "dev_index", "step", "keep", "hist", "o0dt", "o1dt",
                 "final_out", "state_out", "pred", "stream0", "stream1", "launch", "like0", "like1", "hist_sigs", "sig", "layout", "strides", "__weakref__")  # fmt: skip


@dataclasses.dataclass
class RKWrapperCore(SkrampleWrapperCore):
    """Runge-Kutta samplers turned inside out: the pipeline calls `step()` once per *stage* and
    receives the next stage input (or, after the last stage, the step result)."""

    schedule: SkrampleSchedule
    sampler_order: int = traits.UnifiedModelling.order
    stochasticity: float = 0
    model: DiffusionModel = NoiseModel()  # noqa: RUF009
    derivative_transform: DiffusionModel | None = traits.UnifiedModelling.derivative_transform
    noise_type: type[TensorNoiseCommon] = Random
    noise_props: TensorNoiseProps | None = None
    compute_scale: torch.dtype | None = torch.float32
    allow_dynamic: bool = True
    invert_prediction: bool = False
    fake_config: dict[str, Any] = dataclasses.field(default_factory=DEFAULT_FAKE_CONFIG.copy)
    prefetch_noise: bool = False
    "(not in the reference) see SkrampleWrapperScheduler.prefetch_noise: the next step's noise is drawn on a side stream during this step's stages (opt-in)"
    alias_history: bool | str = "auto"
    "(not in the reference) see SkrampleWrapperScheduler.alias_history; snapshots are per stage call"

    def __post_init__(self) -> None:
        super().__post_init__()
        self._index = 0
        self._derivatives: list = []  # lazy derivative forms of the stages of the current step
        self._sample = None  # base sample of the current step (alias of the caller's tensor)
        self._last_noise = None
        self._rk_programs: dict = {}
        self._rk_programs_for = None
        self._schedule = self.schedule

    @abc.abstractmethod
    def functional_sampler(self): ...

    def functional_interface(self):
        return self.functional_sampler(), self._schedule, self.model

    @abc.abstractmethod
    def tableau(self) -> tableaux.Tableau: ...

    def adjust_steps(self, steps: int) -> int:
        return self.functional_interface()[0].adjust_steps(steps)

    @abc.abstractmethod
    def _schedule_full(self, steps: int) -> Sequence[Point]: ...

    @functools.cached_property
    def all_points(self) -> Sequence[Point]:
        "every point a stage is evaluated at, clean-end stages included"
        return self._schedule_full(self._steps)

    @functools.cached_property
    def trim_indices(self) -> tuple[int, ...]:
        "positions in all_points of the rows of schedule_np_trim (stages on the clean end are dropped: the network is never called there)"
        clean = self.schedule.point_0
        kept = tuple(i for i, p in enumerate(self.all_points) if abs(p.timestep - clean.timestep) > 1e-8 and abs(p.sigma - clean.sigma) > 1e-8)
        return kept if kept else tuple(range(len(self.all_points)))

    @functools.cached_property
    def schedule_np_trim(self) -> np.ndarray:
        "all_points without the stages that sit on the clean end"
        return np.asarray([self.all_points[i] for i in self.trim_indices], dtype=np.float64)

    @property
    def sigma_space(self) -> scheduling.SigmaSpace:
        return self.schedule.space

    @property
    def schedule_np(self) -> np.ndarray:
        return self.schedule_np_trim

    @property
    def order(self) -> int:
        return len(self.tableau().stages)

    @property
    def config(self) -> OrderedDict:
        return attr_dict(**self.fake_config)

    def set_begin_index(self, begin_index: int = 0) -> None:
        assert begin_index % self.order == 0, f"Expected {begin_index=} to be multiple of {self.order=}!"
        super().set_begin_index(begin_index)
        self.fake_config["begin_index"] = begin_index

    def set_timesteps(self, num_inference_steps=None, device=None, timesteps=None, sigmas=None, mu=None) -> None:
        self._index = 0
        self._derivatives.clear()
        self._sample = None
        self._alias_stamps = []
        self._alias_auto = None
        with contextlib.suppress(AttributeError):
            del self.all_points
        with contextlib.suppress(AttributeError):
            del self.schedule_np_trim
        with contextlib.suppress(AttributeError):
            del self.trim_indices
        self.schedule = self._schedule
        steps = self._resolve_steps(num_inference_steps, timesteps, sigmas)
        if steps is None:
            return
        self._steps = steps
        if self.allow_dynamic:
            self.schedule = _apply_dynamic(self.schedule, steps, mu)
        self._retire_noise_generator()
        self._forget_issued_timesteps()
        if device is not None:
            self._device = torch.device(device)

    def reset_run(self) -> None:
        "(not in the reference) see SkrampleWrapperScheduler.reset_run"
        self._index = 0
        self._derivatives, self._sample = [], None
        self._alias_stamps = []
        self._alias_auto = None
        self._noise_ahead = None
        self._drain_noise_ahead()
        if self._noise_generator is not None:
            self._noise_generator._draws = 0

    def _next_noise_step(self) -> Step | None:
        "the step whose noise the next draw of this run will be for (one draw per step, at its last stage)"
        nxt = self._index // self.order + 1
        return Step.from_int(nxt, self._steps) if nxt < self._steps else None

    def scale_noise(self, sample: Tensor, timestep: Tensor, noise: Tensor) -> Tensor:
        idx = self._lookup(self.schedule_np[:, 0].tolist(), timestep, 0)
        return Point(*self.schedule_np[idx]).add_noise(sample, noise)

    def _stage_form(self, sample, derivative, space: DiffusionModel, s0: Point, s1: Point, sn: Point, generator):
        """append this stage's derivative; return the lazy form of the next stage input, or of the step
        result when all stages are in (reference step_tableau_inside_out, diffusers.py:746-796)"""
        nodes, weights = self.tableau()
        self._derivatives.append(derivative)
        if self._sample is None:
            self._sample = sample
        base = lift(self._sample)
        if len(self._derivatives) == len(weights):
            noise = None
            if abs(self.stochasticity) > 1e-8:
                noise = self.get_step_noise(Step.from_int(self._index // self.order, self._steps), self._sample, self.noise_type, self.noise_props, generator, self.compute_scale, lazy_ok=True)
                self._noise_wanted = (self._next_noise_step(), self._sample)
            self._last_noise = noise
            mix = sum((d * w for d, w in zip(self._derivatives[1:], weights[1:])), self._derivatives[0] * weights[0])
            form = space.update_form(base, mix, DeltaPoint(s0, s1), noise, self.stochasticity)
            self._derivatives = []
            self._sample = None
            return form
        row = nodes[len(self._derivatives)][1]
        if row:
            mix = sum((d * w for d, w in zip(self._derivatives[1:], row[1:])), self._derivatives[0] * row[0]) / math.fsum(row)
            return space.update_form(base, mix, DeltaPoint(s0, sn))
        raise ValueError

    def step_tableau_inside_out(self, sample: Tensor, output, model_transform: DiffusionModel, S0: Point, S1: Point, SN: Point, generator=None) -> Tensor:
        """Reference-named entry (diffusers.py:746-796): feed one derivative, get the next stage input (or the step result
        once every stage is in) as a tensor in compute_scale.  `step` itself uses the lazy form and fuses it with the
        derivative conversion of the same call."""
        form = self._stage_form(sample, output if isinstance(output, lazy.Lin) else lift(output), model_transform, S0, S1, SN, generator)
        return lazy.settle(form, dtype=self.compute_scale)

    def step(self, model_output: Tensor, timestep, sample: Tensor, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0, generator=None, return_dict: bool = True):
        if model_output is sample:  # (see SkrampleWrapperScheduler.step)
            model_output, sample = lazy.distinct(model_output, sample)
        value = _host_number(timestep)
        expected = self.all_points[self._index].timestep
        if value is None:  # device timestep: checked through its position in the `timesteps` tensor we handed out (no sync)
            idx = self._device_timestep_index(timestep)
            if idx is not None:
                # `timesteps` is the TRIMMED table: element idx is stage trim_indices[idx] of all_points (a tableau with a
                # c = 1 stage before its last one -- Cash-Karp, Fehlberg, SSPRK3 ... -- drops rows ahead of the final stages)
                at = self.trim_indices[idx] if idx < len(self.trim_indices) else -1
                assert at == self._index, f"Expected timestep {expected} for step {self._index}, got element {idx} of the schedule!"
        if value is not None:
            assert value == expected, f"Expected timestep {expected} for step {self._index}, got {timestep=}!"
        aliasing = self.order > 1 and self._alias_now(model_output, sample)
        if self.order > 1 and not aliasing:
            sample, model_output = lazy.snapshot(sample), lazy.snapshot(model_output)
        elif aliasing:
            self._alias_check(model_output, sample)
            try:
                result = self._step_stage(model_output, sample, generator, return_dict)
                self._issue_noise_ahead()
                return result
            finally:
                # between stages exactly the tensors the pending state still reads are held: the step's base sample and the
                # leaves of the stored derivative forms (the caller's own network outputs only when no rounded conversion
                # produced an engine-owned derivative tensor); nothing once the step is complete
                live: dict[int, Tensor] = {}
                if self._sample is not None and isinstance(self._sample, Tensor):
                    live[id(self._sample)] = self._sample
                for form in self._derivatives:
                    if isinstance(form, Lin):
                        for leaf, _ in form.terms.values():
                            if isinstance(leaf, Tensor):
                                live[id(leaf)] = leaf
                known = {id(t): (t, ptr, ver) for t, ptr, ver in self._alias_stamps}
                self._alias_stamps = [known.get(i) or (t, t.data_ptr(), t._version) for i, t in live.items() if t.numel() > 0]
        result = self._step_stage(model_output, sample, generator, return_dict)
        self._issue_noise_ahead()
        return result

    def _step_stage(self, model_output: Tensor, sample: Tensor, generator, return_dict: bool):
        if self.compute_scale is None and isinstance(sample, Tensor) and isinstance(model_output, Tensor):
            # 16-bit tensors without a compute scale: the reference's own rounded tensor ops, recorded and replayed (sampling/native.py)
            from .sampling import native

            done = native.rk_step(self, model_output, sample, generator)
            if done is not None:
                return self._finish(done[0], done[1], model_output, return_dict)
            self._derivatives = [lift(d) if isinstance(d, Tensor) else d for d in self._derivatives]  # (a step begun in that mode goes on fused)
        # stage programs: the same lower-once / replay-by-binding scheme as SkrampleWrapperScheduler.step
        owner = (self.schedule, self._steps, self.sampler_order, self.stochasticity, self.model, self.derivative_transform, self.compute_scale, self.invert_prediction)
        if self._rk_programs_for != owner:
            self._rk_programs, self._rk_programs_for = {}, owner
        held = len(self._derivatives)
        key = (self._index, held, sample.dtype, model_output.dtype, tuple(sample.shape))
        recorded = lazy.grad_recorded(model_output, sample, self._sample, *(leaf for form in self._derivatives if isinstance(form, Lin) for leaf, _ in form.terms.values()))
        prog = self._rk_programs.get(key) if not recorded else False  # (a step autograd records is not replayed by pointer binding)
        if prog:
            done = self._replay_stage(prog, model_output, sample, generator)
            if done is not None:
                return self._finish(done[0], done[1], model_output, return_dict)

        points = [*self.all_points, Point(0, 0, 1)]
        conv = None
        if self.derivative_transform:
            space = self.derivative_transform
            convert = models.ModelConvert(self.model, self.derivative_transform)
            rounded = convert.rounded_program(points[self._index], negate_output=self.invert_prediction)
            if rounded is not None and rounded[:2] != (0, 0):
                # the reference converts in the input dtype, op by op, BEFORE widening (diffusers.py:819-834)
                conv = lazy.RoundedConversion(sample, model_output, *rounded)
                derivative = conv.node()
            else:
                output = -Lin.leaf(model_output) if self.invert_prediction else lift(model_output)
                ws, wo = convert.weights_to(points[self._index])
                derivative = lift(sample) * ws + output * wo if ws != 0 else output * wo
        else:
            derivative, space = (-Lin.leaf(model_output) if self.invert_prediction else lift(model_output)), self.model

        pending = list(self._derivatives)
        base_before = self._sample
        start_index = self._index
        self._last_noise = None
        i0 = self._index - held
        i1 = self._index + self.order - held
        form = self._stage_form(sample, derivative, space, points[i0], points[i1], points[self._index + 1], generator)
        self._index += 1

        clean = self.schedule.point_0
        synthesised = False
        while self._index < len(self.all_points) and (
            abs(self.all_points[self._index].timestep - clean.timestep) < 1e-8 or abs(self.all_points[self._index].sigma - clean.sigma) < 1e-8
        ):
            # stage on the clean end: synthesise the derivative that reproduces the pending stage input
            synthesised = True
            base = lift(sample if self._sample is None else self._sample)
            delta = DeltaPoint(points[i0], points[i1])
            synth = (form - base * space.gamma(delta)) / space.delta(delta)
            form = self._stage_form(sample, synth, space, points[i0], points[i1], points[self._index + 1], generator)
            self._index += 1

        tracing = prog is None and _hip.trace is None and isinstance(sample, Tensor) and sample.is_cuda and not synthesised
        if tracing:
            _hip.trace = []
        try:
            with lazy.compute_scale(self.compute_scale):
                if conv is not None:
                    converted, result = lazy.evaluate([conv, form], [None, model_output.dtype])
                    self._derivatives = [d.substitute(conv, converted) for d in self._derivatives]
                    pred = converted
                else:
                    result = lazy.evaluate([form], [model_output.dtype])[0]
                    pred = LazyTensor(derivative, model_output.dtype) if (self.derivative_transform or self.invert_prediction) else model_output
            if tracing:
                built = None
                if len(_hip.trace) == 1 and (conv is not None or pred is model_output):
                    built = self._build_stage_program(_hip.trace[0], sample, model_output, base_before, pending, conv is not None, finished=not self._derivatives and self._sample is None)
                self._rk_programs[(start_index, held, sample.dtype, model_output.dtype, tuple(sample.shape))] = built or False
        finally:
            if tracing:
                _hip.trace = None
        return self._finish(result, pred, model_output, return_dict)

    @staticmethod
    def _single_tensor(form):
        "the tensor if `form` is exactly 1.0 * tensor, else None"
        if isinstance(form, Lin) and len(form.terms) == 1:
            (leaf, c), = form.terms.values()
            if isinstance(leaf, Tensor) and c == 1.0:
                return leaf
        return None

    def _build_stage_program(self, entry, sample, model_output, base_before, pending, converted: bool, finished: bool):
        plan, inputs, out0, out1, seeds, numel = entry
        table: dict[int, tuple] = {}
        for j, d in enumerate(pending):
            t = self._single_tensor(d)
            if t is None:
                return None
            table[id(t)] = ("d", j)
        if base_before is not None:
            table[id(base_before)] = ("b",)
        noise = self._last_noise
        if isinstance(noise, Tensor):
            table[id(noise)] = ("n",)
        table[id(model_output)] = ("o",)
        table[id(sample)] = ("x",)
        roles = []
        for t in inputs:
            if id(t) not in table:
                return None
            roles.append(table[id(t)])
        philox = plan.noise_mode == 1
        if philox:
            if not isinstance(noise, lazy.PhiloxNoise) or noise.seeds is not seeds:
                return None
            if (converted and plan.zeta0 != 0.0) or (not converted and plan.zeta1 != 0.0):
                return None  # the draw must feed the step result (out1 when a conversion occupies out0)
        return {
            "plan": plan, "roles": roles, "dtypes": [t.dtype for t in inputs], "numel": numel, "shape": tuple(sample.shape),
            "out_dtypes": (out0.dtype, out1.dtype if out1 is not None else None), "converted": converted, "finished": finished,
            "noise": "philox" if philox else ("tensor" if isinstance(noise, Tensor) else None), "ptrs": (ctypes.c_void_p * max(len(inputs), 1))(),
            "drawn": noise is not None,  # the normal path drew for this stage even if the draw's coefficient is zero (last step: zeta = 0)
        }  # fmt: skip

    def _replay_stage(self, prog: dict, model_output: Tensor, sample: Tensor, generator):
        "fast path of step(): bind today's tensors to a recorded stage launch; None -> take the normal path"
        pending = [self._single_tensor(d) for d in self._derivatives]
        if any(t is None for t in pending):
            return None
        def fits(t, dt) -> bool:
            return isinstance(t, Tensor) and t.dtype == dt and t.numel() == prog["numel"] and t.is_contiguous() and t.data_ptr() % 16 == 0

        # every operand that exists before the draw is validated BEFORE the draw: a fallback to the normal path must not find
        # the noise generator one draw further than a run that never tried the replay
        for role, dt in zip(prog["roles"], prog["dtypes"]):
            kind = role[0]
            if kind != "n" and not fits(sample if kind == "x" else model_output if kind == "o" else self._sample if kind == "b" else pending[role[1]], dt):
                return None
        noise = None
        if prog["noise"] is not None or prog.get("drawn"):
            # (a stage whose draw has a zero coefficient still consumes the draw, as the normal path and the reference do:
            #  the generator's stream position must not depend on which path ran)
            base = sample if self._sample is None else self._sample
            noise = self.get_step_noise(Step.from_int(self._index // self.order, self._steps), base, self.noise_type, self.noise_props, generator, self.compute_scale, lazy_ok=True)
            self._noise_wanted = (self._next_noise_step(), base)
        plan = prog["plan"]
        seeds_ptr = None
        ok = True
        if prog["noise"] == "philox":
            ok = isinstance(noise, lazy.PhiloxNoise) and noise.fusable() and noise.shape == prog["shape"]
        elif prog["noise"] == "tensor":
            ok = isinstance(noise, Tensor) and all(fits(noise, dt) for role, dt in zip(prog["roles"], prog["dtypes"]) if role[0] == "n")
        if not ok:
            self._predrawn_noise = noise  # the normal path consumes this draw instead of making another
            return None
        if prog["noise"] == "philox":
            if prog["converted"]:
                plan.stream1 = noise.stream
            else:
                plan.stream0 = noise.stream
            seeds_ptr = noise.seeds.data_ptr()
        ops = []
        for role, dt in zip(prog["roles"], prog["dtypes"]):
            kind = role[0]
            ops.append(sample if kind == "x" else model_output if kind == "o" else self._sample if kind == "b" else noise if kind == "n" else pending[role[1]])
        dev = sample.device
        out0 = lazy.empty_output(prog["shape"], prog["out_dtypes"][0], dev)
        out1 = lazy.empty_output(prog["shape"], prog["out_dtypes"][1], dev) if prog["out_dtypes"][1] is not None else None
        arr = prog["ptrs"]
        for i, t in enumerate(ops):
            arr[i] = t.data_ptr()
        status = _hip.step_launch_raw(plan, arr, out0.data_ptr(), out1.data_ptr() if out1 is not None else None, seeds_ptr, prog["numel"], torch.cuda.current_stream(dev).cuda_stream)
        _hip.check(status, "skr_step_launch")
        result = out1 if prog["converted"] else out0
        pred = out0 if prog["converted"] else model_output
        if prog["finished"]:
            self._derivatives, self._sample = [], None
        else:
            self._derivatives.append(Lin.leaf(pred))
            if self._sample is None:
                self._sample = sample
        self._index += 1
        return result, pred


def _rk_from_config(cls, config, schedule, subschedule, schedule_modifiers, schedule_props, subschedule_props, merge, model, invert_prediction, **fields):
    parsed = parse_diffusers_config(config=config, sampler=None, schedule=schedule)
    return cls(
        _build_schedule(parsed, schedule, subschedule, schedule_modifiers, schedule_props, subschedule_props, merge),
        model=model or parsed.model,
        fake_config=config.copy() if isinstance(config, dict) else dict(config.config),
        invert_prediction=parsed.invert_prediction if invert_prediction is None else invert_prediction,
        **fields,
    )


@dataclasses.dataclass
class RKUltraWrapperScheduler(RKWrapperCore):
    providers: Mapping[int, Any] = functional.RKUltra.providers

    @classmethod
    def from_diffusers_config(
        cls,
        config,
        schedule: type[SkrampleSchedule] | None = None,
        sampler_order: int = functional.RKUltra.order,
        stochasticity: float = 0,
        subschedule: type[SubSchedule] | None = None,
        schedule_modifiers: list[tuple[type[ScheduleModifier], dict[str, Any]]] = [],  # noqa: B006
        providers: Mapping[int, Any] = functional.RKUltra.providers,
        model: DiffusionModel | None = None,
        noise_type: type[TensorNoiseCommon] = Random,
        derivative_transform: DiffusionModel | None = functional.RKUltra.derivative_transform,
        compute_scale: torch.dtype | None = torch.float32,
        schedule_props: dict[str, Any] = {},  # noqa: B006
        subschedule_props: dict[str, Any] = {},  # noqa: B006
        noise_props: TensorNoiseProps | None = None,
        modifier_merge_strategy: MergeStrategy = MergeStrategy.UniqueBefore,
        allow_dynamic: bool = True,
        invert_prediction: bool | None = None,
    ) -> "RKUltraWrapperScheduler":
        return _rk_from_config(
            cls, config, schedule, subschedule, schedule_modifiers, schedule_props, subschedule_props, modifier_merge_strategy, model, invert_prediction,
            sampler_order=sampler_order, stochasticity=stochasticity, providers=providers, derivative_transform=derivative_transform,
            noise_type=noise_type, noise_props=noise_props, compute_scale=compute_scale, allow_dynamic=allow_dynamic,
        )  # fmt: skip

    def functional_sampler(self) -> functional.RKUltra:
        return functional.RKUltra(order=self.sampler_order, stochasticity=self.stochasticity, derivative_transform=self.derivative_transform, providers=MappingProxyType(dict(self.providers)))

    def tableau(self) -> tableaux.Tableau:
        return self.functional_sampler().tableau()

    def _schedule_full(self, steps: int) -> Sequence[Point]:
        "stage times are c_j fractions of each step: read the points straight off the schedule"
        nodes = self.tableau().stages
        seen: list[Point] = []
        for n in range(steps):
            t0, t1 = Step.from_int(n, steps)
            seen.extend(self.schedule.ipoints([t0 + c * (t1 - t0) for c, _ in nodes]))
        return seen


@dataclasses.dataclass
class DynasauRKWrapperScheduler(RKWrapperCore):
    @classmethod
    def from_diffusers_config(
        cls,
        config,
        schedule: type[SkrampleSchedule] | None = None,
        sampler_order: int = functional.RKUltra.order,
        stochasticity: float = 0,
        subschedule: type[SubSchedule] | None = None,
        schedule_modifiers: list[tuple[type[ScheduleModifier], dict[str, Any]]] = [],  # noqa: B006
        model: DiffusionModel | None = None,
        noise_type: type[TensorNoiseCommon] = Random,
        derivative_transform: DiffusionModel | None = functional.RKUltra.derivative_transform,
        compute_scale: torch.dtype | None = torch.float32,
        schedule_props: dict[str, Any] = {},  # noqa: B006
        subschedule_props: dict[str, Any] = {},  # noqa: B006
        noise_props: TensorNoiseProps | None = None,
        modifier_merge_strategy: MergeStrategy = MergeStrategy.UniqueBefore,
        allow_dynamic: bool = True,
        invert_prediction: bool | None = None,
    ) -> "DynasauRKWrapperScheduler":
        return _rk_from_config(
            cls, config, schedule, subschedule, schedule_modifiers, schedule_props, subschedule_props, modifier_merge_strategy, model, invert_prediction,
            sampler_order=sampler_order, stochasticity=stochasticity, derivative_transform=derivative_transform,
            noise_type=noise_type, noise_props=noise_props, compute_scale=compute_scale, allow_dynamic=allow_dynamic,
        )  # fmt: skip

    def functional_sampler(self) -> functional.DynasauRK:
        return functional.DynasauRK(order=self.sampler_order, stochasticity=self.stochasticity, derivative_transform=self.derivative_transform)

    def tableau(self) -> tableaux.Tableau:
        fs = self.functional_sampler()
        stages = len(fs.tableau(Step(0, 1)).stages)
        return fs.tableau(Step.from_int(self._index // stages, self._steps))

    def _schedule_full(self, steps: int) -> Sequence[Point]:
        """The points the functional sampler itself calls the network at (reference diffusers.py:1029-1042): a scalar run over
        `functional_interface()`'s schedule -- the PRISTINE one, so a Karras / Exponential sub-schedule keeps its constructor's `steps`
        here while RKUltra's table reads the re-targeted one -- with the sampler's own rule of not calling the network at t = 0 or
        sigma = 0, which makes the count fall short and the assertion fire for schedules whose last stage lands there."""
        seen: list[Point] = []

        def record(x: float, t: float, s: float, a: float) -> float:
            seen.append(Point(t, s, a))
            return x

        self.functional_sample_model(1, record, steps)
        assert len(seen) == self.order * steps
        return seen
