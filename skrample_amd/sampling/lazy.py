"""Lazy linear forms over device tensors -- the bridge between the fp64 host math and the fused
HIP step kernel.

Every solver step of every sampler is a linear combination  sum_k c_k * T_k  of a handful of
same-shaped tensors (SURVEY.md "three facts" #2).  The samplers in this package therefore never
execute tensor arithmetic: they run their (scalar, fp64) algebra on `Lin` objects, which only
accumulate coefficients, and `evaluate()` turns the final one or two forms into ONE launch of
`skr_step_launch` (include/skrample_hip.h).  Plain Python numbers flow through the same code
unchanged -- that is host scalar logic (schedule dry-runs, coefficient tests).

Operand residency decides where a form is evaluated, never availability of the library:
  * HIP-device tensors  -> the fused kernel, always (a missing libskrample_hip.so raises; nothing falls back);
  * host-resident operands (CPU torch tensors, numpy arrays -- the reference's generic `T`, common.py:11-17, and
    BASELINE config 1 "on CPU torch") -> `_host_evaluate`, the same  sum_k c_k * T_k  in plain torch on the host.
    Device tensors can never reach it (mixed residency is refused).
"""

from __future__ import annotations

import contextvars
import ctypes
import math
import os
from typing import Any, Sequence

import torch

from .. import _hip
from .._hip import SkrampleHipError

NUMBER = (int, float)

# dtype in which *derived, persisted* state is kept (UniPC's corrected sample) and, when float64,
# the accumulator precision.  The scheduler wrapper sets it from `compute_scale`.
_compute_dtype: contextvars.ContextVar = contextvars.ContextVar("skr_compute_dtype", default=None)


class compute_scale:
    "context manager: `with compute_scale(torch.float32): sampler.sample_packed(...)`"

    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        self.token = _compute_dtype.set(self.dtype)
        return self

    def __exit__(self, *exc):
        _compute_dtype.reset(self.token)


class PhiloxNoise:
    """Symbolic standard-normal tensor N(seeds[b], stream) of a given shape: drawn inside the step
    kernel (0 bytes of HBM traffic), or realised into a tensor on demand.
    Element e of sample b comes from Philox4x32-10 block e//4, lane e%4, key = seeds[b],
    counter high words = stream (oracle/skr_oracle/noise.py::philox_normal)."""

    __slots__ = ("seeds", "stream", "shape", "device", "_cache")

    def __init__(self, seeds: torch.Tensor, stream: int, shape: Sequence[int], device: torch.device):
        self.seeds, self.stream, self.shape, self.device = seeds, int(stream), tuple(shape), device
        self._cache: dict | None = None

    @classmethod
    def quick(cls, seeds: torch.Tensor, stream: int, shape: tuple, device: torch.device) -> "PhiloxNoise":
        "the same object without argument conversion (the replayed-step fast path makes one per step)"
        self = cls.__new__(cls)
        self.seeds, self.stream, self.shape, self.device, self._cache = seeds, stream, shape, device, None
        return self

    @property
    def sample_numel(self) -> int:
        return math.prod(self.shape[1:]) if len(self.shape) > 1 else (self.shape[0] if self.shape else 1)

    def numel(self) -> int:
        return math.prod(self.shape)

    def realize(self, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        "materialise through skr_noise_random (any shape)"
        if self._cache is None:
            self._cache = {}
        if dtype not in self._cache:
            out = torch.empty(self.shape, dtype=dtype, device=self.device)
            lib = _hip.load()
            batch = self.shape[0] if len(self.shape) > 1 else 1
            _hip.check(
                lib.skr_noise_random(out.data_ptr(), _hip.DTYPE_CODE[dtype], self.seeds.data_ptr(), self.stream, batch, self.numel() // max(batch, 1), _hip.current_stream_ptr(self.device)),
                "skr_noise_random",
            )
            self._cache[dtype] = out
        return self._cache[dtype]

    def fusable(self) -> bool:
        return len(self.shape) > 1 and self.sample_numel % 8 == 0 and self.numel() > 0


class Node:
    "leaf standing for the value of another form that is stored as the first output of the same launch"

    __slots__ = ("form",)

    def __init__(self, form):
        self.form = form


class RoundedConversion:
    """out0 of a launch defined not as a linear form but as the reference's *op-by-op rounded*
    conversion from_x(s, to_x(s, o)) in the tensors' own dtype (include/skrample_hip.h, convert_*).
    Used by the Runge-Kutta wrapper, where the reference converts before widening to compute_scale."""

    def __init__(self, sample: torch.Tensor, output: torch.Tensor, to_kind: int, from_kind: int, k: Sequence[float]):
        _check_tensor(sample), _check_tensor(output)
        if sample.dtype != output.dtype or sample.shape != output.shape:
            raise SkrampleHipError("rounded conversion needs sample and output of one dtype and shape")
        self.sample, self.output, self.to_kind, self.from_kind, self.k = sample, output, int(to_kind), int(from_kind), [float(v) for v in k]
        self.shape, self.device, self.dtype = tuple(sample.shape), sample.device, sample.dtype

    def node(self) -> "Lin":
        n = Node(self)
        return Lin({id(n): (n, 1.0)}, self.shape, self.device)

    def expanded(self, keep=None):
        return self


def check_guidance_numbers(scale, rescale=0.0) -> None:
    "what a guidance scale and a guidance_rescale must be, wherever they enter (Guidance, CapturedLoop.retarget): one set of messages"
    if isinstance(scale, bool) or not isinstance(scale, NUMBER):
        raise SkrampleHipError(f"the guidance scale is a Python number, not {type(scale).__name__}")
    if isinstance(rescale, bool) or not isinstance(rescale, NUMBER):
        raise SkrampleHipError(f"guidance_rescale is a Python number, not {type(rescale).__name__}")
    if not rescale >= 0.0:
        raise SkrampleHipError(f"guidance_rescale must be >= 0, not {rescale}")


class Guidance:
    """The classifier-free-guidance prediction  uncond + scale * (cond - uncond)  as ONE leaf of a step's form: its value is torch's --
    three tensor ops, each rounded in the tensors' dtype, the Python scalar kept in the op-math type -- and `evaluate_guided` computes
    it inside the launch that consumes it (include/skrample_hip.h, skr_step_launch_guided).  `node()` is a `Lin` leaf, as
    `RoundedConversion.node()` is: a sampler's algebra carries it wherever the prediction stands, with whatever coefficient it gets.
    `rescale` (guidance_rescale; 0.0: nothing changes): the prediction is diffusers' rescale_noise_cfg of it -- the four lines in
    `torch_lines` -- with dim 0 the sample; on the HIP device the two per-sample stds are one statistics launch (`factor`,
    skr_guidance_rescale_factor) and the elementwise part runs inside the consuming launch (skr_step_launch_guided_rescaled)."""

    def __init__(self, uncond: torch.Tensor, cond: torch.Tensor, scale: float, rescale: float = 0.0):
        if not isinstance(uncond, torch.Tensor) or not isinstance(cond, torch.Tensor):
            raise SkrampleHipError(f"guidance takes two torch tensors, not {type(uncond).__name__} and {type(cond).__name__}")
        _check_tensor(uncond), _check_tensor(cond)
        if uncond.dtype != cond.dtype or uncond.shape != cond.shape or uncond.device != cond.device:
            raise SkrampleHipError(
                f"guidance needs uncond and cond of one dtype, shape and device: {uncond.dtype} {tuple(uncond.shape)} {uncond.device} vs {cond.dtype} {tuple(cond.shape)} {cond.device}"
            )
        check_guidance_numbers(scale, rescale)
        if rescale != 0.0 and (uncond.ndim < 2 or uncond.numel() // max(uncond.shape[0], 1) < 2):
            raise SkrampleHipError(f"rescaled guidance takes the std of every sample: it needs tensors of ndim >= 2 (dim 0 the sample) with at least 2 elements per sample, not {tuple(uncond.shape)}")
        self.uncond, self.cond, self.scale, self.rescale = uncond, cond, float(scale), float(rescale)
        self.shape, self.device, self.dtype = tuple(uncond.shape), uncond.device, uncond.dtype

    def node(self) -> "Lin":
        n = Node(self)
        return Lin({id(n): (n, 1.0)}, self.shape, self.device)

    def expanded(self, keep=None):
        return self

    def torch_lines(self) -> torch.Tensor:
        "the pipeline's three lines -- and, rescaled, the four of rescale_noise_cfg -- by torch itself (host-resident operands; operands that autograd records)"
        d = self.cond - self.uncond
        m = self.scale * d
        p = self.uncond + m
        if self.rescale != 0.0:
            c, phi = self.cond, self.rescale
            std_text = c.std(dim=list(range(1, c.ndim)), keepdim=True)
            std_cfg = p.std(dim=list(range(1, p.ndim)), keepdim=True)
            resc = p * (std_text / std_cfg)
            p = phi * resc + (1 - phi) * p
        return p

    def factor(self) -> torch.Tensor:
        """std(cond) / std(p) per sample as a tensor of the operands' dtype and shape (B, 1, ...): one statistics launch
        (skr_guidance_rescale_factor), summed in storage order -- a dense channels-last sample is one contiguous span, so such operands
        are read as they stand; torch's own two stds and division for host-resident operands and operands that autograd records."""
        u, c = self.uncond, self.cond
        if len(self.shape) < 2:
            raise SkrampleHipError(f"rescaled guidance needs tensors of ndim >= 2 (dim 0 the sample), not {self.shape}")
        if is_host(self.device) or grad_recorded(u, c):
            p = u + self.scale * (c - u)
            return c.std(dim=list(range(1, c.ndim)), keepdim=True) / p.std(dim=list(range(1, p.ndim)), keepdim=True)
        prepare = _prepare_keeping_layout if in_place_layout((u, c), self.shape) is not None else _prepare_tensor
        return self.device_factor(prepare(u), prepare(c))

    def device_factor(self, u: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
        "`factor` over device operands a launch takes as they stand (16-byte aligned; contiguous or dense channels-last, both alike)"
        factor = torch.empty((self.shape[0],) + (1,) * (len(self.shape) - 1), dtype=self.dtype, device=self.device)
        if u.numel():
            _hip.launch_guidance_factor(u, c, self.scale, u.numel() // self.shape[0], factor)
        return factor


def _check_tensor(t: torch.Tensor) -> torch.Tensor:
    if t.device.type not in ("cuda", "cpu"):
        _hip.require_device(t, "sampler operand")
    if t.dtype not in _hip.DTYPE_CODE:
        raise SkrampleHipError(f"unsupported tensor dtype {t.dtype}; the engine handles bf16/f16/f32/f64")
    return t


# ---- host-resident operands ---------------------------------------------------------------------------------------
NUMPY = "numpy"  # `device` of forms built from numpy arrays: evaluated on the host, results handed back as ndarrays
_numpy_views: dict[int, tuple] = {}  # id(ndarray) -> (ndarray, torch view): one leaf per array however often it is lifted


def is_host(device) -> bool:
    return device == NUMPY or (isinstance(device, torch.device) and device.type == "cpu")


def _from_numpy(x) -> torch.Tensor:
    import numpy as np

    hit = _numpy_views.get(id(x))
    if hit is not None and hit[0] is x:
        # a C-contiguous array is SHARED with its tensor.  A strided one (a slice, a reversed or transposed view) was copied, and the caller
        # may have refilled it since: its copy stands only while it still holds the array's numbers.  (It cannot simply go unremembered:
        # a step lifts one array several times, and the same tensor must come back each time for the form to hold ONE operand)
        held = hit[1].numpy()
        if np.may_share_memory(held, x) or np.array_equal(held.reshape(-1).view(np.uint8), np.ascontiguousarray(x).reshape(-1).view(np.uint8)):
            return hit[1]
    t = torch.from_numpy(np.ascontiguousarray(x))
    if t.dtype not in _hip.DTYPE_CODE:
        raise SkrampleHipError(f"unsupported array dtype {x.dtype}; float16/32/64 arrays are handled")
    if len(_numpy_views) >= 64:
        _numpy_views.pop(next(iter(_numpy_views)))
    _numpy_views[id(x)] = (x, t)
    return t


class Lin:
    "sum_k coef_k * leaf_k ; leaves are HIP tensors, PhiloxNoise or Node objects"

    __slots__ = ("terms", "shape", "device")
    __array_priority__ = 1000

    def __init__(self, terms: dict, shape, device):
        self.terms = terms  # id(leaf) -> (leaf, coef)
        self.shape = tuple(shape)
        self.device = device

    # ---- construction ---------------------------------------------------------------------------
    @staticmethod
    def leaf(obj) -> "Lin":
        if isinstance(obj, torch.Tensor):
            _check_tensor(obj)
            return Lin({id(obj): (obj, 1.0)}, obj.shape, obj.device)
        if isinstance(obj, PhiloxNoise):
            return Lin({id(obj): (obj, 1.0)}, obj.shape, obj.device)
        raise TypeError(type(obj))

    def node(self) -> "Lin":
        "this form, to be stored by the launch that also evaluates its consumers"
        n = Node(self)
        return Lin({id(n): (n, 1.0)}, self.shape, self.device)

    # ---- algebra --------------------------------------------------------------------------------
    def _scaled(self, k: float) -> "Lin":
        return Lin({i: (leaf, c * k) for i, (leaf, c) in self.terms.items()}, self.shape, self.device)

    def _plus(self, other, sign: float) -> "Lin":
        if isinstance(other, NUMBER):
            if other == 0:
                return self
            raise SkrampleHipError("adding a non-zero scalar to a tensor form is not a sampler operation")
        other = lift(other)
        if other.shape != self.shape:
            raise SkrampleHipError(f"shape mismatch in sampler operands: {self.shape} vs {other.shape}")
        terms = dict(self.terms)
        for i, (leaf, c) in other.terms.items():
            if i in terms:
                terms[i] = (leaf, terms[i][1] + sign * c)
            else:
                terms[i] = (leaf, sign * c)
        return Lin(terms, self.shape, self.device)

    def __add__(self, other):
        return self._plus(other, 1.0)

    __radd__ = __add__

    def __sub__(self, other):
        return self._plus(other, -1.0)

    def __rsub__(self, other):
        return self._scaled(-1.0)._plus(other, 1.0)

    def __neg__(self):
        return self._scaled(-1.0)

    def __mul__(self, k):
        if not isinstance(k, NUMBER):
            if hasattr(k, "item") and getattr(k, "ndim", 1) == 0:
                k = float(k.item())
            else:
                raise SkrampleHipError("products of two tensors are not part of any solver step")
        return self._scaled(float(k))

    __rmul__ = __mul__

    def __truediv__(self, k):
        if not isinstance(k, NUMBER):
            raise SkrampleHipError("division by a tensor is not part of any solver step")
        if k == 0:
            raise ZeroDivisionError("tensor form divided by zero")
        return Lin({i: (leaf, c / k) for i, (leaf, c) in self.terms.items()}, self.shape, self.device)

    # ---- expansion ------------------------------------------------------------------------------
    def expanded(self, keep: "Lin | None" = None) -> "Lin":
        "substitute every Node leaf whose form is not `keep`"
        if not any(isinstance(leaf, Node) and leaf.form is not keep for leaf, _ in self.terms.values()):
            return self
        acc = Lin({}, self.shape, self.device)
        for i, (leaf, c) in self.terms.items():
            if isinstance(leaf, Node) and leaf.form is not keep:
                if isinstance(leaf.form, RoundedConversion):
                    raise SkrampleHipError("a rounded conversion can only be consumed by the launch that stores it")
                if isinstance(leaf.form, Guidance):
                    raise SkrampleHipError("a guided prediction is not a linear form: it is settled by evaluate_guided()")
                acc = acc._plus(leaf.form.expanded(keep)._scaled(c), 1.0)
            else:
                acc = acc._plus(Lin({i: (leaf, c)}, self.shape, self.device), 1.0)
        return acc

    def numel(self) -> int:
        return math.prod(self.shape)

    def substitute(self, target, tensor: torch.Tensor) -> "Lin":
        "replace every Node leaf of `target` (a form or RoundedConversion) by the tensor that now holds its value"
        if not any(isinstance(leaf, Node) and leaf.form is target for leaf, _ in self.terms.values()):
            return self
        acc = Lin({}, self.shape, self.device)
        for i, (leaf, c) in self.terms.items():
            piece = Lin.leaf(tensor)._scaled(c) if isinstance(leaf, Node) and leaf.form is target else Lin({i: (leaf, c)}, self.shape, self.device)
            acc = acc._plus(piece, 1.0)
        return acc


def lift(x):
    "number -> number, HIP tensor / PhiloxNoise / Lin -> Lin, anything else -> refused"
    if isinstance(x, Lin):
        return x
    if isinstance(x, NUMBER):
        return x
    if isinstance(x, torch.Tensor):
        if x.ndim == 0 and not x.is_cuda:  # numpy/torch scalars that slipped through float()
            return float(x.item())
        return Lin.leaf(x)
    if isinstance(x, PhiloxNoise):
        return Lin.leaf(x)
    if isinstance(x, LazyTensor):
        return x.form
    if hasattr(x, "dtype") and hasattr(x, "shape") and getattr(x, "shape", None) == ():
        return float(x)
    if type(x).__module__ == "numpy" and hasattr(x, "__array_interface__"):
        t = _from_numpy(x)
        return Lin({id(t): (t, 1.0)}, t.shape, NUMPY)
    raise SkrampleHipError(
        f"operand of type {type(x).__name__} is not supported: skrample_amd computes on torch tensors (HIP device: fused "
        "kernels; CPU: host executor), numpy arrays and host scalars"
    )


# ---------------------------------------------------------------------------------------------------
# evaluation: <= 2 outputs, one kernel launch
# ---------------------------------------------------------------------------------------------------
def _default_dtype(form: Lin) -> torch.dtype:
    for leaf, _ in form.expanded().terms.values():
        if isinstance(leaf, torch.Tensor):
            return leaf.dtype
    return torch.float32


# ---- HBM-aware output placement ---------------------------------------------------------------------------
# A step reads 4-5 equally sized tensors at the same offsets.  torch's caching allocator hands out large blocks
# at 2 MiB multiples, so all streams then start on the same HBM channel/bank phase and collide; shifting the
# tensors this engine allocates (every step result, i.e. the next step's `sample` and history `sample`) by odd
# multiples of 4 KiB takes ~3.5 % off the fused DPM-2 step (tools/tune/tune_step.hip, "mask=21" runs).
_STAGGER_SLOTS = int(os.environ.get("SKR_STAGGER_SLOTS", "8"))  # (environment overrides: tuning experiments only)
_STAGGER_BYTES = int(os.environ.get("SKR_STAGGER_BYTES", "8192"))
_stagger_next = 0


_ITEMSIZE = {torch.bfloat16: 2, torch.float16: 2, torch.float32: 4, torch.float64: 8}
_strides_cache: dict = {}


def _channels_last_strides(shape) -> tuple:
    "strides of dense channels-last storage (torch.channels_last / channels_last_3d): axis 1 innermost, the other axes in order"
    strides, acc = [0] * len(shape), shape[1]
    strides[1] = 1
    for axis in range(len(shape) - 1, 1, -1):
        strides[axis] = acc
        acc *= shape[axis]
    strides[0] = acc
    return tuple(strides)


def empty_output(shape, dtype: torch.dtype, device: torch.device, channels_last: bool = False) -> torch.Tensor:
    """uninitialised result tensor, contiguous or in channels-last storage, whose start is shifted by 4 KiB + k*8 KiB (k cycles) inside
    its allocation"""
    global _stagger_next
    shape = tuple(shape)
    numel = math.prod(shape)
    item = _ITEMSIZE.get(dtype, 4)
    small = numel * item < (16 << 20)  # small tensors are launch/host-bound and live in L2 / MALL anyway
    if small and not channels_last:
        return torch.empty(shape, dtype=dtype, device=device)
    strides = _strides_cache.get((shape, channels_last))
    if strides is None:
        if channels_last:
            strides = _channels_last_strides(shape)
        else:
            acc, rev = 1, []
            for d in reversed(shape):
                rev.append(acc)
                acc *= d
            strides = tuple(reversed(rev))
        _strides_cache[shape, channels_last] = strides
    if small:
        return torch.empty_strided(shape, strides, dtype=dtype, device=device)
    k = _stagger_next
    _stagger_next = (k + 1) % _STAGGER_SLOTS
    flat = torch.empty(numel + (4096 + _STAGGER_SLOTS * _STAGGER_BYTES) // item, dtype=dtype, device=device)
    return flat.as_strided(shape, strides, (4096 + k * _STAGGER_BYTES) // item)


def _prepare_tensor(t: torch.Tensor) -> torch.Tensor:
    if not t.is_contiguous():
        t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone()
    return t


# ---- channels-last operands ------------------------------------------------------------------------------------------------
# A step is elementwise, so over operands that all share one dense layout it runs on the storage order as it stands
# (skr_step_launch_channels_last: only the fused Philox draw looks at the layout; skr_step_launch_masked_channels_last for masked
# steps, whose mask index looks at it too).  False restores the contiguous copies of every non-contiguous operand (tests,
# tools/bench_channels_last.py and tools/bench_masked_channels_last.py compare the two).
channels_last = True


_layout_cache: dict = {}  # (shape, strides) -> layout_of's answer: the walk below costs microseconds, and every step of a loop asks for the same few


def layout_of(t: torch.Tensor) -> "tuple[int, int] | None":
    """(channels, plane) of a dense channels-last tensor (torch.channels_last / channels_last_3d: axis 1 innermost in storage, the
    other axes in order), None for everything else -- contiguous tensors, rank < 3, C == 1 or a single-position plane (their storage
    order is the logical one), slices, other permutations."""
    key = (t.shape, t.stride())
    try:
        return _layout_cache[key]
    except KeyError:
        if len(_layout_cache) >= 256:
            _layout_cache.clear()
        found = _layout_cache[key] = _layout_from(*key)
        return found


def _layout_from(shape, strides) -> "tuple[int, int] | None":
    ndim = len(shape)
    if ndim < 3:
        return None
    channels, plane = shape[1], 1
    for d in shape[2:]:
        plane *= d
    if channels <= 1 or plane <= 1 or shape[0] < 1:
        return None
    want = _channels_last_strides(shape)
    for axis in range(ndim):
        if shape[axis] != 1 and strides[axis] != want[axis]:
            return None
    return channels, plane


def shared_layout(tensors, shape) -> "tuple[int, int] | None":
    "the layout every tensor of `tensors` has (all of `shape`, all dense channels-last), or None"
    layout, shape, first = None, tuple(shape), None
    for t in tensors:
        if tuple(t.shape) != shape:
            return None
        strides = t.stride()
        if strides != first:  # (the same strides as the tensor before: the same answer)
            layout = layout_of(t)
            if layout is None:
                return None
            first = strides
    return layout


def snapshot(t: torch.Tensor) -> torch.Tensor:
    """the engine's own copy of a caller's tensor: in the caller's layout when that is contiguous or dense channels-last (a launch takes
    it as it is), contiguous for every other view -- `clone()` alone would hand the strides of a permuted operand on to the copy, and to
    whatever is returned of it"""
    return t.clone() if t.is_contiguous() or layout_of(t) is not None else t.clone(memory_format=torch.contiguous_format)


def distinct(*operands) -> tuple:
    """the operands of one call, with a tensor that the caller passed in more than one role (`model_output is sample`, `uncond is cond`)
    seen through a view object of its own per role -- no copy.  Forms merge their leaves by identity, so one object in two roles would
    collapse into one operand with the summed coefficient, whose rounding is not that of the same numbers in two tensors."""
    seen, out = set(), []
    for t in operands:
        if isinstance(t, torch.Tensor) and id(t) in seen:
            t = t[...]
        seen.add(id(t))
        out.append(t)
    return tuple(out)


def _prepare_keeping_layout(t: torch.Tensor) -> torch.Tensor:
    "a channels-last operand as it is; an alignment clone keeps the format"
    if t.data_ptr() % 16:
        t = t.clone(memory_format=torch.preserve_format)
    return t


def in_place_layout(tensors, shape, allowed: bool = True) -> "tuple[int, int] | None":
    """Does a launch over `tensors` run in place on channels-last storage, and in which layout: (channels, plane) when the caller allows
    it (nothing grad-recorded), `channels_last` is on, no `_hip.indexed` hook is installed and every tensor has `shape` in one dense
    channels-last layout; None: the contiguous route."""
    if not (allowed and channels_last and _hip.indexed is None):
        return None
    return shared_layout(tensors, shape)


def evaluate(forms: Sequence[Lin], dtypes: Sequence[torch.dtype | None], acc_f64: bool | None = None) -> list[torch.Tensor]:
    """Materialise one or two forms in a single fused launch.  forms[1] may reference forms[0]
    through a Node leaf (then out1 = chain*out0 + ...)."""
    if not 1 <= len(forms) <= 2:
        raise SkrampleHipError("evaluate() takes one or two forms")
    conv = forms[0] if isinstance(forms[0], RoundedConversion) else None
    if conv is not None:
        if len(forms) != 2:
            raise SkrampleHipError("a rounded conversion is stored alongside the form that consumes it")
        dtypes = [conv.dtype, dtypes[1]]
        # the two operands lead group A; their coef0 is ignored by the kernel
        forms = [conv, forms[1]]
        f0 = Lin({id(conv.sample): (conv.sample, 0.0), id(conv.output): (conv.output, 0.0)}, conv.shape, conv.device)
    else:
        f0 = forms[0].expanded()
    f1 = forms[1].expanded(keep=forms[0]) if len(forms) == 2 else None
    shape, device = f0.shape, f0.device
    numel = math.prod(shape)
    out_dtypes = [d if d is not None else (f.dtype if isinstance(f, RoundedConversion) else _default_dtype(f)) for d, f in zip(dtypes, forms)]
    if is_host(device) or (f1 is not None and is_host(f1.device)):
        return _host_evaluate(conv, f0, f1, out_dtypes, acc_f64)

    # chain coefficient
    chain = 0.0
    if f1 is not None:
        rest = {}
        for i, (leaf, c) in f1.terms.items():
            if isinstance(leaf, Node):
                chain += c
            else:
                rest[i] = (leaf, c)
        f1 = Lin(rest, f1.shape, f1.device)

    # channels-last route: every tensor operand in one dense channels-last layout, no rounded conversion (Runge-Kutta stages), no capture
    # hook, no autograd recording
    leaves = [leaf for f in (f0, f1) if f is not None for leaf, _ in f.terms.values() if isinstance(leaf, torch.Tensor)]
    keep_layout = conv is None and not grad_recorded(*leaves)
    plan, operands, seeds = _lower(conv, f0, f1, chain, out_dtypes, acc_f64, keep_layout=keep_layout)
    layout = in_place_layout(operands, shape, keep_layout)
    if layout is not None:
        plan.sample_numel = layout[0] * layout[1]
        out0 = empty_output(shape, out_dtypes[0], device, channels_last=True)
        out1 = empty_output(shape, out_dtypes[1], device, channels_last=True) if f1 is not None else None
        _hip.launch_step(plan, operands, out0, out1, seeds, numel, device, layout)
        return [out0] if out1 is None else [out0, out1]
    if torch.is_grad_enabled() and any(t.requires_grad for t in operands):
        if conv is not None:
            plan_a = conversion_gradient(conv.to_kind, conv.from_kind, conv.k)
        else:
            plan_a = None
        outs = _StepFunction.apply(plan, plan_a, seeds, shape, numel, device, *operands)
        return list(outs) if f1 is not None else [outs]
    out0 = empty_output(shape, out_dtypes[0], device)
    out1 = empty_output(shape, out_dtypes[1], device) if f1 is not None else None
    _hip.launch_step(plan, operands, out0, out1, seeds, numel, device)
    return [out0] if out1 is None else [out0, out1]


def _lower(conv, f0: "Lin", f1: "Lin | None", chain: float, out_dtypes, acc_f64: bool | None, fuse1: bool = True, max_terms: int = _hip.MAX_TERMS,
           keep_layout: bool = False):
    """Two expanded forms over one operand list -> (plan, operands, seeds): leaves merged (a tensor in both forms is ONE operand with both
    coefficients), at most one fused Philox draw per form, operands in at most two dtype groups.  `out_dtypes` has one entry per OUTPUT:
    evaluate() stores both forms (two entries when f1 is given), evaluate_masked() blends them into one (one entry; `fuse1` False: a
    Philox leaf of the second form is realised to a tensor, its launch has no second draw)."""
    shape, numel = f0.shape, math.prod(f0.shape)
    # split leaves
    tensors: dict[int, torch.Tensor] = {}
    c0: dict[int, float] = {}
    c1: dict[int, float] = {}
    noise0: list[tuple[PhiloxNoise, float]] = []
    noise1: list[tuple[PhiloxNoise, float]] = []
    for which, form in ((0, f0), (1, f1)):
        if form is None:
            continue
        for i, (leaf, c) in form.terms.items():
            if c == 0.0 and not (conv is not None and which == 0):
                continue
            if isinstance(leaf, PhiloxNoise):
                (noise0 if which == 0 else noise1).append((leaf, c))
            else:
                tensors[i] = leaf
                (c0 if which == 0 else c1)[i] = c

    # in-kernel Philox: one draw per output, fusable shapes only; the rest is realised to tensors
    noise_dtype = torch.float64 if torch.float64 in out_dtypes else torch.float32

    def pick(noises, fuse=True):
        fused, extra = None, []
        for nz, c in noises:
            if fused is None and fuse and nz.fusable() and nz.shape == shape:
                fused = (nz, c)
            else:
                extra.append((nz.realize(noise_dtype), c))
        return fused, extra

    fused0, extra0 = pick(noise0)
    fused1, extra1 = pick(noise1, fuse1)
    if fused0 is not None and fused1 is not None and fused0[0].seeds is not fused1[0].seeds:
        extra1.append((fused1[0].realize(noise_dtype), fused1[1]))
        fused1 = None
    for t, c in extra0:
        tensors[id(t)] = t
        c0[id(t)] = c0.get(id(t), 0.0) + c
    for t, c in extra1:
        tensors[id(t)] = t
        c1[id(t)] = c1.get(id(t), 0.0) + c

    # dtype groups (<= 2); stragglers are cast with a single-term launch of the same kernel
    wide = torch.float64 if any(t.dtype == torch.float64 for t in tensors.values()) or torch.float64 in out_dtypes else torch.float32
    if acc_f64 is None:
        acc_f64 = wide == torch.float64 or _compute_dtype.get() == torch.float64
    if acc_f64:
        wide = torch.float64
    # (keep_layout: operands that all share one dense channels-last layout go in as they are -- evaluate() reads the layout off them)
    prepare = _prepare_keeping_layout if in_place_layout(tensors.values(), shape, keep_layout) is not None else _prepare_tensor
    prepared = {i: prepare(t) for i, t in tensors.items()}
    for t in prepared.values():
        if t.shape != shape and t.numel() != numel:
            raise SkrampleHipError(f"operand shape {tuple(t.shape)} does not match {shape}")
    narrow_types = [t.dtype for t in prepared.values() if t.dtype != wide]
    group_a = max(dict.fromkeys(narrow_types), key=narrow_types.count) if narrow_types else wide  # (first seen wins a tie: no dependence on hash order)
    if conv is not None and conv.dtype == wide:
        group_a = wide  # the rounded conversion's operands lead group A: whatever is narrower (fp32 noise beside fp64 latents) is widened, exactly, below
    # outputs must be group_a or wide
    for k, od in enumerate(out_dtypes):
        if od not in (group_a, wide):
            if not narrow_types or all(d == wide for d in narrow_types):
                group_a = od  # no narrow inputs: the narrow slot is free for the output dtype
            else:
                raise SkrampleHipError(f"output dtype {od} incompatible with operand dtypes {group_a}/{wide}")
    for i, t in list(prepared.items()):
        if t.dtype not in (group_a, wide):
            prepared[i] = cast(t, wide)
    ids_a = [i for i, t in prepared.items() if t.dtype == group_a]
    ids_b = [i for i, t in prepared.items() if t.dtype != group_a]
    if conv is not None:
        if group_a != conv.dtype:
            raise SkrampleHipError("rounded conversion operands must form the narrow dtype group")
        lead = [id(conv.sample), id(conv.output)]
        ids_a = lead + [i for i in ids_a if i not in lead]
    order = ids_a + ids_b
    if len(order) > max_terms:
        raise SkrampleHipError(f"{len(order)} operands exceed the kernel limit of {max_terms}")

    plan = _hip.StepPlanC()
    plan.n_terms = len(order)
    plan.n_group_a = len(ids_a)
    plan.dtype_a = _hip.DTYPE_CODE[group_a]
    plan.dtype_b = _hip.DTYPE_CODE[wide]
    plan.out0_dtype = _hip.DTYPE_CODE[out_dtypes[0]]
    plan.out1_dtype = _hip.DTYPE_CODE[out_dtypes[1]] if len(out_dtypes) > 1 else _hip.NONE
    plan.acc_f64 = 1 if acc_f64 else 0
    for k, i in enumerate(order):
        plan.coef0[k] = c0.get(i, 0.0)
        plan.coef1[k] = c1.get(i, 0.0)
    plan.chain = chain
    if conv is not None:
        plan.convert_to, plan.convert_from = conv.to_kind, conv.from_kind
        for k in range(4):
            plan.convert_k[k] = conv.k[k]
    seeds = None
    if fused0 is not None or fused1 is not None:
        plan.noise_mode = 1
        src = fused0 or fused1
        seeds = src[0].seeds
        plan.sample_numel = src[0].sample_numel
        if fused0 is not None:
            plan.zeta0, plan.stream0 = fused0[1], fused0[0].stream
        if fused1 is not None:
            plan.zeta1, plan.stream1 = fused1[1], fused1[0].stream
    return plan, [prepared[i] for i in order], seeds


# ---- masked steps (in-painting): out = m * form + (1 - m) * known, one launch --------------------------------------------------------
def mask_layout(mask_shape: Sequence[int], shape: Sequence[int]) -> tuple[int, int]:
    """(mask_numel, batch_stride) of a mask over a (B, *sample) tensor (skr_step_mask).  The mask broadcasts over LEADING axes only:
    behind its leading 1s (and missing axes) it spells the trailing axes of the sample out in full -- (B,1,H,W), (1,1,H,W), (B,C,H,W),
    (H,W) over (B,C,H,W).  A batch axis of B selects one mask per sample; it is only accepted on a mask of the tensor's own rank."""
    shape, mask_shape = tuple(shape), tuple(mask_shape)
    refuse = f"a mask of shape {mask_shape} does not broadcast over leading axes of {shape}"
    if len(shape) < 2 or not 1 <= len(mask_shape) <= len(shape):
        raise SkrampleHipError(refuse)
    full = (1,) * (len(shape) - len(mask_shape)) + mask_shape
    if full[0] not in (1, shape[0]):
        raise SkrampleHipError(f"{refuse}: its batch axis must be 1 or {shape[0]}")
    inner = 1
    while inner < len(shape) and full[inner] == 1:
        inner += 1  # (a leading sample axis the mask is broadcast over)
    if full[inner:] != shape[inner:]:
        raise SkrampleHipError(f"{refuse}: behind its leading 1s it must spell out {shape[inner:]}")
    mask_numel = math.prod(shape[inner:])
    return mask_numel, (mask_numel if full[0] == shape[0] and shape[0] != 1 else 0)


def evaluate_masked(form: Lin, known: Lin, mask: torch.Tensor, dtype: torch.dtype | None = None, acc_f64: bool | None = None) -> torch.Tensor:
    """mask * form + (1 - mask) * known in ONE launch (skr_step_launch_masked): `form` is a solver step (it may hold one fused Philox
    draw), `known` the re-noised kept region.  The leaves of both are merged into one operand list.  Host-resident operands evaluate
    the same expression with torch ops in the accumulate type.
    Channels-last: when every tensor leaf of both forms shares one dense channels-last layout (`shared_layout`), `lazy.channels_last`
    is on, no `_hip.indexed` hook is installed and nothing is grad-recorded, the launch is skr_step_launch_masked_channels_last: no
    operand is copied, the result is channels-last and has the bits of the contiguous launch; the mask goes in logical order.
    Mixed layouts, captured loops and recorded steps take the contiguous path.
    Autograd: device operands that require grad while autograd records go through `_MaskedStepFunction`, whose backward is one
    skr_step_masked_backward_launch; the forward's bits are those of the launch without autograd.  The mask has no gradient (it would
    need the operands and a reduction over the broadcast axes): a mask that requires grad is refused.  Host-resident operands that
    require grad stay refused: the host executor of a masked step has no backward."""
    f0, f1 = lift(form), lift(known)
    if not isinstance(f0, Lin) or not isinstance(f1, Lin) or not isinstance(mask, torch.Tensor):
        raise SkrampleHipError("evaluate_masked() takes two tensor forms and a mask tensor")
    f0, f1 = f0.expanded(), f1.expanded()
    if f1.shape != f0.shape:
        raise SkrampleHipError(f"shape mismatch between the step form {f0.shape} and the known form {f1.shape}")
    if any(isinstance(leaf, Node) for f in (f0, f1) for leaf, _ in f.terms.values()):
        raise SkrampleHipError("a masked launch has one output: its forms cannot refer to a stored form")
    shape, device = f0.shape, f0.device
    _check_tensor(mask)
    mask_numel, batch_stride = mask_layout(mask.shape, shape)
    out_dtype = dtype if dtype is not None else _default_dtype(f0)
    leaves = [leaf for f in (f0, f1) for leaf, _ in f.terms.values() if isinstance(leaf, torch.Tensor)]
    if grad_recorded(mask):
        raise SkrampleHipError("the mask of a masked step has no gradient: detach it, or run the step under torch.no_grad()")
    recorded = grad_recorded(*leaves)
    if is_host(device) or is_host(f1.device):
        if recorded:
            raise SkrampleHipError("a masked step has no backward: run it under torch.no_grad() or on operands that do not require grad")
        return _host_evaluate_masked(f0, f1, mask, out_dtype, acc_f64)
    if not mask.is_cuda or mask.device != device:
        raise SkrampleHipError("operands of one step must all live on the HIP device or all on the host")
    # channels-last route: every tensor leaf of both forms in one dense channels-last layout, no capture hook, no autograd recording
    plan, operands, seeds = _lower(None, f0, f1, 0.0, [out_dtype], acc_f64, fuse1=False, max_terms=_hip.ROW_TERMS, keep_layout=not recorded)
    if mask.dtype == torch.float64 and not plan.acc_f64:
        raise SkrampleHipError("a float64 mask needs float64 accumulation")
    numel = math.prod(shape)
    plan.sample_numel = numel // shape[0] if shape[0] else 1
    layout = in_place_layout(operands, shape, not recorded)
    if layout is not None:
        # the operands stay as they are and the result is channels-last; the mask keeps its logical order (a single-channel mask is
        # contiguous in either memory format: no copy)
        out = empty_output(shape, out_dtype, device, channels_last=True)
        _hip.launch_step_masked(plan, operands, out, _prepare_tensor(mask), mask_numel, batch_stride, seeds, numel, device, layout)
        return out
    if recorded:
        return _MaskedStepFunction.apply(plan, seeds, shape, numel, device, _prepare_tensor(mask), mask_numel, batch_stride, *operands)
    out = empty_output(shape, out_dtype, device)
    _hip.launch_step_masked(plan, operands, out, _prepare_tensor(mask), mask_numel, batch_stride, seeds, numel, device)
    return out


# The blend a scheduler wrapper has pending for the step it is about to take (SkrampleWrapperScheduler.set_inpaint): a sampler whose step
# is one single-output launch settles its form through it (StatedSampler.sample_packed), which makes that launch the masked one.
_pending_blend: contextvars.ContextVar = contextvars.ContextVar("skr_pending_blend", default=None)


class MaskedBlend:
    "context manager: `with MaskedBlend(known, mask): sampler.sample_packed(...)`; taken up at most once"

    def __init__(self, known: Lin, mask: torch.Tensor):
        self.known, self.mask, self.used = known, mask, False

    def __enter__(self):
        self.token = _pending_blend.set(self)
        return self

    def __exit__(self, *exc):
        _pending_blend.reset(self.token)

    def settle(self, form: Lin, dtype: torch.dtype | None) -> torch.Tensor:
        self.used = True
        return evaluate_masked(form, self.known, self.mask, dtype)


def pending_blend() -> "MaskedBlend | None":
    blend = _pending_blend.get()
    return blend if blend is not None and not blend.used else None


# ---- guided steps (classifier-free guidance): the three torch lines in front of a step, inside its launch ----------------------------
def guide_only(guidance: Guidance) -> torch.Tensor:
    """the guided prediction as a tensor of its own, with torch's bits: one guidance-only launch of skr_step_launch_guided on the HIP
    device (uncond and cond in one dense channels-last layout: on the storage order as it stands, the result channels-last); torch's own
    three lines for host-resident operands and for operands that autograd records (torch records them).
    A rescaled guidance (`guidance.rescale != 0`) is the statistics launch and the guidance-only form of skr_step_launch_guided_rescaled
    under the same conditions, and torch's lines with rescale_noise_cfg's four otherwise."""
    u, c = guidance.uncond, guidance.cond
    if is_host(guidance.device) or grad_recorded(u, c):
        return _host_result(guidance.torch_lines(), (u, c), guidance.shape)
    in_place = in_place_layout((u, c), guidance.shape) is not None
    prepare = _prepare_keeping_layout if in_place else _prepare_tensor
    u, c = prepare(u), prepare(c)
    out = empty_output(guidance.shape, guidance.dtype, guidance.device, channels_last=in_place)
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = 1
    plan.dtype_a = plan.dtype_b = _hip.DTYPE_CODE[guidance.dtype]
    plan.out0_dtype = plan.out1_dtype = _hip.NONE
    plan.acc_f64 = 1 if guidance.dtype == torch.float64 else 0
    plan.coef0[0] = 1.0
    numel = math.prod(guidance.shape)
    if guidance.rescale != 0.0:  # the statistic over the same storage order, then the rescaled guidance-only launch
        _hip.launch_step_guided_rescaled(plan, [u], None, c, out, guidance.scale, 0, guidance.device_factor(u, c), guidance.rescale, numel // guidance.shape[0], None, numel, guidance.device)
    else:
        _hip.launch_step_guided(plan, [u], None, c, out, guidance.scale, 0, None, numel, guidance.device)
    return out


def evaluate_guided(form: Lin, guidance: Guidance, dtype: torch.dtype | None = None, acc_f64: bool | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """(final, guided): `form`, which holds `guidance.node()` wherever the prediction stands, and the guided prediction itself, in ONE
    launch (skr_step_launch_guided).  The node is lowered as the operand `uncond` at its natural position in the operand list -- that
    position is the launch's `slot` -- so `final` has the bits of evaluate() over the form with the tensor `guided` in the node's place,
    and `guided` the bits of torch's three lines.
    What the one launch does not cover takes the guidance-only launch (`guide_only`) and then evaluate(): contiguous copies would be
    needed (channels-last or strided operands), the node's coefficient is zero, `uncond` is an operand of the form in its own right or
    is cast to another dtype group, or the form has more than 16 operands.  Host-resident operands and operands that autograd records
    evaluate the three lines with torch and then the existing executors.  Mixed residency is refused as everywhere.
    A rescaled guidance takes the same routes with one statistics launch in front (skr_guidance_rescale_factor, then
    skr_step_launch_guided_rescaled); `guided` is then the rescaled prediction."""
    f = lift(form)
    if not isinstance(f, Lin) or not isinstance(guidance, Guidance):
        raise SkrampleHipError("evaluate_guided() takes a tensor form and a Guidance")
    f = f.expanded(keep=guidance)
    if any(isinstance(leaf, Node) and leaf.form is not guidance for leaf, _ in f.terms.values()):
        raise SkrampleHipError("a guided launch has one step output: its form cannot refer to another stored form")
    if f.shape != guidance.shape:
        raise SkrampleHipError(f"shape mismatch between the step form {f.shape} and the guidance operands {guidance.shape}")
    leaves = [leaf for leaf, _ in f.terms.values() if isinstance(leaf, torch.Tensor)]
    host = [is_host(t.device) for t in (*leaves, guidance.uncond)] + ([True] if f.device == NUMPY else [])
    if any(host) and not all(host):
        raise SkrampleHipError("operands of one step must all live on the HIP device or all on the host")
    out_dtype = dtype if dtype is not None else guidance.dtype
    u, c = guidance.uncond, guidance.cond
    fused = not any(host) and not grad_recorded(*leaves, u, c) and all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in (*leaves, u, c))
    fused = fused and id(u) not in f.terms and any(isinstance(leaf, Node) and k != 0.0 for leaf, k in f.terms.values())
    if fused:
        plan, operands, seeds = _lower(None, f.substitute(guidance, u), None, 0.0, [out_dtype], acc_f64)
        slot = next((k for k, t in enumerate(operands) if t is u), None)
        if slot is not None and len(operands) <= _hip.ROW_TERMS:
            final = empty_output(f.shape, out_dtype, guidance.device)
            guided = empty_output(f.shape, guidance.dtype, guidance.device)
            numel = math.prod(f.shape)
            if guidance.rescale != 0.0:  # the statistics launch, then the step with its per-sample factor
                _hip.launch_step_guided_rescaled(plan, operands, final, c, guided, guidance.scale, slot, guidance.device_factor(u, c), guidance.rescale, numel // f.shape[0],
                                                 seeds, numel, guidance.device)
            else:
                _hip.launch_step_guided(plan, operands, final, c, guided, guidance.scale, slot, seeds, numel, guidance.device)
            return final, guided
    guided = guide_only(guidance)
    return evaluate([f.substitute(guidance, guided)], [out_dtype], acc_f64)[0], guided


# The guidance a scheduler wrapper has pending for the step it is about to take (SkrampleWrapperScheduler.step_guided): a sampler whose
# step is one single-output launch settles its form through it (StatedSampler.sample_packed), which makes that launch the guided one.
_pending_guidance: contextvars.ContextVar = contextvars.ContextVar("skr_pending_guidance", default=None)


class GuidedStep:
    "context manager: `with GuidedStep(guidance): sampler.sample_packed(...)`; taken up at most once, and keeps the stored prediction"

    def __init__(self, guidance: Guidance):
        self.guidance, self.used, self.guided = guidance, False, None

    def __enter__(self):
        self.token = _pending_guidance.set(self)
        return self

    def __exit__(self, *exc):
        _pending_guidance.reset(self.token)

    def settle(self, form: Lin, dtype: torch.dtype | None) -> torch.Tensor:
        self.used = True
        final, self.guided = evaluate_guided(form, self.guidance, dtype)
        return final


def pending_guidance() -> "GuidedStep | None":
    pending = _pending_guidance.get()
    return pending if pending is not None and not pending.used else None


def _host_evaluate_masked(f0: "Lin", f1: "Lin", mask: torch.Tensor, out_dtype: torch.dtype, acc_f64) -> torch.Tensor:
    "host executor of evaluate_masked (CPU torch tensors): the same expression in the accumulate type, rounded once"
    leaves = [leaf for form in (f0, f1) for leaf, _ in form.terms.values() if isinstance(leaf, torch.Tensor)]
    for t in (*leaves, mask):
        if t.device.type != "cpu":
            raise SkrampleHipError("operands of one step must all live on the HIP device or all on the host")
    if f0.device == NUMPY or f1.device == NUMPY:
        raise SkrampleHipError("masked steps take torch tensors")
    wide = torch.float64 if acc_f64 or _compute_dtype.get() == torch.float64 or out_dtype == torch.float64 or any(t.dtype == torch.float64 for t in leaves) else torch.float32

    def total(form):
        acc = torch.zeros(form.shape, dtype=wide)
        for leaf, c in form.terms.values():
            if isinstance(leaf, PhiloxNoise):
                raise SkrampleHipError("in-kernel Philox noise exists on the HIP device only")
            if c != 0.0:
                acc.add_(leaf.to(wide) * c)
        return acc

    m = mask.to(wide).reshape((1,) * (len(f0.shape) - mask.ndim) + tuple(mask.shape))
    return _host_result((m * total(f0) + (1 - m) * total(f1)).to(out_dtype), leaves, f0.shape)


# ---- autograd ------------------------------------------------------------------------------------------------------------------------
# A step is linear in its tensor operands with host fp64 coefficients, so its backward is the transposed step (skr_step_backward_launch):
#     grad_k = a_k * g0 + b_k * g1,   a_k = coef0_k,  b_k = chain * coef0_k + coef1_k
# one launch, no saved tensors.  The Functions below are used only while autograd records and an operand requires grad: every other
# call takes the launches above unchanged.
def grad_recorded(*tensors) -> bool:
    "autograd is recording and some tensor among `tensors` requires grad"
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


def conversion_gradient(to_kind: int, from_kind: int, k: Sequence[float]) -> tuple[float, float]:
    """(d out0 / d s, d out0 / d o) of the rounded pair conversion out0 = from_x(s, to_x(s, o)) (include/skrample_hip.h, convert_*):
    affine in (s, o), so its derivative is two numbers, folded into the operands' coef0"""
    # to_x: x = xs * s + xo * o
    # (only the kind's own constants are read: the others may be 0)
    xs, xo = {0: lambda: (0.0, 1.0), 1: lambda: (1.0 / k[1], -k[0] / k[1]), 2: lambda: (k[1], -k[0]), 3: lambda: (0.0, k[0])}[to_kind]()
    # from_x: v = vs * s + vx * x
    vs, vx = {0: lambda: (0.0, 1.0), 1: lambda: (1.0 / k[3], -k[2] / k[3]), 2: lambda: (k[2] / k[3], -1.0 / k[3]), 3: lambda: (0.0, 1.0 / k[2])}[from_kind]()
    return vs + vx * xs, vx * xo


def transposed(plan, conv_grad, n: int) -> tuple[list[float], list[float]]:
    "(a_k, b_k) of every operand of a forward plan: the gradient of operand k is a_k * grad(out0) + b_k * grad(out1)"
    a = [plan.coef0[k] for k in range(n)]
    if conv_grad is not None:
        a[0], a[1] = conv_grad
    b = [plan.chain * a[k] + plan.coef1[k] for k in range(n)] if plan.out1_dtype != _hip.NONE else [0.0] * n
    return a, b


def launch_backward(g0, g1, a: Sequence[float], b: Sequence[float], like: Sequence[torch.Tensor], acc_f64: bool) -> list[torch.Tensor]:
    """grads[k] = a[k] * g0 + b[k] * g1 (g0 or g1 may be None) in one skr_step_backward_launch; grads[k] has like[k]'s dtype and shape.
    `like` must be grouped by dtype (at most two groups)."""
    if g0 is None:
        g0, g1, a, b = g1, None, b, a
    device = g0.device
    g0 = _prepare_tensor(g0)
    g1 = _prepare_tensor(g1) if g1 is not None else None
    grads = [torch.empty(t.shape, dtype=t.dtype, device=device) for t in like]
    plan = _hip.StepGradPlanC()
    plan.n_grads = len(grads)
    plan.dtype_a = _hip.DTYPE_CODE[grads[0].dtype]
    plan.n_group_a = sum(1 for t in grads if t.dtype == grads[0].dtype)
    plan.dtype_b = _hip.DTYPE_CODE[grads[-1].dtype]
    if any(t.dtype != grads[0].dtype for t in grads[: plan.n_group_a]) or len({t.dtype for t in grads}) > 2:
        raise SkrampleHipError("gradients must come in at most two dtype groups")
    plan.g0_dtype = _hip.DTYPE_CODE[g0.dtype]
    plan.g1_dtype = _hip.DTYPE_CODE[g1.dtype] if g1 is not None else _hip.NONE
    plan.acc_f64 = 1 if acc_f64 else 0
    for k in range(len(grads)):
        plan.a[k] = a[k]
        plan.b[k] = b[k] if g1 is not None else 0.0
    arr = (ctypes.c_void_p * len(grads))(*[t.data_ptr() for t in grads])
    status = _hip.load().skr_step_backward_launch(ctypes.byref(plan), g0.data_ptr(), g1.data_ptr() if g1 is not None else None, arr, g0.numel(), _hip.current_stream_ptr(device))
    _hip.check(status, "skr_step_backward_launch")
    return grads


class _StepFunction(torch.autograd.Function):
    "one fused step launch (forward) and its transposed step (backward)"

    @staticmethod
    def forward(ctx, plan, conv_grad, seeds, shape, numel, device, *operands):
        ctx.set_materialize_grads(False)
        ctx.plan, ctx.conv_grad = plan, conv_grad
        # plain tensors: a view made here (empty_output's staggered placement) would make a later in-place op on the result raise
        out0 = torch.empty(shape, dtype=_hip.CODE_DTYPE[plan.out0_dtype], device=device)
        out1 = torch.empty(shape, dtype=_hip.CODE_DTYPE[plan.out1_dtype], device=device) if plan.out1_dtype != _hip.NONE else None
        _hip.launch_step(plan, list(operands), out0, out1, seeds, numel, device)
        ctx.like = [(t.shape, t.dtype) for t in operands]
        return out0 if out1 is None else (out0, out1)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g0, g1=None):
        n = len(ctx.like)
        skip = 6
        want = [k for k in range(n) if ctx.needs_input_grad[skip + k]]
        result: list = [None] * (skip + n)
        if not want or (g0 is None and g1 is None):
            return tuple(result)
        a, b = transposed(ctx.plan, ctx.conv_grad, n)
        like = [_Like(*ctx.like[k]) for k in want]
        grads = launch_backward(g0, g1, [a[k] for k in want], [b[k] for k in want], like, bool(ctx.plan.acc_f64))
        for k, g in zip(want, grads):
            result[skip + k] = g
        return tuple(result)


class _Like:
    "shape and dtype of a tensor a gradient is made for"

    __slots__ = ("shape", "dtype")

    def __init__(self, shape, dtype):
        self.shape, self.dtype = shape, dtype


def launch_masked_backward(g, mask: torch.Tensor, mask_numel: int, batch_stride: int, a: Sequence[float], b: Sequence[float], like: Sequence, sample_numel: int, acc_f64: bool) -> list[torch.Tensor]:
    """grads[k] = (a[k] * m + b[k] * (1 - m)) * g in one skr_step_masked_backward_launch; grads[k] has like[k]'s dtype and shape.
    `like` must be grouped by dtype (at most two groups), as for launch_backward."""
    device = g.device
    g = _prepare_tensor(g)
    grads = [torch.empty(t.shape, dtype=t.dtype, device=device) for t in like]
    plan = _hip.StepGradPlanC()
    plan.n_grads = len(grads)
    plan.dtype_a = _hip.DTYPE_CODE[grads[0].dtype]
    plan.n_group_a = sum(1 for t in grads if t.dtype == grads[0].dtype)
    plan.dtype_b = _hip.DTYPE_CODE[grads[-1].dtype]
    if any(t.dtype != grads[0].dtype for t in grads[: plan.n_group_a]) or len({t.dtype for t in grads}) > 2:
        raise SkrampleHipError("gradients must come in at most two dtype groups")
    plan.g0_dtype, plan.g1_dtype = _hip.DTYPE_CODE[g.dtype], _hip.NONE
    plan.acc_f64 = 1 if acc_f64 else 0
    for k in range(len(grads)):
        plan.a[k], plan.b[k] = a[k], b[k]
    arr = (ctypes.c_void_p * len(grads))(*[t.data_ptr() for t in grads])
    desc = _hip.StepMaskC(mask.data_ptr(), _hip.DTYPE_CODE[mask.dtype], 0, mask_numel, batch_stride)
    status = _hip.load().skr_step_masked_backward_launch(ctypes.byref(plan), g.data_ptr(), ctypes.byref(desc), arr, g.numel(), sample_numel, _hip.current_stream_ptr(device))
    _hip.check(status, "skr_step_masked_backward_launch")
    return grads


class _MaskedStepFunction(torch.autograd.Function):
    "one masked step launch (forward) and its transposed step (backward); the mask is the only tensor kept"

    @staticmethod
    def forward(ctx, plan, seeds, shape, numel, device, mask, mask_numel, batch_stride, *operands):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(mask)
        ctx.plan, ctx.mask_numel, ctx.batch_stride = plan, mask_numel, batch_stride
        # a plain tensor, as in _StepFunction: no view whose later in-place modification would raise
        out = torch.empty(shape, dtype=_hip.CODE_DTYPE[plan.out0_dtype], device=device)
        _hip.launch_step_masked(plan, list(operands), out, mask, mask_numel, batch_stride, seeds, numel, device)
        ctx.like = [(t.shape, t.dtype) for t in operands]
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        n = len(ctx.like)
        skip = 8
        want = [k for k in range(n) if ctx.needs_input_grad[skip + k]]
        result: list = [None] * (skip + n)
        if not want or g is None:
            return tuple(result)
        plan, (mask,) = ctx.plan, ctx.saved_tensors
        like = [_Like(*ctx.like[k]) for k in want]
        grads = launch_masked_backward(g, mask, ctx.mask_numel, ctx.batch_stride, [plan.coef0[k] for k in want], [plan.coef1[k] for k in want],
                                       like, plan.sample_numel, bool(plan.acc_f64))
        for k, grad in zip(want, grads):
            result[skip + k] = grad
        return tuple(result)



def _host_evaluate(conv, f0: "Lin", f1, out_dtypes, acc_f64) -> list:
    """Host executor for host-resident operands (CPU torch tensors / numpy arrays): the same one or two forms, evaluated
    with plain torch ops in the accumulator precision the kernel uses (fp32, or fp64 when asked for), each output rounded
    once.  Not a fallback: forms over HIP tensors never come here, and a form that mixes residencies is refused."""
    as_numpy = f0.device == NUMPY or (f1 is not None and f1.device == NUMPY)
    leaves = [leaf for form in (f0, f1) if form is not None for leaf, _ in form.terms.values() if isinstance(leaf, torch.Tensor)]
    if conv is not None:
        leaves += [conv.sample, conv.output]
    for t in leaves:
        if t.device.type != "cpu":
            raise SkrampleHipError("operands of one step must all live on the HIP device or all on the host")
    wide = torch.float64 if acc_f64 or _compute_dtype.get() == torch.float64 or torch.float64 in out_dtypes or any(t.dtype == torch.float64 for t in leaves) else torch.float32

    def total(form, start=None):
        acc = start
        for leaf, c in form.terms.values():
            if isinstance(leaf, Node):
                continue  # the chained term is added by the caller
            if isinstance(leaf, PhiloxNoise):
                raise SkrampleHipError("in-kernel Philox noise exists on the HIP device only")
            if c == 0.0:
                continue
            term = leaf.to(wide) * c
            acc = term if acc is None else acc.add_(term)
        return acc if acc is not None else torch.zeros(form.shape, dtype=wide)

    if conv is not None:
        # the reference's op-by-op conversion in the operands' own dtype (diffusers.py:819-834, models.py:92-224)
        s_, o_, k = conv.sample, conv.output, conv.k
        x = {0: lambda: o_, 1: lambda: (s_ - k[0] * o_) / k[1], 2: lambda: k[1] * s_ - k[0] * o_, 3: lambda: o_ * k[0]}[conv.to_kind]()
        v0 = {0: lambda: x, 1: lambda: (s_ - k[2] * x) / k[3], 2: lambda: (k[2] * s_ - x) / k[3], 3: lambda: x / k[2]}[conv.from_kind]()
        acc0 = v0.to(wide)
    else:
        acc0 = total(f0)
    outs = [acc0.to(out_dtypes[0])]
    if f1 is not None:
        chain = sum(c for leaf, c in f1.terms.values() if isinstance(leaf, Node))
        acc1 = total(f1, acc0 * chain if chain != 0.0 else None)
        outs.append(acc1.to(out_dtypes[1]))
    outs = [_host_result(o, leaves, f0.shape) for o in outs]
    return [o.numpy() for o in outs] if as_numpy else outs


def _host_result(out: torch.Tensor, leaves, shape) -> torch.Tensor:
    """a host result in the layout a device launch returns: dense channels-last when every tensor operand shares that layout, contiguous
    otherwise (torch's own ops hand the strides of a permuted or sliced operand on to their result)"""
    if leaves and shared_layout(leaves, shape) is not None:
        return out if layout_of(out) is not None else empty_output(shape, out.dtype, out.device, channels_last=True).copy_(out)
    return out.contiguous()


def cast(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    "dtype conversion through the engine (a one-term fused launch)"
    if t.dtype == dtype:
        return t
    return evaluate([Lin.leaf(t)], [dtype])[0]


_norm_ws: dict = {}


def error_mean(a, b: torch.Tensor, power: int) -> float:
    "mean(|a - b|^power) over a device tensor pair (a may be the number 0); one reduction launch + read-back (ndarrays: on the host)"
    a = _from_numpy(a) if type(a).__module__ == "numpy" and hasattr(a, "__array_interface__") and getattr(a, "ndim", 0) > 0 else a
    b = _from_numpy(b) if type(b).__module__ == "numpy" and hasattr(b, "__array_interface__") else b
    _check_tensor(b)
    if not isinstance(a, torch.Tensor) and a != 0:
        raise SkrampleHipError("error norm against a non-zero scalar is not supported")
    if not b.is_cuda:  # host-resident operands: plain torch (fp64 accumulation, as the kernel)
        d = (b.double() if not isinstance(a, torch.Tensor) else a.double() - b.double()).abs()
        return float((d if power == 1 else d.pow(power)).mean())
    if isinstance(a, torch.Tensor):
        _check_tensor(a)
        if a.dtype != b.dtype or a.shape != b.shape:
            raise SkrampleHipError("error norm operands must share dtype and shape")
        a = _prepare_tensor(a)
    b = _prepare_tensor(b)
    ws = _norm_ws.get(b.device)
    if ws is None:
        ws = _norm_ws[b.device] = torch.empty(1025, dtype=torch.float64, device=b.device)
    lib = _hip.load()
    status = lib.skr_error_mean(a.data_ptr() if isinstance(a, torch.Tensor) else None, b.data_ptr(), _hip.DTYPE_CODE[b.dtype], b.numel(), power, ws.data_ptr(), ws.data_ptr() + 8, _hip.current_stream_ptr(b.device))
    _hip.check(status, "skr_error_mean")
    return ws[0].item()


def power_blend(a: torch.Tensor, b: torch.Tensor, wa: float, wb: float, power: float, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    "spowf(wa * spowf(a, power) + wb * spowf(b, power), 1 / power) as one elementwise launch; fp32 or fp64 result (ndarrays in: ndarray out)"
    as_numpy = not isinstance(a, torch.Tensor) or not isinstance(b, torch.Tensor)
    a = a if isinstance(a, torch.Tensor) else _from_numpy(a)
    b = b if isinstance(b, torch.Tensor) else _from_numpy(b)
    _check_tensor(a)
    _check_tensor(b)
    if a.shape != b.shape:
        raise SkrampleHipError(f"shape mismatch in sampler operands: {tuple(a.shape)} vs {tuple(b.shape)}")
    if dtype not in (torch.float32, torch.float64):
        raise SkrampleHipError("the signed-power blend is evaluated in float32 or float64")
    if not a.is_cuda and not b.is_cuda:  # host-resident operands
        spow = lambda v, f: v.abs().pow(f) * torch.where(v < 0, -1.0, 1.0).to(v.dtype)  # noqa: E731  (sign(+-0) = +1, as the kernel and the reference)
        blended = spow(wa * spow(a.to(dtype), power) + wb * spow(b.to(dtype), power), 1 / power).contiguous()  # (the device launch copies views: contiguous, as there)
        return blended.numpy() if as_numpy else blended
    a, b = _prepare_tensor(a), _prepare_tensor(b)
    if grad_recorded(a, b):
        return _PowerBlendFunction.apply(float(wa), float(wb), float(power), dtype, a, b)
    out = empty_output(a.shape, dtype, a.device)
    status = _hip.load().skr_power_blend(out.data_ptr(), _hip.DTYPE_CODE[dtype], a.data_ptr(), _hip.DTYPE_CODE[a.dtype], b.data_ptr(), _hip.DTYPE_CODE[b.dtype], float(wa), float(wb), float(power), a.numel(), _hip.current_stream_ptr(a.device))
    _hip.check(status, "skr_power_blend")
    return out


class _PowerBlendFunction(torch.autograd.Function):
    "skr_power_blend (forward) and skr_power_blend_backward: the one non-linear step operation, so the one that saves its operands"

    @staticmethod
    def forward(ctx, wa, wb, power, dtype, a, b):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(a, b)
        ctx.wa, ctx.wb, ctx.power = wa, wb, power
        out = torch.empty(a.shape, dtype=dtype, device=a.device)
        status = _hip.load().skr_power_blend(out.data_ptr(), _hip.DTYPE_CODE[dtype], a.data_ptr(), _hip.DTYPE_CODE[a.dtype], b.data_ptr(), _hip.DTYPE_CODE[b.dtype], wa, wb, power, a.numel(), _hip.current_stream_ptr(a.device))
        _hip.check(status, "skr_power_blend")
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        if g is None:
            return None, None, None, None, None, None
        g = _prepare_tensor(g)
        ga = torch.empty_like(a, memory_format=torch.contiguous_format) if ctx.needs_input_grad[4] else None
        gb = torch.empty_like(b, memory_format=torch.contiguous_format) if ctx.needs_input_grad[5] else None
        status = _hip.load().skr_power_blend_backward(
            ga.data_ptr() if ga is not None else None, gb.data_ptr() if gb is not None else None, g.data_ptr(), _hip.DTYPE_CODE[g.dtype],
            a.data_ptr(), _hip.DTYPE_CODE[a.dtype], b.data_ptr(), _hip.DTYPE_CODE[b.dtype], ctx.wa, ctx.wb, ctx.power, a.numel(), _hip.current_stream_ptr(a.device))
        _hip.check(status, "skr_power_blend_backward")
        return None, None, None, None, ga, gb


def settle(value, like=None, dtype: torch.dtype | None = None):
    "number -> number; form -> tensor (one launch)"
    if isinstance(value, Lin):
        if dtype is None and isinstance(like, torch.Tensor):
            dtype = like.dtype
        return evaluate([value], [dtype])[0]
    return value


class LazyTensor:
    """A form that is evaluated on first use.  Returned where the reference returns a tensor that
    callers rarely read (e.g. `pred_original_sample`): unused, it costs no HBM traffic; used in any
    torch function, arithmetic, indexing or via `.materialize()`, it becomes an ordinary tensor.

    The form's leaves are the caller's own tensors, so a late evaluation would silently use whatever they hold by
    then: every leaf is stamped (data_ptr, _version) at creation and `materialize()` refuses to run once one of them
    has been modified in place -- read the value before reusing the buffers, as with any view."""

    def __init__(self, form: Lin | None, dtype: torch.dtype, form_fn=None, shape=None, device=None, leaves=None, acc_f64: bool | None = None):
        self._form, self._form_fn, self.dtype, self._value = form, form_fn, dtype, None
        # the accumulator of the step that made this tensor (compute_scale=float64): it is read later, outside that step's context
        self._acc_f64 = (_compute_dtype.get() == torch.float64) if acc_f64 is None else bool(acc_f64)
        self._shape, self._device = shape, device
        if leaves is None and form is not None and isinstance(form, Lin):
            leaves = [leaf for leaf, _ in form.terms.values() if isinstance(leaf, torch.Tensor)]
        self._stamps = [(t, t.data_ptr(), t._version) for t in (leaves or ()) if isinstance(t, torch.Tensor)]

    @property
    def form(self) -> Lin:
        if self._form is None:
            self._form = self._form_fn()
        return self._form

    @property
    def shape(self):
        return self._shape if self._form is None and self._shape is not None else self.form.shape

    @property
    def device(self):
        return self._device if self._form is None and self._device is not None else self.form.device

    def materialize(self) -> torch.Tensor:
        if self._value is None:
            for t, ptr, version in self._stamps:
                if t._version != version or t.data_ptr() != ptr:
                    raise SkrampleHipError("an operand of this lazily evaluated tensor was modified in place before it was read; materialize() it (or use it) before reusing the buffers it was computed from")
            self._value = evaluate([self.form], [self.dtype], acc_f64=True if self._acc_f64 else None)[0]
            self._stamps = []
        return self._value

    def to(self, *args, **kwargs):
        return self.materialize().to(*args, **kwargs)

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return getattr(self.materialize(), name)

    # python operators and the container protocol are looked up on the type, not through __getattr__
    def __len__(self):
        return len(self.materialize())

    def __getitem__(self, key):
        return self.materialize()[key]

    def __iter__(self):
        return iter(self.materialize())

    def __neg__(self):
        return -self.materialize()

    def __abs__(self):
        return abs(self.materialize())

    def __array__(self, dtype=None):
        v = self.materialize().detach().cpu()
        return v.float().numpy() if v.dtype in (torch.bfloat16,) else (v.numpy() if dtype is None else v.numpy().astype(dtype))

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        def unwrap(a):
            if isinstance(a, LazyTensor):
                return a.materialize()
            if isinstance(a, (list, tuple)):
                return type(a)(unwrap(v) for v in a)
            return a

        return func(*unwrap(args), **{k: unwrap(v) for k, v in (kwargs or {}).items()})


def _lazy_binary(name: str):
    def op(self, other):
        other = other.materialize() if isinstance(other, LazyTensor) else other
        return getattr(self.materialize(), name)(other)

    op.__name__ = name
    return op


for _name in ("add", "radd", "sub", "rsub", "mul", "rmul", "truediv", "rtruediv", "pow", "rpow", "matmul", "rmatmul", "floordiv", "mod", "eq", "ne", "lt", "le", "gt", "ge"):
    setattr(LazyTensor, f"__{_name}__", _lazy_binary(f"__{_name}__"))
LazyTensor.__hash__ = object.__hash__  # (defining __eq__ would otherwise drop hashability)


def is_number(x: Any) -> bool:
    return isinstance(x, NUMBER)
