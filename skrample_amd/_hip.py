"""ctypes binding of libskrample_hip.so (include/skrample_hip.h).

The HIP library is the product: there is no CPU or eager-PyTorch fallback anywhere in this
package.  If the library is missing or a launch fails, `SkrampleHipError` is raised.
"""

from __future__ import annotations

import ctypes
import operator
import os
import sys
import threading

import torch

MAX_TERMS = 80
ABI_VERSION = 15
SKR_ERR_UNSUPPORTED = 7  # include/skrample_hip.h: valid request outside what the fast kernels cover

BF16, F16, F32, F64, NONE = 0, 1, 2, 3, -1
DTYPE_CODE = {torch.bfloat16: BF16, torch.float16: F16, torch.float32: F32, torch.float64: F64}
CODE_DTYPE = {v: k for k, v in DTYPE_CODE.items()}

LIB_NAME = "libskrample_hip.so"
# (SKR_HIP_LIB: a differently built library for A/B measurements -- tools/ only; the product loads the in-tree one)
LIB_PATH = os.environ.get("SKR_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", LIB_NAME)

EXPORTS = (
    "skr_step_launch",
    "skr_step_launch_indexed",
    "skr_step_launch_indexed_per_sample",
    "skr_step_launch_rolling",
    "skr_step_launch_channels_last",
    "skr_step_launch_masked",
    "skr_step_launch_masked_indexed",
    "skr_step_launch_masked_indexed_per_sample",
    "skr_step_launch_masked_rolling",
    "skr_step_launch_masked_channels_last",
    "skr_step_launch_guided",
    "skr_step_launch_guided_indexed",
    "skr_step_launch_guided_indexed_per_sample",
    "skr_step_launch_guided_rolling",
    "skr_guidance_rescale_factor",
    "skr_step_launch_guided_rescaled",
    "skr_guidance_rescale_factor_rolling",
    "skr_step_launch_guided_rescaled_rolling",
    "skr_guidance_rescale_factor_indexed",
    "skr_guidance_rescale_factor_indexed_per_sample",
    "skr_step_launch_guided_rescaled_indexed",
    "skr_step_launch_guided_rescaled_indexed_per_sample",
    "skr_rolling_advance",
    "skr_step_backward_launch",
    "skr_step_masked_backward_launch",
    "skr_program_create",
    "skr_program_create_channels_last",
    "skr_program_launch",
    "skr_program_destroy",
    "skr_tape_launch",
    "skr_noise_random",
    "skr_noise_offset",
    "skr_noise_offset_rolling",
    "skr_noise_offset_rolling_covers",
    "skr_noise_brownian",
    "skr_noise_pyramid",
    "skr_noise_pyramid_rolling",
    "skr_noise_pyramid_rolling_covers",
    "skr_noise_pyramid_any",
    "skr_noise_pyramid_nd",
    "skr_noise_colored",
    "skr_noise_colored_any",
    "skr_colorize",
    "skr_error_mean",
    "skr_power_blend",
    "skr_power_blend_backward",
    "skr_philox_u32",
    "skr_normal_u32",
    "skr_abi_version",
    "skr_strerror",
    "skr_last_hip_error",
    "skr_build_info",
    "skr_set_tuning",
    "skr_stat",
)


class SkrampleHipError(RuntimeError):
    "The HIP engine is unavailable or rejected a request.  Never silently degraded."


class StepPlanC(ctypes.Structure):
    "mirror of `skr_step_plan`"

    _fields_ = [
        ("n_terms", ctypes.c_int32),
        ("n_group_a", ctypes.c_int32),
        ("dtype_a", ctypes.c_int32),
        ("dtype_b", ctypes.c_int32),
        ("out0_dtype", ctypes.c_int32),
        ("out1_dtype", ctypes.c_int32),
        ("acc_f64", ctypes.c_int32),
        ("noise_mode", ctypes.c_int32),
        ("coef0", ctypes.c_double * MAX_TERMS),
        ("coef1", ctypes.c_double * MAX_TERMS),
        ("chain", ctypes.c_double),
        ("zeta0", ctypes.c_double),
        ("zeta1", ctypes.c_double),
        ("stream0", ctypes.c_uint64),
        ("stream1", ctypes.c_uint64),
        ("sample_numel", ctypes.c_int64),
        ("convert_to", ctypes.c_int32),
        ("convert_from", ctypes.c_int32),
        ("convert_k", ctypes.c_double * 4),
    ]


class StepLayoutC(ctypes.Structure):
    "mirror of `skr_step_layout`: a sample stored as plane x channels elements, channel innermost"

    _fields_ = [("channels", ctypes.c_int64), ("plane", ctypes.c_int64)]


class StepGradPlanC(ctypes.Structure):
    "mirror of `skr_step_grad_plan`"

    _fields_ = [
        ("n_grads", ctypes.c_int32),
        ("n_group_a", ctypes.c_int32),
        ("dtype_a", ctypes.c_int32),
        ("dtype_b", ctypes.c_int32),
        ("g0_dtype", ctypes.c_int32),
        ("g1_dtype", ctypes.c_int32),
        ("acc_f64", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("a", ctypes.c_double * MAX_TERMS),
        ("b", ctypes.c_double * MAX_TERMS),
    ]


TAPE_MAX_OPS, TAPE_REGS, TAPE_MAX_INPUTS, TAPE_MAX_OUTPUTS = 96, 16, 24, 4  # include/skrample_hip.h SKR_TAPE_*
(TAPE_LOAD, TAPE_STORE, TAPE_MUL_S, TAPE_DIV_S, TAPE_ADD_S, TAPE_RSUB_S, TAPE_RDIV_S, TAPE_ADD, TAPE_SUB, TAPE_MUL, TAPE_DIV, TAPE_NEG,
 TAPE_ADD_MS, TAPE_SUB_MS, TAPE_RSUB_MS, TAPE_MULZ_S) = range(16)  # fmt: skip


class TapeOpC(ctypes.Structure):
    "mirror of `skr_tape_op`"

    _fields_ = [("code", ctypes.c_int32), ("dst", ctypes.c_int32), ("a", ctypes.c_int32), ("b", ctypes.c_int32), ("k", ctypes.c_double)]


class TapeC(ctypes.Structure):
    "mirror of `skr_tape`"

    _fields_ = [("n_ops", ctypes.c_int32), ("n_inputs", ctypes.c_int32), ("n_outputs", ctypes.c_int32), ("dtype", ctypes.c_int32), ("ops", TapeOpC * TAPE_MAX_OPS)]


ROW_TERMS = 16  # include/skrample_hip.h SKR_ROW_TERMS
PER_SAMPLE_CHUNK = 2048  # elements per workgroup of the one-trip kernels: a sample of a per-sample launch is made of whole ones


def ragged_sample(sample_numel: int) -> bool:
    """a sample the ragged form of the table launches takes (include/skrample_hip.h, "ragged samples"): at least one chunk, a multiple
    of 8 elements, not whole chunks -- its last workgroup is partly empty"""
    return PER_SAMPLE_CHUNK <= sample_numel < 2**31 and sample_numel % 8 == 0 and sample_numel % PER_SAMPLE_CHUNK != 0


def one_dtype_f32(plan: "StepPlanC", *also: int) -> bool:
    """THE coverage rule of the masked, guided and ragged row kernels, the one place it is written: the operands of both groups, the first
    output and `also` (dtype codes: a mask's, a batch's) are one 16- or 32-bit dtype, evaluated in float32"""
    one = plan.dtype_a
    return (one in (BF16, F16, F32) and plan.out0_dtype == one and (plan.n_group_a == plan.n_terms or plan.dtype_b == one)
            and all(code == one for code in also) and not plan.acc_f64)  # fmt: skip


def one_group_launch(plan: "StepPlanC", *also: int) -> bool:
    "what a masked or guided rolling batch steps with: one single-output launch of one operand group under the coverage rule"
    return plan.out1_dtype == NONE and plan.n_group_a == plan.n_terms and one_dtype_f32(plan, *also)


def single_output_plan(plan: "StepPlanC") -> bool:
    "what a ragged launch must be: one output under the coverage rule, no rounded conversion, 1..ROW_TERMS operands"
    return plan.out1_dtype == NONE and one_dtype_f32(plan) and not plan.convert_to and not plan.convert_from and 1 <= plan.n_terms <= ROW_TERMS


RAGGED_SINGLE_OUTPUT = ("ragged samples (not whole 2048-element chunks) are served for single-output launches only -- Euler, DPM, Adams and UniP steps in one 16- or "
                        "32-bit dtype under the default compute scale; the two-output (UniPC, SPC), Runge-Kutta, masked and guided row kernels need whole chunks")


class StepRowC(ctypes.Structure):
    "mirror of `skr_step_row`: the scalars of one launch, resident on the device for indexed launches"

    _fields_ = [
        ("coef0", ctypes.c_double * ROW_TERMS),
        ("coef1", ctypes.c_double * ROW_TERMS),
        ("chain", ctypes.c_double),
        ("zeta0", ctypes.c_double),
        ("zeta1", ctypes.c_double),
        ("stream0", ctypes.c_uint64),
        ("stream1", ctypes.c_uint64),
        ("convert_k", ctypes.c_double * 4),
    ]


class StepMaskC(ctypes.Structure):
    "mirror of `skr_step_mask`: the keep-region mask of a masked step launch"

    _fields_ = [
        ("mask", ctypes.c_void_p),
        ("dtype", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("mask_numel", ctypes.c_int64),
        ("batch_stride", ctypes.c_int64),
    ]


class StepGuidanceC(ctypes.Structure):
    "mirror of `skr_step_guidance`: the second network output, the scale and the operand a guided step launch replaces"

    _fields_ = [
        ("cond", ctypes.c_void_p),
        ("guided_out", ctypes.c_void_p),
        ("scale", ctypes.c_double),
        ("slot", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class StepRescaleC(ctypes.Structure):
    "mirror of `skr_step_rescale`: the per-sample factor of the statistics launch, guidance_rescale and the statistic's sample size"

    _fields_ = [
        ("factor_dev", ctypes.c_void_p),
        ("phi", ctypes.c_double),
        ("sample_numel", ctypes.c_int64),
        ("reserved", ctypes.c_int64),
    ]


GUIDANCE_SPAN = 2048  # elements per partial sum of skr_guidance_rescale_factor (SKR_GUIDANCE_PARTIALS)


def guidance_partials(numel: int, sample_numel: int) -> int:
    "doubles of workspace skr_guidance_rescale_factor needs (include/skrample_hip.h, SKR_GUIDANCE_PARTIALS)"
    return 4 * (numel // sample_numel) * ((sample_numel + GUIDANCE_SPAN - 1) // GUIDANCE_SPAN)


# The launch table.  A launch has a KIND -- what it computes -- and a FORM -- where its scalars and its layout come from; the C entry's name
# and its argument list follow from the two by ONE rule, which the prototypes (load()), every launcher of the package (launch_call,
# IndexedRows.launch, rolling.RollingBatch._launch) and the tests read.  A new kind or form is a row here.
FACTOR = "guidance_factor"  # the statistics launch of rescaled guidance: a kind of its own, with arguments of its own
STEP_KINDS = {"plain": ("out1",), "masked": ("mask",), "guided": ("guide",), "guided_rescaled": ("guide", "rescale")}  # kind -> what follows out0
FORMS = ("direct", "channels_last", "indexed", "indexed_per_sample", "rolling")
_vp, _i64, _i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
ARGTYPES = {"plan": ctypes.POINTER(StepPlanC), "operands": ctypes.POINTER(_vp), "out0": _vp, "out1": _vp, "mask": ctypes.POINTER(StepMaskC),
            "guide": ctypes.POINTER(StepGuidanceC), "rescale": ctypes.POINTER(StepRescaleC), "seeds": _vp, "layout": ctypes.POINTER(StepLayoutC), "numel": _i64,
            "rows": _vp, "index": _vp, "row_offset": _i32, "stream": _vp,
            "uncond": _vp, "cond": _vp, "dtype": _i32, "scale": ctypes.c_double, "sample_numel": _i64, "factor": _vp, "stats": _vp, "partials": _vp}  # fmt: skip


def _entry(kind: str, form: str) -> "tuple[str, tuple[str, ...]] | None":
    "the rule: (C entry name, argument names in order) of a kind in a form, None for a combination the library does not have"
    table = ("rows", "index", "row_offset") if form in FORMS[2:] else ()
    suffix = "" if form == "direct" else "_" + form
    if kind == FACTOR:  # (the scale is a row value in the table forms)
        names = ("uncond", "cond", "dtype", *(() if table else ("scale",)), "numel", "sample_numel", *table, "factor", "stats", "partials", "stream")
        return None if form == "channels_last" else ("skr_guidance_rescale_factor" + suffix, names)
    if form == "channels_last" and kind not in ("plain", "masked"):
        return None
    layout = ("layout",) if form == "channels_last" else ()
    return ("skr_step_launch" + ("" if kind == "plain" else "_" + kind) + suffix, ("plan", "operands", "out0", *STEP_KINDS[kind], "seeds", *layout, "numel", *table, "stream"))


ENTRIES = {key: found for key in ((kind, form) for kind in (*STEP_KINDS, FACTOR) for form in FORMS) if (found := _entry(*key)) is not None}
BY_REFERENCE = {"plan", "mask", "guide", "rescale", "layout"}  # callers hand over the structure, the entry takes its address
# per key: (name, the arguments picked from a dict of values in one call, the positions that go by reference)
_LAID_OUT = {key: (name, operator.itemgetter(*names), tuple(i for i, n in enumerate(names) if n in BY_REFERENCE)) for key, (name, names) in ENTRIES.items()}


def _lay_out(kind: str, form: str, values: dict) -> "tuple[str, list]":
    try:
        name, pick, references = _LAID_OUT[kind, form]
    except KeyError:  # a combination the library does not have is an error, never another route
        raise SkrampleHipError(f"the library has no {form} form of a {kind} launch") from None
    args = list(pick(values))
    for i in references:
        args[i] = ctypes.byref(args[i])
    return name, args


def entry_name(kind: str, form: str) -> str:
    "the C entry of a kind of launch in a form"
    if (kind, form) not in ENTRIES:
        raise SkrampleHipError(f"the library has no {form} form of a {kind} launch")
    return ENTRIES[kind, form][0]


def entry_args(kind: str, form: str, **values) -> list:
    "the arguments of that entry from values by name (structures go by reference); names the entry does not take are ignored"
    return _lay_out(kind, form, values)[1]


def call_entry(lib, kind: str, form: str, values: dict) -> int:
    "one call of the entry, looked up in `lib` by name at call time, on the arguments `values` names; returns the status"
    name, args = _lay_out(kind, form, values)
    return getattr(lib, name)(*args)


def plan_structure(plan: StepPlanC, sample_numel: bool = True, mask: "StepMaskC | None" = None, guide: "StepGuidanceC | None" = None,
                   rescale: "StepRescaleC | None" = None) -> tuple:
    """what a captured launch freezes: everything of a plan except the scalars a row carries (`sample_numel` = False: and the sample size).
    A masked launch (`mask`: its descriptor) adds that it is one, the mask's dtype and whether one mask serves the whole batch
    (batch_stride == 0), and -- shape-like, dropped with the sample size -- the mask's elements per sample.
    A guided launch (`guide`: its descriptor) adds that it is one, the operand the guided value replaces (`slot`) and whether that value
    is stored; its scale is a row value.  `rescale` (a rescaled guided launch: its descriptor) adds nothing: phi is a row value as well and
    the factor a buffer of the hook, so the plain and the rescaled guided launch of a step are ONE structure -- a refill may move a slot
    between guidance_rescale == 0 and != 0."""
    plain = (plan.n_terms, plan.n_group_a, plan.dtype_a, plan.dtype_b, plan.out0_dtype, plan.out1_dtype, plan.acc_f64, plan.noise_mode,
             plan.sample_numel if sample_numel else None, plan.convert_to, plan.convert_from)  # fmt: skip
    if guide is not None:
        return (*plain, "guided", guide.slot, bool(guide.guided_out))
    if mask is None:
        return plain
    return (*plain, "masked", mask.dtype, mask.batch_stride == 0, mask.mask_numel if sample_numel else None)


def upload_rows(rows_dev: torch.Tensor, first_row: int, rows) -> None:
    "copy `rows` (StepRowC) into the device table `rows_dev` (uint8) from row `first_row` on (stream-ordered)"
    blob = b"".join(bytes(r) for r in rows)
    at = first_row * ctypes.sizeof(StepRowC)
    rows_dev[at : at + len(blob)].copy_(torch.frombuffer(bytearray(blob), dtype=torch.uint8), non_blocking=False)


class IndexedRows:
    """Device-resident step scalars of a captured sampling loop (skr_step_launch_indexed).

    `batch` (a per-sample capture): the emitted launches are skr_step_launch_indexed_per_sample launches, and `sample_index_dev`
    -- int32[batch], beside `index_dev` -- holds every sample's `slot * length`; sample b of the captured batch reads row
    `sample_index_dev[b] + k`.
    `guided` (a capture with guidance): guided launches go through the recorder as well (skr_step_launch_guided_indexed[_per_sample]),
    each row carrying its launch's guidance scale.
    `rescaled` (with `guided`; `samples`: the captured batch): rescaled guided launches go through it too, each row carrying
    guidance_rescale in convert_k[1] -- 0.0 for a plain guided launch.  Every emitted guided step is then TWO launches on buffers the hook
    owns (`factor`, `partials`: allocated in the recording pass, the same in every step of the graph), with the same row offset:
    skr_guidance_rescale_factor_indexed[_per_sample], then skr_step_launch_guided_rescaled_indexed[_per_sample] -- whether or not the
    recording pass rescaled, since a row with phi == 0 makes the first return at once and the second the plain guided step.

    Ragged samples (at least one 2048-element chunk, a multiple of 8 elements, not whole chunks): plain single-output launches are
    recorded and emitted as they stand -- the row entries take the ragged form themselves --; a whole-batch capture needs `samples` for
    that, to give a launch without noise the sample size it does not carry.  Any other launch on ragged samples is refused while
    recording, before a stream captures.

    mode "record": launches run normally and append one row each (their structure is remembered);
    mode "emit"  : launches become indexed launches reading row `base + k` (k = position in the loop) -- used under graph capture;
    mode "refill": launches run normally (on whatever tensors the dry run uses) and overwrite row `slot*length + k` after checking
                   that the structure is the captured one -- how a captured loop is re-targeted to another schedule."""

    def __init__(self, device: torch.device, slots: int = 4, batch: int | None = None, guided: bool = False, rescaled: bool = False, samples: int | None = None):
        if rescaled and not guided:
            raise ValueError("rescaled=True needs guided=True: guidance_rescale is applied to the guided prediction a guided launch forms")
        if rescaled and (samples is None or samples < 1):
            raise ValueError("rescaled=True needs samples=: the captured batch, one factor per sample")
        if rescaled and batch is not None and batch != samples:
            raise ValueError(f"a per-sample capture of {batch} samples cannot hold factors for {samples}")
        self.device, self.slots, self.batch = device, slots, batch
        # a capture with rescaled guidance: the factor T[samples] and the partials workspace of every emitted statistics launch
        self.rescaled, self.samples = rescaled, samples
        self.factor: torch.Tensor | None = None
        self.partials: torch.Tensor | None = None
        # a capture with guidance: launch_step_guided goes through this hook (skr_step_launch_guided_indexed[_per_sample]), and a row
        # carries the guidance scale in convert_k[0]; any other hook refuses a guided launch
        self.guided = guided
        self.mode, self.cursor, self.length = "record", 0, 0
        self.structures: list[tuple] = []  # plan_structure of every recorded launch,
        self.shapeless: list[tuple] = []  # and without its sample size (what a refill must match)
        self.host: list[StepRowC] = []
        self.rows_dev: torch.Tensor | None = None
        self.index_dev = torch.zeros(1, dtype=torch.int32, device=device)
        self.sample_index_dev = torch.zeros(batch, dtype=torch.int32, device=device) if batch is not None else None
        self.slot = 0

    @staticmethod
    def row_from(plan: StepPlanC, scale: float | None = None, phi: float | None = None) -> StepRowC:
        """the row of a launch; `scale`: a guided one's guidance scale, kept in convert_k[0] (such a plan has no rounded conversion);
        `phi` (a hook created with `rescaled`): its guidance_rescale, kept in convert_k[1] -- 0.0 for a plain guided launch"""
        if plan.n_terms > ROW_TERMS:
            raise SkrampleHipError(f"a launch with {plan.n_terms} operands does not fit a device-resident row ({ROW_TERMS})")
        row = StepRowC()
        for k in range(plan.n_terms):
            row.coef0[k], row.coef1[k] = plan.coef0[k], plan.coef1[k]
        row.chain, row.zeta0, row.zeta1, row.stream0, row.stream1 = plan.chain, plan.zeta0, plan.zeta1, plan.stream0, plan.stream1
        for k in range(4):
            row.convert_k[k] = plan.convert_k[k]
        if scale is not None:
            row.convert_k[0] = scale
        if phi is not None:
            row.convert_k[1] = phi
        return row

    def finish_recording(self) -> None:
        self.length = len(self.host)
        size = ctypes.sizeof(StepRowC)
        self.rows_dev = torch.zeros(self.slots * self.length * size, dtype=torch.uint8, device=self.device)
        self.upload(0)

    def upload(self, slot: int) -> None:
        "copy the host rows of `slot` to the device (stream-ordered)"
        upload_rows(self.rows_dev, slot * self.length, self.host[slot * self.length : (slot + 1) * self.length])

    def sample_indices(self, sample_slots) -> torch.Tensor:
        "host int32[batch] of `slot * length`: what `sample_index_dev` must hold for the samples to follow these slots"
        return torch.as_tensor(list(sample_slots), dtype=torch.int64).mul(self.length).to(torch.int32)

    def select(self, sample_slots) -> None:
        "publish the slot of every sample (validated by the caller): one small stream-ordered host-to-device copy"
        self.sample_index_dev.copy_(self.sample_indices(sample_slots))

    def begin(self, mode: str, slot: int = 0) -> None:
        self.mode, self.cursor, self.slot = mode, 0, slot
        if mode == "refill":
            need = (slot + 1) * self.length
            while len(self.host) < need:
                self.host.append(StepRowC())

    def _uncovered(self, plan: StepPlanC, mask: "StepMaskC", numel: int) -> str | None:
        "why the masked row kernel does not cover this launch (include/skrample_hip.h, skr_step_launch_masked_indexed), or None"
        if plan.acc_f64:
            return "masked rows are evaluated in float32, not under compute_scale=float64"
        if not one_dtype_f32(plan, mask.dtype):
            return "masked rows need one 16- or 32-bit dtype for operands, mask and output"
        if plan.sample_numel <= 0 or plan.sample_numel % PER_SAMPLE_CHUNK != 0 or numel % PER_SAMPLE_CHUNK != 0:
            return f"masked rows need samples of whole {PER_SAMPLE_CHUNK}-element chunks, not {plan.sample_numel} elements"
        if mask.mask_numel % 8 != 0:
            return f"masked rows need a mask of a multiple of 8 elements per sample, not {mask.mask_numel}"
        if plan.n_terms < 1:
            return "masked rows need at least one operand"
        return None

    def _uncovered_guided(self, plan: StepPlanC, numel: int) -> str | None:
        "why the guided row kernel does not cover this launch (include/skrample_hip.h, skr_step_launch_guided_indexed), or None"
        if plan.out0_dtype == NONE:
            return ("the guidance-only launch has no row form: it serves the two-output samplers (UniPC, SPC), a guided step under set_inpaint, "
                    "compute_scale=None and channels-last or strided operands")
        if plan.acc_f64:
            return "guided rows are evaluated in float32, not under compute_scale=float64"
        if not one_dtype_f32(plan):
            return "guided rows need one 16- or 32-bit dtype for operands, cond and both outputs"
        if numel % PER_SAMPLE_CHUNK != 0 or (plan.noise_mode == 1 and (plan.sample_numel <= 0 or plan.sample_numel % PER_SAMPLE_CHUNK != 0)):
            return f"guided rows need whole {PER_SAMPLE_CHUNK}-element chunks, not {numel} elements in samples of {plan.sample_numel}"
        if plan.n_terms < 1:
            return "guided rows need at least one operand"
        return None

    def _ragged_whole_batch(self, plan: StepPlanC, numel: int) -> bool:
        """a plain launch of a whole-batch capture that only the ragged form of skr_step_launch_indexed takes: ragged samples -- the plan's,
        or the captured batch's (`samples`) for a launch that carries no sample size -- and a draw, or a launch that is not whole chunks"""
        samples = getattr(self, "samples", None)
        per = plan.sample_numel if plan.sample_numel > 0 else (numel // samples if samples and numel % samples == 0 else 0)
        return ragged_sample(per) and numel % per == 0 and (plan.noise_mode == 1 or numel % PER_SAMPLE_CHUNK != 0)

    def _uncovered_rescaled(self, plan: StepPlanC, numel: int) -> str | None:
        "why the rescaled guided row kernels do not cover this launch of the captured batch (skr_step_launch_guided_rescaled_indexed), or None"
        if numel % self.samples != 0 or (numel // self.samples) % PER_SAMPLE_CHUNK != 0:
            return f"rescaled guided rows need samples of whole {PER_SAMPLE_CHUNK}-element chunks, not {numel} elements for {self.samples} samples"
        if plan.sample_numel > 0 and plan.sample_numel != numel // self.samples:
            return f"rescaled guided rows take the statistic over the samples the noise is drawn by: {numel // self.samples} elements, not {plan.sample_numel}"
        return None

    def launch(self, lib, plan: StepPlanC, arr, out0_ptr, out1_ptr, seeds_ptr, numel: int, stream_ptr: int, mask: "StepMaskC | None" = None,
               guide: "StepGuidanceC | None" = None, rescale: "StepRescaleC | None" = None) -> int:
        """one launch of the loop; `mask` (its descriptor): a masked one (skr_step_launch_masked and its row forms; out1_ptr is None);
        `guide` (its descriptor): a guided one (skr_step_launch_guided and its row forms; out1_ptr is None), whose scale goes into the row;
        `rescale` (with `guide`, under a hook created with `rescaled`): a rescaled guided one, whose phi goes into the row as well"""
        k = self.cursor
        self.cursor += 1
        scale = guide.scale if guide is not None else None
        phi = None
        rescaled = guide is not None and getattr(self, "rescaled", False)  # (a recorder put together without the constructor has no such field)
        if rescaled:
            phi = rescale.phi if rescale is not None else 0.0  # (a plain guided launch is what the wrapper issues for guidance_rescale == 0)
        kind = "guided_rescaled" if rescale is not None else "guided" if guide is not None else "masked" if mask is not None else "plain"
        values = dict(plan=plan, operands=arr, out0=out0_ptr, out1=out1_ptr, mask=mask, guide=guide, rescale=rescale, seeds=seeds_ptr, numel=numel, stream=stream_ptr)
        if self.mode == "record":
            plain = mask is None and guide is None
            if self.batch is not None and (numel % self.batch != 0 or (numel // self.batch) % PER_SAMPLE_CHUNK != 0):
                # (what skr_step_launch_indexed_per_sample would answer during the capture: said here, before a stream is capturing)
                if not (plain and numel % self.batch == 0 and ragged_sample(numel // self.batch)):
                    raise SkrampleHipError(f"launch {k}: {lib.skr_strerror(SKR_ERR_UNSUPPORTED).decode()}: per-sample rows need samples of whole {PER_SAMPLE_CHUNK}-element chunks, "
                                           f"not {numel} elements for {self.batch} samples")
                if not single_output_plan(plan):
                    raise SkrampleHipError(f"launch {k}: {lib.skr_strerror(SKR_ERR_UNSUPPORTED).decode()}: {RAGGED_SINGLE_OUTPUT}")
            if self.batch is None and plain and self._ragged_whole_batch(plan, numel) and not single_output_plan(plan):
                # (what skr_step_launch_indexed would answer during the capture)
                raise SkrampleHipError(f"launch {k}: {lib.skr_strerror(SKR_ERR_UNSUPPORTED).decode()}: {RAGGED_SINGLE_OUTPUT}")
            if mask is not None:
                why = self._uncovered(plan, mask, numel)
                if why is not None:  # (what skr_step_launch_masked_indexed would answer during the capture)
                    raise SkrampleHipError(f"launch {k}: {lib.skr_strerror(SKR_ERR_UNSUPPORTED).decode()}: {why}")
            if guide is not None:
                why = self._uncovered_guided(plan, numel)
                if why is not None:  # (what skr_step_launch_guided_indexed would answer during the capture)
                    raise SkrampleHipError(f"launch {k}: {lib.skr_strerror(SKR_ERR_UNSUPPORTED).decode()}: {why}")
                if rescaled:
                    why = self._uncovered_rescaled(plan, numel)
                    if why is not None:  # (what skr_step_launch_guided_rescaled_indexed would answer during the capture)
                        raise SkrampleHipError(f"launch {k}: {lib.skr_strerror(SKR_ERR_UNSUPPORTED).decode()}: {why}")
                    if self.factor is None:  # allocated here, before a stream captures; every emitted step of the graph uses these two
                        self.factor = torch.zeros(self.samples, dtype=CODE_DTYPE[plan.dtype_a], device=self.device)
                        self.partials = torch.zeros(guidance_partials(numel, numel // self.samples), dtype=torch.float64, device=self.device)
                    elif self.factor.dtype != CODE_DTYPE[plan.dtype_a] or self.partials.numel() != guidance_partials(numel, numel // self.samples):
                        raise SkrampleHipError(f"launch {k}: the guided steps of one rescaled capture share one factor and one workspace: one dtype and one size")
            row = self.row_from(plan, scale, phi)
            self.structures.append(plan_structure(plan, mask=mask, guide=guide, rescale=rescale))
            self.shapeless.append(plan_structure(plan, sample_numel=False, mask=mask, guide=guide, rescale=rescale))
            self.host.append(row)
            return call_entry(lib, kind, "direct", values)  # the launch itself, with the plan's own scalars
        if k >= self.length:
            raise SkrampleHipError("more launches than the captured loop has")
        if self.mode == "refill":
            found = plan_structure(plan, sample_numel=False, mask=mask, guide=guide, rescale=rescale)
            if mask is not None and len(found) == len(self.shapeless[k]) and numel == plan.sample_numel:
                found = (*found[:-2], self.shapeless[k][-2], found[-1])  # (a dry run on one sample has no batch stride to compare)
            if found != self.shapeless[k]:
                raise SkrampleHipError(f"launch {k} of the new schedule has a different structure than the captured loop: re-capture")
            self.host[self.slot * self.length + k] = self.row_from(plan, scale, phi)
            return call_entry(lib, kind, "direct", values)  # the launch itself, with the plan's own scalars
        if plan_structure(plan, mask=mask, guide=guide, rescale=rescale) != self.structures[k]:
            raise SkrampleHipError(f"launch {k} differs in structure between the recording pass and the capture")
        # emit: the row form of the launch, reading row `k` behind the loop's slot (or behind every sample's own)
        per_sample = self.sample_index_dev is not None
        form = "indexed_per_sample" if per_sample else "indexed"
        values.update(rows=self.rows_dev.data_ptr(), index=(self.sample_index_dev if per_sample else self.index_dev).data_ptr(), row_offset=k)
        if rescaled or per_sample:
            count, holder = (self.samples, "factor") if rescaled else (self.batch, "per-sample index")
            if plan.sample_numel <= 0:  # (a launch without noise carries no sample size: the captured batch gives it)
                plan = values["plan"] = StepPlanC.from_buffer_copy(plan)
                plan.sample_numel = numel // count
            if numel != count * plan.sample_numel:
                raise SkrampleHipError(f"launch {k} covers {numel} elements, not the {count} samples of {plan.sample_numel} the {holder} holds")
        elif kind == "plain" and plan.sample_numel <= 0 and self._ragged_whole_batch(plan, numel):
            # (a launch without noise carries no sample size; one that is not whole chunks takes the ragged form, which needs it: the captured batch gives it)
            plan = values["plan"] = StepPlanC.from_buffer_copy(plan)
            plan.sample_numel = numel // self.samples
        if rescaled:
            # the two launches of a guided step of a rescaled capture, on the hook's factor and partials and with the same row offset: the statistics
            # row launch over (inputs[slot], cond), then the rescaled row step.  A row with phi == 0 makes the first return before it reads
            # anything and the second the plain guided step.
            per = numel // self.samples
            status = call_entry(lib, FACTOR, form, dict(values, uncond=arr[guide.slot], cond=guide.cond, dtype=plan.dtype_a, sample_numel=per, factor=self.factor.data_ptr(),
                                                        stats=None, partials=self.partials.data_ptr()))  # fmt: skip
            if status != 0:
                return status
            kind, values["rescale"] = "guided_rescaled", StepRescaleC(self.factor.data_ptr(), 0.0, per, 0)  # (phi is the row's)
        return call_entry(lib, kind, form, values)


# Launch hooks, PER THREAD (a scheduler instance is single-threaded by contract, but several may run in different threads of one
# process, and a hook installed by one of them must not record or redirect the launches of another):
#   _hip.indexed  IndexedRows | None   installed by skrample_amd.graphs while it records / captures / re-targets a loop
#   _hip.trace    list | None          launches are appended while a wrapper lowers a step program (sampling/program.py)
# Both read and assign like plain module attributes (`_hip.trace = []`); the module's class routes them to thread-local storage.
_hooks = threading.local()


class _HipModule(type(sys)):
    @property
    def indexed(self) -> "IndexedRows | None":
        return getattr(_hooks, "indexed", None)

    @indexed.setter
    def indexed(self, value) -> None:
        _hooks.indexed = value

    @property
    def trace(self) -> "list | None":
        return getattr(_hooks, "trace", None)

    @trace.setter
    def trace(self, value) -> None:
        _hooks.trace = value


sys.modules[__name__].__class__ = _HipModule


def hooks_clear() -> bool:
    "no launch hook installed on this thread (the replayed-step fast path launches by program handle, which the hooks do not see)"
    return getattr(_hooks, "indexed", None) is None and getattr(_hooks, "trace", None) is None


def step_launch_raw(plan: StepPlanC, arr, out0_ptr, out1_ptr, seeds_ptr, numel: int, stream_ptr: int) -> int:
    "every skr_step_launch of the package goes through here (status returned, not checked)"
    lib = load()
    rows = getattr(_hooks, "indexed", None)
    if rows is not None:
        return rows.launch(lib, plan, arr, out0_ptr, out1_ptr, seeds_ptr, numel, stream_ptr)
    return lib.skr_step_launch(ctypes.byref(plan), arr, out0_ptr, out1_ptr, seeds_ptr, numel, stream_ptr)


_lock = threading.Lock()
_lib: ctypes.CDLL | None = None


def load() -> ctypes.CDLL:
    "dlopen the engine (once) and declare the prototypes"
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.isfile(LIB_PATH):
            raise SkrampleHipError(
                f"{LIB_PATH} not found: the HIP extension is not built. "
                "Run `python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
                "skrample_amd has no CPU fallback."
            )
        try:
            lib = ctypes.CDLL(LIB_PATH)
        except OSError as exc:  # pragma: no cover - depends on the box
            raise SkrampleHipError(f"cannot load {LIB_PATH}: {exc}") from exc
        vp, i64, u64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int32
        for name, names in ENTRIES.values():  # the step launches and the guidance statistics: prototypes from the table's one rule
            entry = getattr(lib, name)
            entry.argtypes, entry.restype = [ARGTYPES[n] for n in names], ctypes.c_int
        lib.skr_rolling_advance.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp]
        lib.skr_rolling_advance.restype = ctypes.c_int
        lib.skr_step_backward_launch.argtypes = [ctypes.POINTER(StepGradPlanC), vp, vp, ctypes.POINTER(vp), i64, vp]
        lib.skr_step_backward_launch.restype = ctypes.c_int
        lib.skr_step_masked_backward_launch.argtypes = [ctypes.POINTER(StepGradPlanC), vp, ctypes.POINTER(StepMaskC), ctypes.POINTER(vp), i64, i64, vp]
        lib.skr_step_masked_backward_launch.restype = ctypes.c_int
        lib.skr_program_create.argtypes = [ctypes.POINTER(StepPlanC), i64, ctypes.POINTER(vp)]
        lib.skr_program_create.restype = ctypes.c_int
        lib.skr_program_create_channels_last.argtypes = [ctypes.POINTER(StepPlanC), i64, ctypes.POINTER(StepLayoutC), ctypes.POINTER(vp)]
        lib.skr_program_create_channels_last.restype = ctypes.c_int
        lib.skr_program_launch.argtypes = [vp, ctypes.POINTER(vp), vp, vp, vp, u64, u64, vp]
        lib.skr_program_launch.restype = ctypes.c_int
        lib.skr_program_destroy.argtypes = [vp]
        lib.skr_program_destroy.restype = None
        lib.skr_tape_launch.argtypes = [ctypes.POINTER(TapeC), ctypes.POINTER(vp), ctypes.POINTER(vp), i64, vp]
        lib.skr_tape_launch.restype = ctypes.c_int
        lib.skr_noise_random.argtypes = [vp, i32, vp, u64, i64, i64, vp]
        lib.skr_noise_random.restype = ctypes.c_int
        lib.skr_noise_offset.argtypes = [vp, i32, vp, u64, u64, i64, ctypes.POINTER(i64), i32, ctypes.c_uint32, ctypes.c_double, vp]
        lib.skr_noise_offset.restype = ctypes.c_int
        lib.skr_noise_offset_rolling.argtypes = [vp, i32, vp, vp, i32, u64, i32, i64, ctypes.POINTER(i64), i32, ctypes.c_uint32, ctypes.c_double, vp]
        lib.skr_noise_offset_rolling.restype = ctypes.c_int
        lib.skr_noise_offset_rolling_covers.argtypes = [i64, ctypes.POINTER(i64), i32]
        lib.skr_noise_offset_rolling_covers.restype = ctypes.c_int
        lib.skr_noise_brownian.argtypes = [vp, i32, vp, ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), i32, ctypes.c_double, vp, i32, i64, i64, vp]
        lib.skr_noise_brownian.restype = ctypes.c_int
        lib.skr_noise_pyramid.argtypes = [vp, i32, vp, vp, vp, vp, u64, u64, i64, i64, i64, i64, i32, ctypes.c_double, i32, i32, vp]
        lib.skr_noise_pyramid.restype = ctypes.c_int
        lib.skr_noise_pyramid_rolling.argtypes = [vp, i32, vp, vp, vp, vp, vp, i32, u64, i32, i64, i64, i64, i64, i32, ctypes.c_double, i32, vp]
        lib.skr_noise_pyramid_rolling.restype = ctypes.c_int
        lib.skr_noise_pyramid_rolling_covers.argtypes = [i64, i64, i64, i64, i32]
        lib.skr_noise_pyramid_rolling_covers.restype = ctypes.c_int
        lib.skr_noise_pyramid_any.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, u64, u64, i64, i64, i64, i64, i32, ctypes.c_double, i32, i32, vp]
        lib.skr_noise_pyramid_any.restype = ctypes.c_int
        lib.skr_noise_pyramid_nd.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, u64, u64, i64, i32, ctypes.POINTER(i64), i32, i32, ctypes.c_double, i32, i32, vp]
        lib.skr_noise_pyramid_nd.restype = ctypes.c_int
        lib.skr_noise_colored.argtypes = [vp, i32, vp, vp, vp, i64, vp, u64, i64, i32, i32, i32, ctypes.c_double, i32, ctypes.c_double, vp]
        lib.skr_noise_colored.restype = ctypes.c_int
        lib.skr_noise_colored_any.argtypes = [vp, i32, vp, vp, vp, vp, u64, i64, i32, ctypes.POINTER(i32), ctypes.c_double, i32, ctypes.c_double, vp]
        lib.skr_noise_colored_any.restype = ctypes.c_int
        lib.skr_colorize.argtypes = [vp, i32, vp, vp, vp, i64, i32, ctypes.POINTER(i32), ctypes.c_double, i32, ctypes.c_double, vp]
        lib.skr_colorize.restype = ctypes.c_int
        lib.skr_error_mean.argtypes = [vp, vp, i32, i64, i32, vp, vp, vp]
        lib.skr_error_mean.restype = ctypes.c_int
        lib.skr_philox_u32.argtypes = [vp, u64, u64, u64, i64, vp]
        lib.skr_philox_u32.restype = ctypes.c_int
        lib.skr_normal_u32.argtypes = [vp, vp, i64, i32, vp]
        lib.skr_normal_u32.restype = ctypes.c_int
        lib.skr_power_blend.argtypes = [vp, i32, vp, i32, vp, i32, ctypes.c_double, ctypes.c_double, ctypes.c_double, i64, vp]
        lib.skr_power_blend.restype = ctypes.c_int
        lib.skr_power_blend_backward.argtypes = [vp, vp, vp, i32, vp, i32, vp, i32, ctypes.c_double, ctypes.c_double, ctypes.c_double, i64, vp]
        lib.skr_power_blend_backward.restype = ctypes.c_int
        lib.skr_abi_version.restype = ctypes.c_int
        lib.skr_strerror.argtypes = [ctypes.c_int]
        lib.skr_strerror.restype = ctypes.c_char_p
        lib.skr_last_hip_error.restype = ctypes.c_int
        lib.skr_build_info.restype = ctypes.c_char_p
        lib.skr_stat.argtypes = [ctypes.c_char_p]
        lib.skr_stat.restype = ctypes.c_int64
        lib.skr_set_tuning.argtypes = [ctypes.c_char_p, i32]
        lib.skr_set_tuning.restype = ctypes.c_int
        if lib.skr_abi_version() != ABI_VERSION:
            raise SkrampleHipError(f"ABI mismatch: library {lib.skr_abi_version()} != binding {ABI_VERSION}; rebuild")
        _lib = lib
        return lib


def check(status: int, what: str) -> None:
    if status != 0:
        lib = load()
        msg = lib.skr_strerror(status).decode()
        extra = f" (hipError {lib.skr_last_hip_error()})" if status == 6 else ""
        raise SkrampleHipError(f"{what}: {msg}{extra}")


def require_device(t: torch.Tensor, what: str) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise SkrampleHipError(
            f"{what} must be a torch tensor on a HIP device; skrample_amd executes on the GPU only "
            "(no CPU path). Got " + (f"{t.device}" if isinstance(t, torch.Tensor) else type(t).__name__)
        )


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)  # the handle without building a torch.cuda.Stream object (1.5 -> 0.3 us per step)


def current_stream_ptr(device: torch.device) -> int:
    "hipStream_t of torch's current stream on `device`"
    if _raw_stream is not None and device.index is not None:
        return _raw_stream(device.index)
    return torch.cuda.current_stream(device).cuda_stream


def _ptr(t):
    "`data_ptr()` of a tensor, None (a NULL argument) for None"
    return t.data_ptr() if t is not None else None


def _operand_array(tensors):
    "the operand pointer array of a step launch"
    return (ctypes.c_void_p * max(len(tensors), 1))(*[t.data_ptr() for t in tensors])


class StepCall(tuple):
    """The record of one step launch: what a `_hip.trace` list (per thread, see _HipModule) receives for it.  It IS the six-tuple
    (plan, inputs, out0, out1, seeds, numel) that the step programs, bench.py and the tools unpack to lift the exact plans the samplers emit,
    and it says what the launch is by name, never by its length: `kind` (a key of STEP_KINDS), `layout` ((channels, plane) or None: read
    off the tensors) and -- None where the kind has none -- `mask`, `mask_numel`, `batch_stride` (masked), `cond`, `guided_out`, `scale`,
    `slot` (guided), `factor`, `phi`, `sample_numel` (guided_rescaled).  A step program is built from a plain one only."""

    kind, layout = "plain", None
    mask = mask_numel = batch_stride = cond = guided_out = scale = slot = factor = phi = sample_numel = None
    plan, inputs, out0, out1, seeds, numel = (property(operator.itemgetter(i)) for i in range(6))

    def __new__(cls, plan, inputs, out0, out1, seeds, numel, kind: str = "plain", **named):
        self = tuple.__new__(cls, (plan, list(inputs), out0, out1, seeds, numel))
        if named:  # (a plain contiguous launch, the common one, is the class's defaults)
            self.__dict__.update(named, kind=kind)
        return self


class FactorCall:
    "the record of the statistics launch of rescaled guidance: no tuple and no plan, so nothing unpacks it as a step launch"

    kind, layout = FACTOR, None

    def __init__(self, uncond, cond, scale, sample_numel, factor, stats):
        self.uncond, self.cond, self.scale, self.sample_numel, self.factor, self.stats = uncond, cond, scale, sample_numel, factor, stats


NO_RESCALED_ROWS = ("rescaled guidance (guidance_rescale) has no row form in a loop captured without it: pass rescaled=True to capture_sampling_loop (guidance_rescale "
                    "is then a row value), capture the loop with indexed=False, which freezes guidance_rescale into the graph, or pass guidance_rescale=0.0")


def launch_call(call: "StepCall | FactorCall", device: torch.device) -> None:
    """THE launcher of the eager entry points: one launch on torch's current stream of `device`, from its record.  Refuses what the installed
    indexed-rows hook was not created for, appends the record to a `_hip.trace` list, builds the descriptors, hands the launch to the hook
    (IndexedRows.launch: recorded, emitted in its row form or refilled) or calls the direct / channels-last entry of the table, and checks
    the status under that entry's name."""
    lib = load()
    kind, layout = call.kind, call.layout
    rows = getattr(_hooks, "indexed", None)
    if rows is not None:
        if layout is not None:  # (the hook has no channels-last form: the caller takes the contiguous route while one is installed)
            raise SkrampleHipError("captured loops with device-resident rows take contiguous operands")
        if kind == "guided" and not getattr(rows, "guided", False):
            raise SkrampleHipError("guided steps are not part of captured loops unless the loop is captured for them: pass guidance_scale= to capture_sampling_loop")
        if kind in ("guided_rescaled", FACTOR) and not getattr(rows, "rescaled", False):
            raise SkrampleHipError(NO_RESCALED_ROWS)
    trace = getattr(_hooks, "trace", None)
    if trace is not None:
        trace.append(call)
    form = "direct" if layout is None else "channels_last"
    name = entry_name(kind, form)
    if kind == FACTOR:
        if rows is not None and rows.mode == "emit":  # (the step launch that follows emits the statistics row launch itself, on the hook's buffers)
            return
        numel = call.uncond.numel()  # (the workspace comes from torch's allocator, which is safe under graph capture)
        partials = torch.empty(max(guidance_partials(numel, call.sample_numel), 1), dtype=torch.float64, device=device)
        values = dict(uncond=call.uncond.data_ptr(), cond=call.cond.data_ptr(), dtype=DTYPE_CODE[call.uncond.dtype], scale=float(call.scale), numel=numel, sample_numel=int(call.sample_numel),
                      factor=call.factor.data_ptr(), stats=_ptr(call.stats), partials=partials.data_ptr(), stream=current_stream_ptr(device))  # fmt: skip
        return check(call_entry(lib, kind, form, values), name)
    plan, inputs, out0, out1, seeds, numel = call
    mask = StepMaskC(call.mask.data_ptr(), DTYPE_CODE[call.mask.dtype], 0, call.mask_numel, call.batch_stride) if call.mask is not None else None
    guide = StepGuidanceC(call.cond.data_ptr(), _ptr(call.guided_out), float(call.scale), int(call.slot), 0) if call.cond is not None else None
    rescale = StepRescaleC(call.factor.data_ptr(), float(call.phi), int(call.sample_numel), 0) if call.factor is not None else None
    arr, stream = _operand_array(inputs), current_stream_ptr(device)
    if rows is not None:
        status = rows.launch(lib, plan, arr, _ptr(out0), _ptr(out1), _ptr(seeds), numel, stream, mask=mask, guide=guide, rescale=rescale)
    else:
        values = dict(plan=plan, operands=arr, out0=_ptr(out0), out1=_ptr(out1), mask=mask, guide=guide, rescale=rescale, seeds=_ptr(seeds),
                      layout=StepLayoutC(*layout) if layout is not None else None, numel=numel, stream=stream)  # fmt: skip
        status = call_entry(lib, kind, form, values)
    check(status, name)


def launch_step(plan: StepPlanC, inputs: list[torch.Tensor], out0, out1, seeds, numel: int, device: torch.device, layout: tuple[int, int] | None = None) -> None:
    """one fused kernel launch (skr_step_launch).  With `layout` = (channels, plane) the operands and outputs all share that dense
    channels-last layout (skr_step_launch_channels_last)."""
    launch_call(StepCall(plan, inputs, out0, out1, seeds, numel, **({} if layout is None else {"layout": layout})), device)


def launch_step_masked(plan: StepPlanC, operands: list[torch.Tensor], out: torch.Tensor, mask: torch.Tensor, mask_numel: int, batch_stride: int, seeds, numel: int, device: torch.device,
                       layout: tuple[int, int] | None = None) -> None:
    """one masked step launch (skr_step_launch_masked): out = m * (coef0 form + noise) + (1 - m) * (coef1 form).  Under the indexed-rows
    hook it is recorded, emitted as skr_step_launch_masked_indexed[_per_sample] or refilled, as a plain step launch is.  With `layout` the
    operands and the output share that channels-last layout (skr_step_launch_masked_channels_last); `mask` stays contiguous, in logical order."""
    launch_call(StepCall(plan, operands, out, None, seeds, numel, "masked", mask=mask, mask_numel=mask_numel, batch_stride=batch_stride, layout=layout), device)


def launch_step_guided(plan: StepPlanC, operands: list[torch.Tensor], out, cond: torch.Tensor, guided_out, scale: float, slot: int, seeds, numel: int, device: torch.device) -> None:
    """one guided step launch (skr_step_launch_guided): operands[slot] is `uncond`, and the value p = uncond + scale * (cond - uncond),
    rounded as torch's three tensor ops round it, takes its place in the step's sum; `guided_out` (or None) receives p.  `out` None with a
    plan whose out0_dtype is NONE is the guidance-only form.  Under an indexed-rows hook created for a guided capture
    (IndexedRows(guided=True): capture_sampling_loop with `guidance_scale`) the launch is recorded, emitted as
    skr_step_launch_guided_indexed[_per_sample] -- the scale a row value -- or refilled.  Under any other hook it raises: that loop was
    captured without guidance."""
    launch_call(StepCall(plan, operands, out, None, seeds, numel, "guided", cond=cond, guided_out=guided_out, scale=scale, slot=slot), device)


def launch_guidance_factor(uncond: torch.Tensor, cond: torch.Tensor, scale: float, sample_numel: int, factor: torch.Tensor, stats: "torch.Tensor | None" = None) -> None:
    """the statistics launch of rescaled guidance (skr_guidance_rescale_factor): factor[s] = std(cond_s) / std(p_s) per sample of `sample_numel`
    elements in storage order, rounded as torch rounds it; `stats` (float64[2 * samples] or None) receives the two standard deviations.
    Under an indexed-rows hook created for a rescaled capture (IndexedRows(guided=True, rescaled=True)) it runs as it stands while the hook
    records or refills, and is NOT issued while the hook emits.  Under any other hook it raises."""
    launch_call(FactorCall(uncond, cond, scale, sample_numel, factor, stats), uncond.device)


def launch_step_guided_rescaled(plan: StepPlanC, operands: list[torch.Tensor], out, cond: torch.Tensor, guided_out, scale: float, slot: int, factor: torch.Tensor, phi: float,
                                sample_numel: int, seeds, numel: int, device: torch.device) -> None:
    """one rescaled guided step launch (skr_step_launch_guided_rescaled): launch_step_guided with the guided value p replaced by
    phi * (p * factor[sample]) + (1 - phi) * p, rounded as torch's four tensor ops round it; `guided_out` (or None) receives that value.
    Under an indexed-rows hook created for a rescaled capture (capture_sampling_loop with `rescaled=True`) the launch is recorded, emitted
    as skr_guidance_rescale_factor_indexed[_per_sample] plus skr_step_launch_guided_rescaled_indexed[_per_sample] -- scale and phi row
    values, `factor` replaced by the hook's own -- or refilled (IndexedRows.launch).  Under any other hook it raises."""
    launch_call(StepCall(plan, operands, out, None, seeds, numel, "guided_rescaled", cond=cond, guided_out=guided_out, scale=scale, slot=slot, factor=factor, phi=phi,
                         sample_numel=sample_numel), device)  # fmt: skip
