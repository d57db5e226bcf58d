"""Rescaled guidance in rolling batches without a GPU: the two new exports at the C boundary, the host-side checks of the built library,
and the bookkeeping of a `RollingBatch(guided=True, rescaled=True)` on stub rows (the dry run and the launches are replaced, as in
tests/test_guided_rolling_host.py: nothing here enqueues device work)."""

import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest
import torch
from conftest import ROOT

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip, rolling
from skrample_amd.rolling import RollingBatch
from skrample_amd.sampling import structured as PT

STATS, STEP = "skr_guidance_rescale_factor_rolling", "skr_step_launch_guided_rescaled_rolling"
OK, NULL, DTYPE, TERMS, ALIGN, SHAPE, LAUNCH, UNSUPPORTED = range(8)
HISTORY = [("x",), ("o",), ("po", -1), ("po", -2)]
UNIT = (4, 32, 32)


# ---- header, exports, ABI ----------------------------------------------------------------------------------------------------------
def test_header_declares_both_entries_and_the_binding_lists_them():
    header = open(os.path.join(ROOT, "include", "skrample_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    ws = r"\s*"
    stats = (r"const\s+void\s*\*\s*uncond", r"const\s+void\s*\*\s*cond", r"int32_t\s+dtype", r"int64_t\s+numel", r"int64_t\s+sample_numel",
             r"const\s+skr_step_row\s*\*\s*rows_dev", r"const\s+int32_t\s*\*\s*sample_index_dev", r"int32_t\s+row_offset", r"void\s*\*\s*factor_dev",
             r"double\s*\*\s*stats_dev", r"double\s*\*\s*partials_dev", r"void\s*\*\s*stream")  # fmt: skip
    step = (r"const\s+skr_step_plan\s*\*\s*plan", r"const\s+void\s*\*\s*const\s*\*\s*inputs", r"void\s*\*\s*out", r"const\s+skr_step_guidance\s*\*\s*guide",
            r"const\s+skr_step_rescale\s*\*\s*rescale", r"const\s+uint64_t\s*\*\s*seeds_dev", r"int64_t\s+numel", r"const\s+skr_step_row\s*\*\s*rows_dev",
            r"const\s+int32_t\s*\*\s*sample_index_dev", r"int32_t\s+row_offset", r"void\s*\*\s*stream")  # fmt: skip
    for name, args in ((STATS, stats), (STEP, step)):
        assert re.search(rf"^int\s+{name}{ws}\({ws}" + rf"{ws},{ws}".join(args) + rf"{ws}\){ws};", flat, flags=re.M), name
        assert name in _hip.EXPORTS
    assert re.search(r"#define\s+SKR_ABI_VERSION\s+15\b", header) and _hip.ABI_VERSION == 15  # purely additive
    assert ctypes.sizeof(_hip.StepRowC) == 328 and _hip.StepRowC.convert_k.offset == 296  # the row keeps its layout
    assert _hip.entry_name(_hip.FACTOR, "rolling") == STATS and _hip.entry_name("guided_rescaled", "rolling") == STEP


def test_header_is_still_plain_c_and_the_row_keeps_its_size(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc on this box")
    src = tmp_path / "client.c"
    src.write_text(
        "#include <stddef.h>\n"
        f'#include "{os.path.join(ROOT, "include", "skrample_hip.h")}"\n'
        '_Static_assert(sizeof(skr_step_row) == 328, "row size");\n'
        '_Static_assert(offsetof(skr_step_row, convert_k) == 296, "where the scale and phi sit");\n'
        "int main(void) {\n"
        "  int (*stats)(const void*, const void*, int32_t, int64_t, int64_t, const skr_step_row*, const int32_t*, int32_t, void*, double*, double*,\n"
        f"               void*) = {STATS};\n"
        "  int (*step)(const skr_step_plan*, const void* const*, void*, const skr_step_guidance*, const skr_step_rescale*, const uint64_t*, int64_t,\n"
        f"              const skr_step_row*, const int32_t*, int32_t, void*) = {STEP};\n"
        "  (void)stats;\n"
        "  (void)step;\n"
        "  return SKR_ABI_VERSION == 15 ? 0 : 1;\n"
        "}\n"
    )
    done = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c", str(src), "-o", str(tmp_path / "client.o")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


# ---- the built library ---------------------------------------------------------------------------------------------------------------
def make_plan(n=3, dtype=_hip.BF16, sample_numel=4096, **fields):
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = n
    plan.dtype_a = plan.out0_dtype = dtype
    plan.dtype_b, plan.out1_dtype = _hip.F32, _hip.NONE
    plan.sample_numel = sample_numel
    for k in range(n):
        plan.coef0[k] = 1.0 + k
    plan.noise_mode, plan.zeta0, plan.stream0 = 1, 0.5, 513
    for key, value in fields.items():
        setattr(plan, key, value)
    return plan


def host_pointers(count):
    "16-byte aligned host addresses that stand in for device pointers, and the buffer that must stay zero"
    buf = (ctypes.c_char * (48 * count + 32))()
    base = (ctypes.addressof(buf) + 15) & ~15
    return buf, [base + 48 * k for k in range(count)]


def test_the_statistics_entry_checks_on_the_host_in_the_stated_order():
    "every status is returned ahead of the launch; where the checks are skr_guidance_rescale_factor's, it is the status that entry returns"
    lib = _hip.load()
    assert lib.skr_abi_version() == 15
    entry, lone = getattr(lib, STATS), lib.skr_guidance_rescale_factor
    assert len(entry.argtypes) == 12 and entry.restype is ctypes.c_int
    buf, (u, c, factor, partials, rows, index) = host_pointers(6)
    given = dict(uncond=u, cond=c, dtype=_hip.BF16, numel=8192, sample_numel=4096, rows=rows, index=index, row_offset=0, factor=factor, partials=partials)

    def call(**changed):
        a = {**given, **changed}
        return entry(a["uncond"], a["cond"], a["dtype"], a["numel"], a["sample_numel"], a["rows"], a["index"], a["row_offset"], a["factor"], None, a["partials"], None)

    def call_lone(**changed):
        a = {**given, **changed}
        return lone(a["uncond"], a["cond"], a["dtype"], 7.5, a["numel"], a["sample_numel"], a["factor"], None, a["partials"], None)

    shared = [  # (arguments, status): the checks of skr_guidance_rescale_factor, its order, its codes
        (dict(uncond=None), NULL),
        (dict(cond=None), NULL),
        (dict(factor=None), NULL),
        (dict(partials=None), NULL),
        (dict(partials=None, numel=-1), NULL),  # two faults: the NULL tests come first
        (dict(numel=-1), SHAPE),
        (dict(sample_numel=1), SHAPE),
        (dict(sample_numel=4096 + 2048), SHAPE),  # does not divide numel
        (dict(numel=-1, uncond=u + 4), SHAPE),  # the size ahead of the alignment
        (dict(numel=0), OK),
        (dict(numel=0, cond=c + 2, dtype=99), OK),  # nothing to do ahead of alignment and dtype
        (dict(uncond=u + 4), ALIGN),
        (dict(cond=c + 2), ALIGN),
        (dict(cond=c + 2, dtype=99), ALIGN),  # the alignment ahead of the dtype
        (dict(dtype=99), DTYPE),
        (dict(dtype=_hip.NONE), DTYPE),
    ]
    for arguments, status in shared:
        assert call(**arguments) == status, arguments
        assert call_lone(**arguments) == status, arguments
    own = [  # what the rolling entry adds
        (dict(rows=None), NULL),
        (dict(index=None), NULL),
        (dict(index=None, numel=-1), NULL),
        (dict(rows=None, numel=0), NULL),
        (dict(dtype=99, row_offset=-1), DTYPE),  # the dtype ahead of the coverage
        (dict(dtype=_hip.F64), UNSUPPORTED),
        (dict(numel=6000, sample_numel=3000), UNSUPPORTED),  # samples of whole 2048-element spans only
        (dict(numel=2048, sample_numel=1024), UNSUPPORTED),
        (dict(row_offset=-1), UNSUPPORTED),
        (dict(numel=4096 * ((1 << 31) // 2 + 1), sample_numel=4096), UNSUPPORTED),  # more than INT32_MAX spans
        (dict(uncond=u + 4, row_offset=-1), ALIGN),
    ]
    for arguments, status in own:
        assert call(**arguments) == status, arguments
    assert bytes(buf) == bytes(len(buf))  # nothing was written


def test_the_step_entry_checks_on_the_host_as_its_twin_does():
    "the status of skr_step_launch_guided_rolling for the twin's arguments; what skr_step_launch_guided_rescaled adds, where it adds it"
    lib = _hip.load()
    entry, twin = getattr(lib, STEP), lib.skr_step_launch_guided_rolling
    assert len(entry.argtypes) == 11 and entry.restype is ctypes.c_int
    buf, (a, b, c, out, cond, gout, seeds, rows, index, factor) = host_pointers(10)

    def call(fn, plan=None, slot=1, rows=rows, index=index, row_offset=0, seeds=seeds, numel=8192, out=out, reserved=0, guide=True, with_plan=True, rescale=True,
             factor=factor, rs_numel=4096, rs_reserved=0):  # fmt: skip
        plan = plan if plan is not None else make_plan()
        arr = (ctypes.c_void_p * 3)(a, b, c)
        desc = _hip.StepGuidanceC(cond, gout, 7.5, slot, reserved)  # (the scale is a decoy: ignored)
        if fn is twin:
            return fn(ctypes.byref(plan) if with_plan else None, arr, out, ctypes.byref(desc) if guide else None, seeds, numel, rows, index, row_offset, None)
        rs = _hip.StepRescaleC(factor, 0.25, rs_numel, rs_reserved)  # (phi is a decoy: ignored)
        return fn(ctypes.byref(plan) if with_plan else None, arr, out, ctypes.byref(desc) if guide else None, ctypes.byref(rs) if rescale else None, seeds, numel, rows,
                  index, row_offset, None)  # fmt: skip

    table = [  # the twin's arguments: the twin's status
        (dict(rows=None), NULL),
        (dict(index=None), NULL),
        (dict(index=None, numel=0), NULL),
        (dict(guide=False), NULL),
        (dict(with_plan=False), NULL),
        (dict(seeds=None, plan=make_plan(zeta0=0.0)), NULL),
        (dict(rows=None, slot=7), NULL),
        (dict(slot=7, numel=-1), TERMS),
        (dict(numel=-1, reserved=1), SHAPE),
        (dict(reserved=1, row_offset=-1), UNSUPPORTED),
        (dict(plan=make_plan(convert_to=1)), UNSUPPORTED),
        (dict(out=out + 4, row_offset=-1), ALIGN),
        (dict(plan=make_plan(out0_dtype=_hip.F16), row_offset=-1), DTYPE),
        (dict(row_offset=-1), UNSUPPORTED),
        (dict(plan=make_plan(acc_f64=1)), UNSUPPORTED),
        (dict(plan=make_plan(n_group_a=2)), UNSUPPORTED),
        (dict(numel=0), OK),
    ]
    for arguments, status in table:
        assert call(twin, **arguments) == status, arguments
        assert call(entry, **arguments) == status, arguments
    # shapes the twin refuses, with a statistic's sample that follows the plan's (so that only the twin's fault is there)
    for arguments, rs_numel, status in (
        (dict(numel=8192 + 8, plan=make_plan(noise_mode=0)), 8, UNSUPPORTED),  # ragged: no grid-stride form
        (dict(plan=make_plan(noise_mode=0, sample_numel=8192 - 2048)), 4096, SHAPE),
        (dict(plan=make_plan(noise_mode=0, sample_numel=1024)), 1024, UNSUPPORTED),
    ):
        assert call(twin, **arguments) == status, arguments
        assert call(entry, rs_numel=rs_numel, **arguments) == status, arguments
    own = [  # what the rescale descriptor adds, each where skr_step_launch_guided_rescaled has it
        (dict(rescale=False), NULL),
        (dict(rescale=False, slot=7), NULL),  # beside the NULL plan: ahead of the operand count
        (dict(rs_reserved=1), UNSUPPORTED),
        (dict(rs_reserved=1, numel=-1), SHAPE),  # behind the size, beside the guide's reserved
        (dict(rs_reserved=1, out=out + 4), UNSUPPORTED),  # ahead of the alignment
        (dict(factor=None), NULL),
        (dict(factor=None, out=out + 4), NULL),  # beside the NULL operands: ahead of the alignment
        (dict(factor=None, rs_reserved=1), UNSUPPORTED),
        (dict(factor=None, numel=0), OK),
        (dict(rs_numel=2048), SHAPE),  # not the plan's sample
        (dict(rs_numel=8192), SHAPE),
        (dict(rs_numel=2048, plan=make_plan(noise_mode=0)), SHAPE),  # with or without noise
        (dict(rs_numel=1), SHAPE),
        (dict(rs_numel=3000), SHAPE),  # does not divide numel
        (dict(rs_numel=2048, factor=None), SHAPE),  # the sample size ahead of the NULL operands
    ]
    for arguments, status in own:
        assert call(entry, **arguments) == status, arguments
    assert lib.skr_set_tuning(b"one_trip", 0) == 0
    try:
        assert call(entry) == call(twin) == UNSUPPORTED
    finally:
        assert lib.skr_set_tuning(b"one_trip", 1) == 0
    assert bytes(buf) == bytes(len(buf))  # nothing was written


# ---- a rescaled RollingBatch on stub rows --------------------------------------------------------------------------------------------
def stub_plan(roles, scale):
    "coef0[j] = scale * (j + 1)"
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = len(roles)
    plan.dtype_a = plan.dtype_b = plan.out0_dtype = _hip.BF16
    plan.out1_dtype = _hip.NONE
    for j in range(len(roles)):
        plan.coef0[j] = scale * (j + 1)
    return plan


class StubBatch(RollingBatch):
    "the dry run gives an Adams-3-like ramp-up (2, 3, 4, 4, ... operands); the two launches are recorded by the tests, not made"

    history = HISTORY

    def __init__(self, *args, **kwargs):
        self.traces = 0
        super().__init__(*args, **kwargs)

    def _trace(self, wrapper, steps, seed):
        self.traces += 1
        return [(stub_plan(self.history[: min(i + 2, len(self.history))], 10.0 * (i + 1)), self.history[: min(i + 2, len(self.history))], 100.0 - i) for i in range(steps)]


class EulerStub(StubBatch):
    history = HISTORY[:2]


def wrapper():
    return PD.SkrampleWrapperScheduler(PT.Adams(order=3), PS.Scaled())


def euler():
    return PD.SkrampleWrapperScheduler(PT.Euler(), PS.Scaled())


def rescaled_batch(capacity=4, cls=StubBatch, make=wrapper, **options):
    return cls(make, torch.zeros(capacity, *UNIT, dtype=torch.bfloat16), capacity=capacity, guided=True, rescaled=True, **options)


@pytest.fixture
def launches(monkeypatch):
    "the library replaced by a recorder: (C entry name, arguments -- a descriptor passed by reference as the descriptor) in issue order"
    calls = []

    class Lib:
        def __getattr__(self, name):
            if not name.startswith(("skr_step_launch", "skr_guidance_rescale_factor")):
                raise AttributeError(name)
            return lambda *args: calls.append((name, tuple(getattr(a, "_obj", a) for a in args))) or 0

    monkeypatch.setattr(_hip, "load", lambda: Lib())
    monkeypatch.setattr(_hip, "current_stream_ptr", lambda device: 77)
    return calls


def test_rescaled_needs_guided_and_the_batch_owns_factor_and_partials():
    example = torch.zeros(4, *UNIT, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="rescaled=True needs guided=True"):
        StubBatch(wrapper, example, capacity=4, rescaled=True)
    batch = rescaled_batch()
    assert batch.guided and batch.rescaled and batch.slot == 1
    assert tuple(batch.factor.shape) == (4,) and batch.factor.dtype == torch.bfloat16
    assert batch._partials.dtype == torch.float64 and batch._partials.numel() == _hip.guidance_partials(batch.numel, batch.sample_numel) == 4 * 4 * 2
    plain = StubBatch(wrapper, example, capacity=4, guided=True)
    assert plain.rescaled is False and not hasattr(plain, "factor")


def test_signatures_keep_guidance_rescale_out_of_the_constructor_and_the_tick():
    assert "rescaled" in inspect.signature(RollingBatch.__init__).parameters
    assert "guidance_rescale" not in inspect.signature(RollingBatch.__init__).parameters
    assert list(inspect.signature(RollingBatch.step_guided).parameters) == ["self", "uncond", "cond"]
    assert inspect.signature(RollingBatch.admit).parameters["guidance_rescale"].default == 0.0


def test_rows_carry_phi_or_the_schedule_in_convert_k_1_and_zeros_otherwise():
    batch = rescaled_batch()
    x = torch.zeros(UNIT, dtype=torch.bfloat16)
    batch.admit(0, x, wrapper(), 4, guidance_scale=3.5, guidance_rescale=0.7)
    batch.admit(1, x, wrapper(), 3, guidance_scale=[7.0, -1.25, 0.5], guidance_rescale=[0.5, 0.0, 1])
    batch.admit(2, x, wrapper(), 2, guidance_scale=2.0)  # the default: not rescaled
    assert [(r.convert_k[0], r.convert_k[1]) for r in batch._requests[0].rows] == [(3.5, 0.7)] * 4
    assert [(r.convert_k[0], r.convert_k[1]) for r in batch._requests[1].rows] == [(7.0, 0.5), (-1.25, 0.0), (0.5, 1.0)]
    assert [(r.convert_k[0], r.convert_k[1]) for r in batch._requests[2].rows] == [(2.0, 0.0)] * 2
    for b in range(3):
        for r in batch._requests[b].rows:
            assert r.convert_k[2] == r.convert_k[3] == 0.0 and not any(r.coef1)
    stored = bytes(batch.rows_dev[1 * batch.max_steps * batch.row_bytes :][: 3 * batch.row_bytes].numpy())
    assert stored == b"".join(bytes(r) for r in batch._requests[1].rows)  # the right rows of the table
    unrescaled = StubBatch(wrapper, torch.zeros(4, *UNIT, dtype=torch.bfloat16), capacity=4, guided=True)
    unrescaled.admit(0, x, wrapper(), 3, guidance_scale=2.0, guidance_rescale=0.0)
    unrescaled.admit(1, x, wrapper(), 3, guidance_scale=2.0, guidance_rescale=[0.0, 0, 0.0])
    assert all(r.convert_k[1] == 0.0 for b in (0, 1) for r in unrescaled._requests[b].rows)


def test_admit_refusals_name_their_reason_and_come_before_the_dry_run(monkeypatch):
    uploads = []
    monkeypatch.setattr(rolling, "upload_rows", lambda *args: uploads.append(args))
    batch = rescaled_batch()
    guided = StubBatch(wrapper, torch.zeros(4, *UNIT, dtype=torch.bfloat16), capacity=4, guided=True)
    plain = StubBatch(wrapper, torch.zeros(4, *UNIT, dtype=torch.bfloat16), capacity=4)
    x = torch.zeros(UNIT, dtype=torch.bfloat16)
    traces = (batch.traces, guided.traces, plain.traces)
    for bad, says in ((-0.5, "guidance_rescale must be >= 0, not -0.5"), (float("nan"), "guidance_rescale must be >= 0, not nan"),
                      (True, "guidance_rescale is a Python number, not bool"), ("0.7", "guidance_rescale is a Python number, not str"),
                      (torch.tensor(0.7), "guidance_rescale is a Python number, not Tensor"), (None, "guidance_rescale is a Python number, not NoneType"),
                      ([0.7, -1.0, 0.0, 0.0], "guidance_rescale must be >= 0, not -1.0"), ([0.7, "x", 0.0, 0.0], "guidance_rescale is a Python number, not str"),
                      ([0.7, 0.7, 0.7], "one guidance_rescale per step: 3 values for 4 steps"), ([0.7] * 5, "one guidance_rescale per step: 5 values for 4 steps")):  # fmt: skip
        with pytest.raises(ValueError, match=re.escape(says)):
            batch.admit(0, x, wrapper(), 4, guidance_scale=2.0, guidance_rescale=bad)
    with pytest.raises(ValueError, match="guidance_rescale= needs a batch built with guided=True, rescaled=True"):
        guided.admit(0, x, wrapper(), 4, guidance_scale=2.0, guidance_rescale=0.7)
    with pytest.raises(ValueError, match="guidance_rescale= needs a batch built with guided=True, rescaled=True"):
        guided.admit(0, x, wrapper(), 4, guidance_scale=2.0, guidance_rescale=[0.0, 0.0, 0.0, 0.1])
    with pytest.raises(ValueError, match="guidance_rescale= needs a batch built with guided=True, rescaled=True"):
        plain.admit(0, x, wrapper(), 4, guidance_rescale=0.7)
    assert (batch.traces, guided.traces, plain.traces) == traces and uploads == []
    assert batch.free(0) and guided.free(0) and plain.free(0)


def test_a_tick_is_the_statistics_launch_then_the_step_launch_on_the_same_index_rows_and_offset(launches):
    batch = rescaled_batch()
    x = torch.zeros(UNIT, dtype=torch.bfloat16)
    batch.admit(0, x, wrapper(), 3, guidance_scale=2.0, guidance_rescale=0.7)
    batch.admit(2, x, wrapper(), 3, guidance_scale=2.0)  # a neighbour that does not rescale: the tick is the same two launches
    for tick in range(3):
        u, c = torch.zeros(4, *UNIT, dtype=torch.bfloat16), torch.zeros(4, *UNIT, dtype=torch.bfloat16)
        done = batch.step_guided(u, c)
        assert done == ([0, 2] if tick == 2 else [])
        (first, stats), (second, step) = launches[2 * tick :]
        assert (first, second) == ("skr_guidance_rescale_factor_rolling", "skr_step_launch_guided_rescaled_rolling")
        uncond_ptr, cond_ptr, code, numel, sample_numel, rows, index, offset, factor, stats_ptr, partials, stream = stats
        assert (uncond_ptr, cond_ptr, code, numel, sample_numel) == (u.data_ptr(), c.data_ptr(), _hip.BF16, batch.numel, batch.sample_numel)
        assert (factor, stats_ptr, partials, stream) == (batch.factor.data_ptr(), None, batch._partials.data_ptr(), 77)
        plan, arr, out_ptr, guide, rescale, seeds, step_numel, step_rows, step_index, step_offset, step_stream = step
        assert (rows, index, offset) == (step_rows, step_index, step_offset) == (batch.rows_dev.data_ptr(), batch.index_dev.data_ptr(), 0)
        assert step_numel == numel and step_stream == stream and seeds is None and out_ptr == batch.latents.data_ptr()
        assert arr[batch.slot] == u.data_ptr() and (guide.cond, guide.slot, guide.reserved) == (c.data_ptr(), 1, 0)
        assert guide.guided_out == batch._g[-1].data_ptr()
        assert (rescale.factor_dev, rescale.sample_numel, rescale.reserved) == (batch.factor.data_ptr(), batch.sample_numel, 0)
    assert len(launches) == 6
    assert batch.index_dev.tolist() == [2, -1, 2 * batch.max_steps + 2, -1]


def test_euler_passes_no_guided_out_and_a_guided_batch_keeps_its_one_launch(launches):
    batch = rescaled_batch(capacity=2, cls=EulerStub, make=euler)
    assert batch.keep == 0 and batch._g == []
    batch.admit(0, torch.zeros(UNIT, dtype=torch.bfloat16), euler(), 2, guidance_scale=1.5, guidance_rescale=1.0)
    u, c = torch.zeros(2, *UNIT, dtype=torch.bfloat16), torch.zeros(2, *UNIT, dtype=torch.bfloat16)
    batch.step_guided(u, c)
    assert [name for name, _ in launches] == ["skr_guidance_rescale_factor_rolling", "skr_step_launch_guided_rescaled_rolling"]
    assert launches[1][1][3].guided_out is None
    del launches[:]
    guided = EulerStub(euler, torch.zeros(2, *UNIT, dtype=torch.bfloat16), capacity=2, guided=True)
    guided.admit(0, torch.zeros(UNIT, dtype=torch.bfloat16), euler(), 2, guidance_scale=1.5)
    guided.step_guided(u, c)
    assert [name for name, _ in launches] == ["skr_step_launch_guided_rolling"]


def test_the_constructor_refusals_of_a_guided_batch_are_unchanged():
    example = torch.zeros(4, *UNIT, dtype=torch.bfloat16)
    built = []

    class Counting(StubBatch):
        def _trace(self, wrapper, steps, seed):
            built.append(steps)
            return super()._trace(wrapper, steps, seed)

    for sampler, says in ((PT.UniPC(), "UniPC"), (PT.SPC(), "SPC")):
        with pytest.raises(_hip.SkrampleHipError, match=f"{says} is not one fused launch"):
            Counting(lambda: PD.SkrampleWrapperScheduler(sampler, PS.Scaled()), example, capacity=4, guided=True, rescaled=True)
    with pytest.raises(_hip.SkrampleHipError, match="compute_scale=None is not one fused launch"):
        Counting(lambda: PD.SkrampleWrapperScheduler(PT.Adams(order=3), PS.Scaled(), compute_scale=None), example, capacity=4, guided=True, rescaled=True)
    with pytest.raises(ValueError, match="guided together with inpaint_mask_shape"):
        Counting(wrapper, example, capacity=4, guided=True, rescaled=True, inpaint_mask_shape=(1, 32, 32))
    from skrample_amd.pytorch import noise as generators

    for kind in (generators.Offset, generators.Pyramid):
        with pytest.raises(ValueError, match=f"guided together with {kind.__name__} noise"):
            Counting(lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=1), PS.Scaled(), noise_type=kind), example, capacity=4, guided=True, rescaled=True)
    with pytest.raises(_hip.SkrampleHipError, match="16- or 32-bit dtype"):
        Counting(wrapper, example.double(), capacity=4, guided=True, rescaled=True)
    assert built == []  # refused before the dry run
