"""Guided steps in rolling batches without a GPU: the new export at the C boundary, the host-side checks of the built library, and the
bookkeeping of a guided `skrample_amd.rolling.RollingBatch` on stub rows (the dry run and the launch are replaced, as in
tests/test_rolling_host.py and tests/test_masked_rolling_host.py: nothing here enqueues device work)."""

import ctypes
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

NAME = "skr_step_launch_guided_rolling"
TWIN = "skr_step_launch_guided_indexed_per_sample"
OK, NULL, DTYPE, TERMS, ALIGN, SHAPE, LAUNCH, UNSUPPORTED = range(8)
HISTORY = [("x",), ("o",), ("po", -1), ("po", -2)]
UNIT = (4, 32, 32)


# ---- header, exports, ABI ----------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_and_the_binding_lists_it():
    header = open(os.path.join(ROOT, "include", "skrample_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    ws = r"\s*"
    args = (r"const\s+skr_step_plan\s*\*\s*plan", r"const\s+void\s*\*\s*const\s*\*\s*inputs", r"void\s*\*\s*out", r"const\s+skr_step_guidance\s*\*\s*guide",
            r"const\s+uint64_t\s*\*\s*seeds_dev", r"int64_t\s+numel", r"const\s+skr_step_row\s*\*\s*rows_dev", r"const\s+int32_t\s*\*\s*sample_index_dev",
            r"int32_t\s+row_offset", r"void\s*\*\s*stream")  # fmt: skip
    assert re.search(rf"^int\s+{NAME}{ws}\({ws}" + rf"{ws},{ws}".join(args) + rf"{ws}\){ws};", flat, flags=re.M)
    assert NAME in _hip.EXPORTS
    assert re.search(r"#define\s+SKR_ABI_VERSION\s+15\b", header) and _hip.ABI_VERSION == 15  # purely additive
    assert ctypes.sizeof(_hip.StepRowC) == 328 and _hip.StepRowC.convert_k.offset == 296  # the row keeps its layout
    assert ctypes.sizeof(_hip.StepGuidanceC) == 32
    assert _hip.entry_name("guided", "rolling") == NAME and _hip.entry_name("guided", "indexed_per_sample") == TWIN


def test_header_is_still_plain_c_and_the_row_keeps_its_size(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc on this box")
    src = tmp_path / "client.c"
    src.write_text(
        "#include <stddef.h>\n"
        f'#include "{os.path.join(ROOT, "include", "skrample_hip.h")}"\n'
        '_Static_assert(sizeof(skr_step_row) == 328, "row size");\n'
        '_Static_assert(offsetof(skr_step_row, convert_k) == 296, "where the scale sits");\n'
        "int main(void) {\n"
        "  int (*rolling)(const skr_step_plan*, const void* const*, void*, const skr_step_guidance*, const uint64_t*, int64_t, const skr_step_row*,\n"
        f"                 const int32_t*, int32_t, void*) = {NAME};\n"
        "  (void)rolling;\n"
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


def test_the_built_library_exports_the_entry_and_checks_on_the_host():
    """host buffers that are never read stand in for device pointers: every status below is returned ahead of the launch, and it is the
    status the per-sample twin returns for the same arguments"""
    lib = _hip.load()
    assert lib.skr_abi_version() == 15
    entry, twin = getattr(lib, NAME), getattr(lib, TWIN)
    assert entry.argtypes == twin.argtypes and len(entry.argtypes) == 10 and entry.restype is ctypes.c_int
    buf = (ctypes.c_char * 512)()
    base = (ctypes.addressof(buf) + 15) & ~15
    a, b, c, out, cond, gout, seeds, rows, index = (base + 48 * k for k in range(9))

    def call(fn, plan=None, slot=1, rows=rows, index=index, row_offset=0, seeds=seeds, numel=8192, out=out, reserved=0, guide=True, with_plan=True):
        plan = plan if plan is not None else make_plan()
        arr = (ctypes.c_void_p * 3)(a, b, c)
        desc = _hip.StepGuidanceC(cond, gout, 7.5, slot, reserved)
        return fn(ctypes.byref(plan) if with_plan else None, arr, out, ctypes.byref(desc) if guide else None, seeds, numel, rows, index, row_offset, None)

    table = [
        (dict(rows=None), NULL),
        (dict(index=None), NULL),
        (dict(index=None, numel=0), NULL),
        (dict(guide=False), NULL),
        (dict(with_plan=False), NULL),
        (dict(seeds=None, plan=make_plan(zeta0=0.0)), NULL),  # noise_mode 1 needs seeds whatever the plan (or a row) holds
        (dict(rows=None, slot=7), NULL),  # the order: NULL tests, then the operand count and the slot, then the size, ...
        (dict(slot=7, numel=-1), TERMS),
        (dict(numel=-1, reserved=1), SHAPE),
        (dict(reserved=1, row_offset=-1), UNSUPPORTED),
        (dict(plan=make_plan(convert_to=1)), UNSUPPORTED),
        (dict(out=out + 4, row_offset=-1), ALIGN),
        (dict(plan=make_plan(out0_dtype=_hip.F16), row_offset=-1), DTYPE),
        (dict(row_offset=-1), UNSUPPORTED),
        (dict(numel=8192 + 8, plan=make_plan(noise_mode=0)), UNSUPPORTED),  # ragged: no grid-stride form
        (dict(plan=make_plan(acc_f64=1)), UNSUPPORTED),
        (dict(plan=make_plan(n_group_a=2)), UNSUPPORTED),  # two dtype groups
        (dict(plan=make_plan(noise_mode=0, sample_numel=0)), SHAPE),  # a workgroup lies inside one sample, with or without noise
        (dict(plan=make_plan(noise_mode=0, sample_numel=8192 - 2048)), SHAPE),
        (dict(plan=make_plan(noise_mode=0, sample_numel=1024)), UNSUPPORTED),
        (dict(numel=0), OK),
    ]
    for arguments, status in table:
        assert call(entry, **arguments) == status, arguments
        assert call(twin, **arguments) == status, arguments
    assert lib.skr_set_tuning(b"one_trip", 0) == 0
    try:
        assert call(entry) == call(twin) == UNSUPPORTED
    finally:
        assert lib.skr_set_tuning(b"one_trip", 1) == 0
    assert bytes(buf) == bytes(512)  # nothing was written


# ---- a guided RollingBatch on stub rows ----------------------------------------------------------------------------------------------
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
    "the dry run gives an Adams-3-like ramp-up (2, 3, 4, 4, ... operands); launches are recorded, not made"

    history = HISTORY

    def __init__(self, *args, **kwargs):
        self.launched, self.traces = [], 0
        super().__init__(*args, **kwargs)

    def _trace(self, wrapper, steps, seed):
        self.traces += 1
        return [(stub_plan(self.history[: min(i + 2, len(self.history))], 10.0 * (i + 1)), self.history[: min(i + 2, len(self.history))], 100.0 - i) for i in range(steps)]

    def _launch(self, arr, out0, out1, cond=None, guided_out=None):
        self.launched.append((list(arr), out0, out1, cond, guided_out))


class EulerStub(StubBatch):
    history = HISTORY[:2]


def wrapper():
    return PD.SkrampleWrapperScheduler(PT.Adams(order=3), PS.Scaled())


def euler():
    return PD.SkrampleWrapperScheduler(PT.Euler(), PS.Scaled())


def guided_batch(capacity=4, **options):
    return StubBatch(wrapper, torch.zeros(capacity, *UNIT, dtype=torch.bfloat16), capacity=capacity, guided=True, **options)


def test_slot_is_the_place_of_the_network_output_and_the_batch_owns_a_ring_of_predictions():
    batch = guided_batch()
    assert batch.guided and batch.roles == HISTORY and batch.slot == HISTORY.index(("o",)) == 1 and batch.keep == 2
    assert len(batch._g) == len(batch._x) == batch.keep + 2  # as long as the latents ring: captured phases close
    assert all(tuple(t.shape) == (4, *UNIT) and t.dtype == torch.bfloat16 for t in batch._g)
    assert all(any(t is r for r in batch.ring_tensors()) for t in batch._g)


def test_rows_carry_the_scale_or_the_schedule_and_ramp_up_rows_have_zeros_in_the_history_slots():
    batch = guided_batch()
    x = torch.zeros(UNIT, dtype=torch.bfloat16)
    batch.admit(1, x, wrapper(), 4, guidance_scale=3.5)
    batch.admit(2, x, wrapper(), 3, guidance_scale=[7.0, -1.25, 0.5])
    batch.admit(3, x, wrapper(), 2, guidance_scale=2)  # (an int is a number too)
    assert [r.convert_k[0] for r in batch._requests[1].rows] == [3.5] * 4
    assert [r.convert_k[0] for r in batch._requests[2].rows] == [7.0, -1.25, 0.5]
    assert [r.convert_k[0] for r in batch._requests[3].rows] == [2.0, 2.0]
    rows = batch._requests[1].rows
    assert [list(r.coef0)[:4] for r in rows[:3]] == [[10.0, 20.0, 0.0, 0.0], [20.0, 40.0, 60.0, 0.0], [30.0, 60.0, 90.0, 120.0]]
    for r in rows:
        assert not any(r.coef1) and [r.convert_k[k] for k in (1, 2, 3)] == [0.0, 0.0, 0.0] and not any(list(r.coef0)[4:])
    first = rows[0]  # exact zeros: a new request never reads its slot's previous occupant's predictions
    assert bytes(ctypes.c_double(first.coef0[2])) == bytes(ctypes.c_double(first.coef0[3])) == bytes(8)
    stored = bytes(batch.rows_dev[1 * batch.max_steps * batch.row_bytes :][: 4 * batch.row_bytes].numpy())
    assert stored == b"".join(bytes(r) for r in rows)


def test_ring_rotation_binds_the_history_to_the_batch_own_tensors():
    batch = guided_batch()
    x = torch.zeros(UNIT, dtype=torch.bfloat16)
    batch.admit(0, x, wrapper(), 6, guidance_scale=2.0)
    own = {t.data_ptr() for t in batch._g}
    stores = []
    for tick in range(6):
        u, c = torch.zeros(4, *UNIT, dtype=torch.bfloat16), torch.zeros(4, *UNIT, dtype=torch.bfloat16)
        latents = batch.latents
        done = batch.step_guided(u, c)
        assert done == ([0] if tick == 5 else [])
        ptrs, out0, out1, cond, guided_out = batch.launched[-1]
        assert ptrs[0] == latents.data_ptr() and ptrs[1] == u.data_ptr() and cond is c and out1 is None and out0 is batch.latents
        assert guided_out.data_ptr() in own and guided_out.data_ptr() not in ptrs  # the entry no operand reads
        stores.append(guided_out.data_ptr())
        if tick >= 1:
            assert ptrs[2] == stores[tick - 1]  # ("po", -1): what the last tick stored
        if tick >= 2:
            assert ptrs[3] == stores[tick - 2]  # ("po", -2)
        assert ptrs[2] in own and ptrs[3] in own  # nothing of the caller is held
    assert stores[4] == stores[0] and len(set(stores[:4])) == 4  # a ring of keep + 2
    assert batch._outputs == [] and batch._stamps == []  # no alias guard, no snapshot
    assert batch.index_dev.tolist() == [5, -1, -1, -1]


def test_a_sampler_without_history_passes_no_guided_out_and_owns_no_ring():
    batch = EulerStub(euler, torch.zeros(2, *UNIT, dtype=torch.bfloat16), capacity=2, guided=True)
    assert batch.keep == 0 and batch._g == [] and batch.slot == 1
    batch.admit(0, torch.zeros(UNIT, dtype=torch.bfloat16), euler(), 2, guidance_scale=1.5)
    u, c = torch.zeros(2, *UNIT, dtype=torch.bfloat16), torch.zeros(2, *UNIT, dtype=torch.bfloat16)
    batch.step_guided(u, c)
    assert batch.launched[-1][3] is c and batch.launched[-1][4] is None


def test_refusals_come_before_anything_is_uploaded_and_name_their_reason(monkeypatch):
    uploads = []
    monkeypatch.setattr(rolling, "upload_rows", lambda *args: uploads.append(args))
    example = torch.zeros(4, *UNIT, dtype=torch.bfloat16)
    built = []

    class Counting(StubBatch):
        def _trace(self, wrapper, steps, seed):
            built.append(steps)
            return super()._trace(wrapper, steps, seed)

    for sampler, says in ((PT.UniPC(), "UniPC"), (PT.SPC(), "SPC")):
        with pytest.raises(_hip.SkrampleHipError, match=f"{says} is not one fused launch"):
            Counting(lambda: PD.SkrampleWrapperScheduler(sampler, PS.Scaled()), example, capacity=4, guided=True)
    with pytest.raises(_hip.SkrampleHipError, match="compute_scale=None is not one fused launch"):
        Counting(lambda: PD.SkrampleWrapperScheduler(PT.Adams(order=3), PS.Scaled(), compute_scale=None), example, capacity=4, guided=True)
    with pytest.raises(ValueError, match="guided together with inpaint_mask_shape"):
        Counting(wrapper, example, capacity=4, guided=True, inpaint_mask_shape=(1, 32, 32))
    from skrample_amd.pytorch import noise as generators

    with pytest.raises(ValueError, match="guided together with Offset noise"):
        Counting(lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=1), PS.Scaled(), noise_type=generators.Offset), example, capacity=4, guided=True)
    with pytest.raises(_hip.SkrampleHipError, match="16- or 32-bit dtype"):
        Counting(wrapper, example.double(), capacity=4, guided=True)
    assert built == []  # refused before the dry run
    batch, plain = guided_batch(), StubBatch(wrapper, example, capacity=4)
    x = torch.zeros(UNIT, dtype=torch.bfloat16)
    traces = (batch.traces, plain.traces)
    with pytest.raises(ValueError, match="guidance_scale is required on a guided batch"):
        batch.admit(0, x, wrapper(), 4)
    with pytest.raises(ValueError, match="one scale per step: 3 scales for 4 steps"):
        batch.admit(0, x, wrapper(), 4, guidance_scale=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="a float or a sequence"):
        batch.admit(0, x, wrapper(), 4, guidance_scale=object())
    with pytest.raises(ValueError, match="needs a batch built with guided=True"):
        plain.admit(0, x, wrapper(), 4, guidance_scale=2.0)
    assert (batch.traces, plain.traces) == traces and uploads == [] and batch.free(0) and plain.free(0)
    out = torch.zeros(4, *UNIT, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="step_guided"):
        batch.step(out)
    with pytest.raises(ValueError, match="guided=True"):
        plain.step_guided(out, out)
    batch.admit(0, x, wrapper(), 4, guidance_scale=2.0)
    for bad in (out[:2], out.float(), out.transpose(2, 3)):
        with pytest.raises(ValueError, match="of a tick is a contiguous"):
            batch.step_guided(out, bad)
        with pytest.raises(ValueError, match="of a tick is a contiguous"):
            batch.step_guided(bad, out)
    assert batch.launched == [] and len(uploads) == 1


def test_a_request_whose_uncond_is_elsewhere_is_refused():
    batch = guided_batch()
    swapped = [("o",), ("x",)]
    batch._trace = lambda wrapper, steps, seed: [(stub_plan(swapped, 1.0), swapped, 1.0)] * steps
    with pytest.raises(_hip.SkrampleHipError):
        batch.admit(0, torch.zeros(UNIT, dtype=torch.bfloat16), wrapper(), 2, guidance_scale=1.0)
    assert batch.free(0) and not batch.rows_dev.any()


def test_a_batch_built_without_guided_is_what_it_was(monkeypatch):
    plain = StubBatch(wrapper, torch.zeros(4, *UNIT, dtype=torch.bfloat16), capacity=4)
    assert plain.guided is False and plain.roles == HISTORY and plain._g == [] and not hasattr(plain, "slot")
    x = torch.zeros(UNIT, dtype=torch.bfloat16)
    plain.admit(0, x, wrapper(), 3)
    assert all(r.convert_k[0] == 0.0 for r in plain._requests[0].rows)
    out = torch.zeros(4, *UNIT, dtype=torch.bfloat16)
    assert plain.step(out) == [] and plain.launched[-1][3:] == (None, None)
    assert plain._outputs[0] is out  # the caller's model output is the history, as ever
    calls = []

    class Lib:
        def __getattr__(self, name):
            def launch(*args):
                calls.append((name, args))
                return 0

            return launch

    monkeypatch.setattr(_hip, "load", lambda: Lib())
    monkeypatch.setattr(_hip, "current_stream_ptr", lambda device: 0)
    arr = (ctypes.c_void_p * 1)(out.data_ptr())
    RollingBatch._launch(plain, arr, out, None)
    assert [name for name, _ in calls] == ["skr_step_launch_rolling"] and len(calls[0][1]) == 10
    guided = guided_batch()
    cond, stored = torch.zeros(4, *UNIT, dtype=torch.bfloat16), torch.zeros(4, *UNIT, dtype=torch.bfloat16)
    RollingBatch._launch(guided, arr, out, None, cond, stored)
    RollingBatch._launch(guided, arr, out, None, cond, None)
    name, args = calls[1]
    assert name == NAME and len(args) == 10
    assert args[2] == out.data_ptr() and args[5] == guided.numel and args[6] == guided.rows_dev.data_ptr() and args[7] == guided.index_dev.data_ptr() and args[8] == 0
    desc = args[3]._obj
    assert (desc.cond, desc.guided_out, desc.slot, desc.reserved) == (cond.data_ptr(), stored.data_ptr(), 1, 0)
    assert calls[2][1][3]._obj.guided_out is None
