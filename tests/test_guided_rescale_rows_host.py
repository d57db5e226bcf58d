"""Rescaled guidance with device-resident rows, without a device: the four C ABI declarations and their binding, the row recorder
(_hip.IndexedRows(guided=True, rescaled=True, samples=B)) in its record, refill and emit modes, driven with a stub library whose launch
functions return 0, and what `capture_sampling_loop` / `CapturedLoop.retarget` refuse before they touch a device.
guidance_rescale is a row value: it sits in convert_k[1] beside the scale in convert_k[0]; the plain and the rescaled guided launch of a
step are one structure, so a refill may move a slot between phi == 0 and phi != 0."""

import ctypes
import os
import re

import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip, graphs
from skrample_amd.sampling import structured as PT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = ("skr_guidance_rescale_factor_indexed", "skr_guidance_rescale_factor_indexed_per_sample")
STEP = ("skr_step_launch_guided_rescaled_indexed", "skr_step_launch_guided_rescaled_indexed_per_sample")
OK, NULL, DTYPE, TERMS, ALIGN, SHAPE, LAUNCH, UNSUPPORTED = range(8)


def test_header_declares_the_four_entries_and_the_binding_lists_them():
    header = open(os.path.join(ROOT, "include", "skrample_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    ws = r"\s*"
    tails = {0: r"const\s+int32_t\s*\*\s*index_dev", 1: r"const\s+int32_t\s*\*\s*sample_index_dev"}
    for k in (0, 1):
        args = (r"const\s+void\s*\*\s*uncond", r"const\s+void\s*\*\s*cond", r"int32_t\s+dtype", r"int64_t\s+numel", r"int64_t\s+sample_numel", r"const\s+skr_step_row\s*\*\s*rows_dev",
                tails[k], r"int32_t\s+row_offset", r"void\s*\*\s*factor_dev", r"double\s*\*\s*stats_dev", r"double\s*\*\s*partials_dev", r"void\s*\*\s*stream")  # fmt: skip
        assert re.search(rf"^int\s+{FACTOR[k]}{ws}\({ws}" + rf"{ws},{ws}".join(args) + rf"{ws}\){ws};", flat, flags=re.M), FACTOR[k]
        args = (r"const\s+skr_step_plan\s*\*\s*plan", r"const\s+void\s*\*\s*const\s*\*\s*inputs", r"void\s*\*\s*out", r"const\s+skr_step_guidance\s*\*\s*guide",
                r"const\s+skr_step_rescale\s*\*\s*rescale", r"const\s+uint64_t\s*\*\s*seeds_dev", r"int64_t\s+numel", r"const\s+skr_step_row\s*\*\s*rows_dev", tails[k],
                r"int32_t\s+row_offset", r"void\s*\*\s*stream")  # fmt: skip
        assert re.search(rf"^int\s+{STEP[k]}{ws}\({ws}" + rf"{ws},{ws}".join(args) + rf"{ws}\){ws};", flat, flags=re.M), STEP[k]
    for name in FACTOR + STEP:
        assert name in _hip.EXPORTS
    assert re.search(r"#define\s+SKR_ABI_VERSION\s+15\b", header) and _hip.ABI_VERSION == 15  # purely additive
    assert ctypes.sizeof(_hip.StepRowC) == 328 and _hip.StepRowC.convert_k.offset == 296  # the row keeps its layout
    assert ctypes.sizeof(_hip.StepRescaleC) == 32


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


def test_the_built_library_exports_the_entries_and_checks_on_the_host():
    "host buffers that are never read stand in for device pointers: every status below is returned ahead of the launch"
    lib = _hip.load()
    assert lib.skr_abi_version() == 15
    buf = (ctypes.c_char * 640)()
    base = (ctypes.addressof(buf) + 15) & ~15
    a, b, c, out, cond, gout, seeds, rows, index, factor, partials = (base + 48 * k for k in range(11))
    for k in (0, 1):
        entry, per_sample = getattr(lib, STEP[k]), k == 1
        assert len(entry.argtypes) == 11 and entry.restype is ctypes.c_int

        def call(plan=None, slot=1, rows=rows, index=index, row_offset=0, seeds=seeds, numel=8192, out=out, reserved=0, factor=factor, rs_numel=None, rs_reserved=0, no_rescale=False):
            plan = plan if plan is not None else make_plan()
            arr = (ctypes.c_void_p * 3)(a, b, c)
            guide = _hip.StepGuidanceC(cond, gout, 7.5, slot, reserved)
            rescale = _hip.StepRescaleC(factor, 0.7, plan.sample_numel if rs_numel is None else rs_numel, rs_reserved)
            return entry(ctypes.byref(plan), arr, out, ctypes.byref(guide), None if no_rescale else ctypes.byref(rescale), seeds, numel, rows, index, row_offset, None)

        assert call(rows=None) == NULL and call(no_rescale=True, slot=7) == NULL
        assert call(index=None, numel=0) == (NULL if per_sample else OK)
        assert call(seeds=None, plan=make_plan(zeta0=0.0)) == NULL  # noise_mode 1 needs seeds whatever the plan (or a row) holds
        assert call(slot=7, numel=-1) == TERMS and call(numel=-1, rs_reserved=1) == SHAPE
        assert call(rs_reserved=1, rs_numel=2048) == UNSUPPORTED and call(rs_numel=2048, factor=None) == SHAPE
        assert call(factor=None, row_offset=-1) == NULL and call(out=out + 4, row_offset=-1) == ALIGN
        assert call(plan=make_plan(out0_dtype=_hip.F16), row_offset=-1) == DTYPE and call(row_offset=-1) == UNSUPPORTED
        assert call(numel=8192 + 8, plan=make_plan(noise_mode=0, sample_numel=8), rs_numel=8) == UNSUPPORTED  # ragged: no grid-stride row form
        # a workgroup lies inside one sample, with or without noise, in both entries
        assert call(plan=make_plan(noise_mode=0, sample_numel=0), rs_numel=4096) == SHAPE and call(plan=make_plan(noise_mode=0, sample_numel=8192 - 2048), rs_numel=4096) == SHAPE
        assert call(plan=make_plan(noise_mode=0), rs_numel=2048) == SHAPE and call(plan=make_plan(noise_mode=0, sample_numel=1024)) == UNSUPPORTED

        stat = getattr(lib, FACTOR[k])
        assert len(stat.argtypes) == 12 and stat.restype is ctypes.c_int

        def factor_of(uncond=a, cond=cond, dtype=_hip.BF16, numel=8192, sample_numel=4096, rows=rows, index=index, row_offset=0, factor=factor, partials=partials):
            return stat(uncond, cond, dtype, numel, sample_numel, rows, index, row_offset, factor, None, partials, None)

        assert factor_of(rows=None, numel=-1) == NULL and factor_of(partials=None) == NULL and factor_of(index=None, numel=0) == (NULL if per_sample else OK)
        assert factor_of(numel=-1, uncond=a + 2) == SHAPE and factor_of(sample_numel=1) == SHAPE and factor_of(sample_numel=6144) == SHAPE
        assert factor_of(numel=0, dtype=99) == OK and factor_of(uncond=a + 2, dtype=99) == ALIGN and factor_of(dtype=99, row_offset=-1) == DTYPE
        assert factor_of(dtype=_hip.F64) == UNSUPPORTED and factor_of(numel=6144, sample_numel=3072) == UNSUPPORTED and factor_of(row_offset=-1) == UNSUPPORTED
    assert bytes(buf) == bytes(640)  # nothing was written


class StubLib:
    "stands for the library: every launch returns 0 and is remembered by name with its arguments"

    def __init__(self):
        self.calls, self.args = [], []

    def skr_strerror(self, code):
        return {7: b"request outside kernel coverage"}.get(code, b"error")

    def __getattr__(self, name):
        if not name.startswith(("skr_step_launch", "skr_guidance_rescale_factor")):
            raise AttributeError(name)

        def launch(*args):
            self.calls.append(name)
            self.args.append(args)
            return 0

        return launch


class Pointer:
    "stands for a device tensor of the recorder: only its address is asked"

    def __init__(self, at):
        self.at = at

    def data_ptr(self):
        return self.at


def make_rows(batch=None, samples=2, rescaled=True):
    rows = _hip.IndexedRows(torch.device("cpu"), slots=3, batch=batch, guided=True, rescaled=rescaled, samples=samples if rescaled else None)
    rows.rows_dev, rows.index_dev = Pointer(0x7000), Pointer(0x8000)
    if batch is not None:
        rows.sample_index_dev = Pointer(0x9000)
    return rows


def make_guide(scale=7.3, slot=1, stored=True):
    return _hip.StepGuidanceC(0x1000, 0x3000 if stored else None, scale, slot, 0)


def make_rescale(phi=0.7, sample_numel=4096):
    return _hip.StepRescaleC(0x5000, phi, sample_numel, 0)


ARR = (ctypes.c_void_p * 3)(0xA000, 0xB000, 0xC000)


def launch(rows, lib, plan, guide, rescale=None, numel=2 * 4096):
    return rows.launch(lib, plan, ARR, 0x2000, None, 0x4000, numel, None, guide=guide, rescale=rescale)


def test_the_constructor_refuses_rescaled_without_guided_or_samples():
    with pytest.raises(ValueError, match="rescaled=True needs guided=True"):
        _hip.IndexedRows(torch.device("cpu"), rescaled=True, samples=2)
    with pytest.raises(ValueError, match="samples="):
        _hip.IndexedRows(torch.device("cpu"), guided=True, rescaled=True)
    with pytest.raises(ValueError, match="per-sample capture of 3"):
        _hip.IndexedRows(torch.device("cpu"), batch=3, guided=True, rescaled=True, samples=2)
    plain = _hip.IndexedRows(torch.device("cpu"), guided=True)
    assert not plain.rescaled and plain.factor is None and plain.partials is None


def test_row_from_writes_phi_into_convert_k1_and_the_two_guided_launches_are_one_structure():
    plan = make_plan()
    row = _hip.IndexedRows.row_from(plan, 7.3, 0.7)
    assert row.convert_k[0] == 7.3 and row.convert_k[1] == 0.7 and row.convert_k[2] == row.convert_k[3] == 0.0
    assert _hip.IndexedRows.row_from(plan, 7.3, 0.0).convert_k[1] == 0.0 and _hip.IndexedRows.row_from(plan, 7.3).convert_k[1] == 0.0
    guide = make_guide()
    for shaped in (True, False):
        plain = _hip.plan_structure(plan, sample_numel=shaped, guide=guide)
        assert _hip.plan_structure(plan, sample_numel=shaped, guide=guide, rescale=make_rescale()) == plain
        assert _hip.plan_structure(plan, sample_numel=shaped, guide=guide, rescale=make_rescale(phi=0.25, sample_numel=8192)) == plain
    assert _hip.plan_structure(plan, guide=make_guide(slot=2), rescale=make_rescale()) != _hip.plan_structure(plan, guide=guide, rescale=make_rescale())


def test_record_runs_both_kinds_as_they_stand_and_keeps_phi_in_the_row():
    lib = StubLib()
    rows = make_rows()
    assert launch(rows, lib, make_plan(), make_guide(), make_rescale()) == 0
    assert launch(rows, lib, make_plan(), make_guide()) == 0  # the plain guided launch: what the wrapper issues for guidance_rescale == 0
    assert lib.calls == ["skr_step_launch_guided_rescaled", "skr_step_launch_guided"]
    assert lib.args[0][4]._obj.factor_dev == 0x5000 and lib.args[0][4]._obj.phi == 0.7  # (the wrapper's own factor and phi)
    assert [rows.host[k].convert_k[0] for k in (0, 1)] == [7.3, 7.3] and [rows.host[k].convert_k[1] for k in (0, 1)] == [0.7, 0.0]
    assert rows.structures[0] == rows.structures[1] and rows.shapeless[0] == rows.shapeless[1]
    # one factor T[samples] and one workspace, allocated while recording -- before a stream captures
    assert rows.factor.shape == (2,) and rows.factor.dtype == torch.bfloat16 and rows.partials.dtype == torch.float64
    assert rows.partials.numel() == _hip.guidance_partials(2 * 4096, 4096)
    held = (rows.factor, rows.partials)
    assert launch(rows, lib, make_plan(), make_guide(), make_rescale()) == 0 and (rows.factor, rows.partials) == held  # the same in every step
    with pytest.raises(_hip.SkrampleHipError, match="one dtype and one size"):
        launch(rows, lib, make_plan(dtype=_hip.F16), make_guide(), make_rescale())


@pytest.mark.parametrize("recorded_rescaled", [True, False])
def test_emit_is_two_launches_on_the_hooks_buffers_whatever_the_recording_pass_did(recorded_rescaled):
    lib = StubLib()
    rows = make_rows()
    first = make_rescale() if recorded_rescaled else None
    assert launch(rows, lib, make_plan(), make_guide(), first) == 0 and launch(rows, lib, make_plan(noise_mode=0, sample_numel=0, zeta0=0.0), make_guide(slot=0), first) == 0
    rows.length = 2
    rows.begin("emit")
    lib.calls.clear(), lib.args.clear()
    for k, (plan, guide) in enumerate([(make_plan(), make_guide(scale=-1.0)), (make_plan(noise_mode=0, sample_numel=0, zeta0=0.0), make_guide(slot=0))]):
        assert launch(rows, lib, plan, guide, make_rescale(phi=0.1) if k == 0 else None) == 0  # (scale and phi of an emitted launch are the row's)
    assert lib.calls == [FACTOR[0], STEP[0], FACTOR[0], STEP[0]]
    for k in (0, 1):
        stat, step = lib.args[2 * k], lib.args[2 * k + 1]
        # uncond = inputs[slot], cond, dtype, numel, sample_numel, rows, index, the step's row offset, the hook's factor, no stats, the hook's partials
        assert stat[:11] == ((0xB000, 0xA000)[k], 0x1000, _hip.BF16, 8192, 4096, 0x7000, 0x8000, k, rows.factor.data_ptr(), None, rows.partials.data_ptr())
        assert step[4]._obj.factor_dev == rows.factor.data_ptr() and step[4]._obj.sample_numel == 4096 and step[4]._obj.reserved == 0
        assert step[7:10] == (0x7000, 0x8000, k)  # the same rows, index and row offset
        assert step[0]._obj.sample_numel == 4096  # a launch without noise carries no sample size: the captured batch gives it
    with pytest.raises(_hip.SkrampleHipError, match="more launches"):
        launch(rows, lib, make_plan(), make_guide())
    each = make_rows(batch=2)
    assert launch(each, lib, make_plan(), make_guide(), first) == 0
    each.length = 1
    each.begin("emit")
    lib.calls.clear(), lib.args.clear()
    assert launch(each, lib, make_plan(), make_guide(), first) == 0
    assert lib.calls == [FACTOR[1], STEP[1]] and lib.args[0][5:8] == (0x7000, 0x9000, 0) and lib.args[1][7:10] == (0x7000, 0x9000, 0)


def test_refill_moves_a_slot_between_phi_zero_and_phi_nonzero():
    lib = StubLib()
    rows = make_rows()
    assert launch(rows, lib, make_plan(), make_guide(), make_rescale()) == 0
    rows.length = 1
    rows.begin("refill", 1)
    other = make_plan(sample_numel=8192)  # a dry run on one sample: the sample size is shape-like
    assert launch(rows, lib, other, make_guide(scale=3.3), None, numel=8192) == 0  # phi == 0: a plain guided launch
    assert lib.calls[-1] == "skr_step_launch_guided" and rows.host[1].convert_k[0] == 3.3 and rows.host[1].convert_k[1] == 0.0
    rows.begin("refill", 2)
    assert launch(rows, lib, other, make_guide(scale=3.3), make_rescale(phi=0.25, sample_numel=8192), numel=8192) == 0
    assert lib.calls[-1] == "skr_step_launch_guided_rescaled" and rows.host[2].convert_k[1] == 0.25 and rows.host[0].convert_k[1] == 0.7


@pytest.mark.parametrize("what", ["slot", "stored", "plain_for_guided", "operand_count", "dtype"])
def test_refill_with_another_slot_or_structure_is_still_the_recapture_error(what):
    lib = StubLib()
    rows = make_rows()
    assert launch(rows, lib, make_plan(), make_guide(), make_rescale()) == 0
    rows.length = 1
    rows.begin("refill", 1)
    plan, guide, rescale = make_plan(), make_guide(), make_rescale()
    if what == "slot":
        guide = make_guide(slot=2)
    elif what == "stored":
        guide = make_guide(stored=False)
    elif what == "plain_for_guided":
        guide = rescale = None
    elif what == "operand_count":
        plan = make_plan(n=4)
    elif what == "dtype":
        plan = make_plan(dtype=_hip.F16)
    before = len(lib.calls)
    with pytest.raises(_hip.SkrampleHipError, match="different structure than the captured loop: re-capture"):
        launch(rows, lib, plan, guide, rescale)
    assert len(lib.calls) == before  # nothing was launched
    rows.begin("emit")
    with pytest.raises(_hip.SkrampleHipError, match="differs in structure between the recording pass and the capture"):
        launch(rows, lib, plan, guide, rescale)


@pytest.mark.parametrize(
    "plan_fields,numel,says",
    [
        ({"out0_dtype": _hip.NONE, "n_terms": 1, "n_group_a": 1}, 2 * 4096, "guidance-only"),  # UniPC / SPC, set_inpaint, compute_scale=None, channels-last
        ({"acc_f64": 1}, 2 * 4096, "float64"),  # compute_scale=float64
        ({"noise_mode": 0}, 2 * 4096 + 8, "2048"),  # a ragged launch
        ({"noise_mode": 0, "sample_numel": 0}, 2 * 3072, "rescaled guided rows need samples of whole 2048"),  # whole chunks in all, samples that are not
        ({"noise_mode": 0, "sample_numel": 0}, 3 * 2048, "rescaled guided rows need samples of whole 2048"),  # three chunks for two samples
        ({"sample_numel": 2048}, 2 * 4096, "the samples the noise is drawn by"),
    ],
)
@pytest.mark.parametrize("rescaled_launch", [True, False])
def test_record_mode_refuses_what_the_row_kernels_do_not_cover(plan_fields, numel, says, rescaled_launch):
    lib = StubLib()
    rows = make_rows()
    with pytest.raises(_hip.SkrampleHipError) as caught:
        launch(rows, lib, make_plan(**plan_fields), make_guide(slot=0), make_rescale() if rescaled_launch else None, numel=numel)
    assert "request outside kernel coverage" in str(caught.value) and says in str(caught.value)
    assert lib.calls == [] and rows.host == [] and rows.structures == [] and rows.factor is None  # refused before anything ran or was recorded


def test_the_wrappers_statistics_launch_runs_while_recording_and_is_not_emitted_again(monkeypatch):
    lib = StubLib()
    monkeypatch.setattr(_hip, "load", lambda: lib)
    monkeypatch.setattr(_hip, "current_stream_ptr", lambda device: None)
    u, factor = torch.zeros(2, 4096, dtype=torch.bfloat16), torch.zeros(2, dtype=torch.bfloat16)
    rows = make_rows()
    _hip.indexed = rows
    try:
        for mode, issued in (("record", 1), ("refill", 2), ("emit", 2)):
            rows.mode = mode
            _hip.launch_guidance_factor(u, u, 7.3, 4096, factor)
            assert lib.calls == ["skr_guidance_rescale_factor"] * issued, mode
        # the rescaled step goes through the recorder
        rows.mode = "record"
        _hip.launch_step_guided_rescaled(make_plan(), [u, u, u], u, u, u, 7.3, 1, factor, 0.7, 4096, torch.zeros(2, dtype=torch.int64), 8192, torch.device("cpu"))
        assert lib.calls[-1] == "skr_step_launch_guided_rescaled" and rows.host[0].convert_k[1] == 0.7 and rows.cursor == 1
    finally:
        _hip.indexed = None


def test_a_hook_without_rescaled_raises_as_before(monkeypatch):
    monkeypatch.setattr(_hip, "load", lambda: StubLib())
    u = torch.zeros(2, 4096, dtype=torch.bfloat16)
    guided_only = make_rows(rescaled=False)
    for hook in (guided_only, object()):
        _hip.indexed = hook
        try:
            with pytest.raises(_hip.SkrampleHipError, match="guidance_rescale.*no row form") as caught:
                _hip.launch_guidance_factor(u, u, 7.5, 4096, u)
            assert caught.value.args[0] == _hip.NO_RESCALED_ROWS and "rescaled=True" in _hip.NO_RESCALED_ROWS
            with pytest.raises(_hip.SkrampleHipError, match="guidance_rescale.*no row form"):
                _hip.launch_step_guided_rescaled(make_plan(), [u, u, u], u, u, u, 7.5, 1, u, 0.7, 4096, None, 8192, u.device)
        finally:
            _hip.indexed = None
    assert guided_only.host == [] and guided_only.cursor == 0


def test_capture_and_retarget_refuse_by_name_before_they_touch_a_device():
    w = PD.SkrampleWrapperScheduler(PT.Euler(), PS.Karras(PS.Scaled()))
    x = torch.zeros(2, 4, 32, 32)
    model = lambda x, t: (x, x)  # noqa: E731
    with pytest.raises(ValueError, match="rescaled=True needs indexed=True"):
        graphs.capture_sampling_loop(w, model, x, 4, guidance_scale=7.3, guidance_rescale=0.7, rescaled=True)
    with pytest.raises(ValueError, match="rescaled=True belongs to a guided loop"):
        graphs.capture_sampling_loop(w, model, x, 4, indexed=True, rescaled=True)
    with pytest.raises(ValueError, match="guidance_scale"):
        graphs.capture_sampling_loop(w, model, x, 4, indexed=True, guidance_rescale=0.7, rescaled=True)

    def loop_of(rescaled, guidance_scale=7.3):
        rows = _hip.IndexedRows(torch.device("cpu"), guided=guidance_scale is not None, rescaled=rescaled, samples=2 if rescaled else None)
        rows.upload = lambda slot: None  # (no device table to publish to)
        ran = []
        loop = graphs.CapturedLoop(None, x, x, None, rows, lambda *args: ran.append(args), guidance_scale=guidance_scale, guidance_rescale=0.7 if guidance_scale else 0.0, rescaled=rescaled)
        return loop, ran

    loop, ran = loop_of(False)
    with pytest.raises(ValueError, match="captured without rescaled=True"):
        loop.retarget(w, 1, guidance_rescale=0.25)
    with pytest.raises(ValueError, match="captured without rescaled=True"):
        loop.retarget(w, 1, guidance_rescale=0.0)
    assert ran == []
    loop, ran = loop_of(True)
    for bad, says in ((-0.5, "guidance_rescale must be >= 0"), (float("nan"), "guidance_rescale must be >= 0"), ("0.7", "guidance_rescale is a Python number"), (True, "guidance_rescale is a Python number")):
        with pytest.raises(_hip.SkrampleHipError, match=says):  # lazy.Guidance's messages
            loop.retarget(w, 1, guidance_rescale=bad)
    with pytest.raises(_hip.SkrampleHipError, match="the guidance scale is a Python number"):
        loop.retarget(w, 1, guidance_scale="7")
    assert ran == [] and loop.rows.mode == "record"  # refused before anything of the slot changed
    loop.retarget(w, 1, guidance_scale=3.3, guidance_rescale=0.25)
    loop.retarget(w, 2)  # None: the captured values
    loop.retarget(w, 2, guidance_rescale=0.0)
    assert [args[2:] for args in ran] == [(3.3, 0.25), (7.3, 0.7), (7.3, 0.0)]
