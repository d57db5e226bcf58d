"""Guided steps with device-resident rows, without a device: the two C ABI declarations and their binding, and the row recorder
(_hip.IndexedRows) with guided launches in its record, refill and emit modes, driven with a stub library whose launch functions return 0.
The guidance scale of a guided launch is a row value: it sits in convert_k[0], which a guided plan (convert_* == 0) leaves free."""

import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from skrample_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("skr_step_launch_guided_indexed", "skr_step_launch_guided_indexed_per_sample")
OK, NULL, DTYPE, TERMS, ALIGN, SHAPE, LAUNCH, UNSUPPORTED = range(8)


def test_header_declares_the_two_entries_and_the_binding_lists_them():
    header = open(os.path.join(ROOT, "include", "skrample_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    ws = r"\s*"
    common = (r"const\s+skr_step_plan\s*\*\s*plan", r"const\s+void\s*\*\s*const\s*\*\s*inputs", r"void\s*\*\s*out", r"const\s+skr_step_guidance\s*\*\s*guide",
              r"const\s+uint64_t\s*\*\s*seeds_dev", r"int64_t\s+numel", r"const\s+skr_step_row\s*\*\s*rows_dev")  # fmt: skip
    tails = {NAMES[0]: r"const\s+int32_t\s*\*\s*index_dev", NAMES[1]: r"const\s+int32_t\s*\*\s*sample_index_dev"}
    for name in NAMES:
        args = (*common, tails[name], r"int32_t\s+row_offset", r"void\s*\*\s*stream")
        assert re.search(rf"^int\s+{name}{ws}\({ws}" + rf"{ws},{ws}".join(args) + rf"{ws}\){ws};", flat, flags=re.M), name
        assert name in _hip.EXPORTS
    assert re.search(r"#define\s+SKR_ABI_VERSION\s+15\b", header) and _hip.ABI_VERSION == 15  # purely additive
    assert re.search(r"#define\s+SKR_ROW_TERMS\s+16\b", header) and _hip.ROW_TERMS == 16
    assert ctypes.sizeof(_hip.StepRowC) == 328 and _hip.StepRowC.convert_k.offset == 296  # the row keeps its layout: the scale found a free field
    assert ctypes.sizeof(_hip.StepGuidanceC) == 32


def test_header_is_still_plain_c_and_the_row_keeps_its_size(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc on this box")
    src = tmp_path / "client.c"
    src.write_text(
        "#include <stddef.h>\n"
        f'#include "{os.path.join(ROOT, "include", "skrample_hip.h")}"\n'
        '_Static_assert(sizeof(skr_step_row) == 328, "row size");\n'
        '_Static_assert(offsetof(skr_step_row, convert_k) == 296, "where the scale sits");\n'
        '_Static_assert(sizeof(skr_step_guidance) == 32, "guidance size");\n'
        "int main(void) {\n"
        "  int (*whole)(const skr_step_plan*, const void* const*, void*, const skr_step_guidance*, const uint64_t*, int64_t, const skr_step_row*,\n"
        f"               const int32_t*, int32_t, void*) = {NAMES[0]};\n"
        "  int (*each)(const skr_step_plan*, const void* const*, void*, const skr_step_guidance*, const uint64_t*, int64_t, const skr_step_row*,\n"
        f"              const int32_t*, int32_t, void*) = {NAMES[1]};\n"
        "  (void)whole; (void)each;\n"
        f"  return SKR_ABI_VERSION == {_hip.ABI_VERSION} ? 0 : 1;\n"
        "}\n"
    )
    done = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c", str(src), "-o", str(tmp_path / "client.o")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


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
    buf = (ctypes.c_char * 512)()
    base = (ctypes.addressof(buf) + 15) & ~15
    a, b, c, out, cond, gout, seeds, rows, index = (base + 48 * k for k in range(9))
    for name in NAMES:
        entry = getattr(lib, name)
        assert len(entry.argtypes) == 10 and entry.restype is ctypes.c_int

        def call(plan=None, slot=1, rows=rows, index=index, row_offset=0, seeds=seeds, numel=8192, out=out, reserved=0):
            plan = plan if plan is not None else make_plan()
            arr = (ctypes.c_void_p * 3)(a, b, c)
            guide = _hip.StepGuidanceC(cond, gout, 7.5, slot, reserved)
            return entry(ctypes.byref(plan), arr, out, ctypes.byref(guide), seeds, numel, rows, index, row_offset, None)

        per_sample = name.endswith("per_sample")
        assert call(rows=None) == NULL
        assert call(index=None, numel=0) == (NULL if per_sample else OK)
        assert call(seeds=None, plan=make_plan(zeta0=0.0)) == NULL  # noise_mode 1 needs seeds whatever the plan (or a row) holds
        assert call(rows=None, slot=7) == NULL and call(slot=7, numel=-1) == TERMS and call(numel=-1, reserved=1) == SHAPE
        assert call(reserved=1, row_offset=-1) == UNSUPPORTED and call(plan=make_plan(convert_to=1)) == UNSUPPORTED
        assert call(out=out + 4, row_offset=-1) == ALIGN and call(plan=make_plan(out0_dtype=_hip.F16), row_offset=-1) == DTYPE
        assert call(row_offset=-1) == UNSUPPORTED
        assert call(numel=8192 + 8, plan=make_plan(noise_mode=0)) == UNSUPPORTED  # ragged: no grid-stride row form
        assert call(plan=make_plan(acc_f64=1)) == UNSUPPORTED and call(plan=make_plan(n_group_a=2)) == UNSUPPORTED
        if per_sample:  # a workgroup lies inside one sample, with or without noise
            assert call(plan=make_plan(noise_mode=0, sample_numel=0)) == SHAPE and call(plan=make_plan(noise_mode=0, sample_numel=8192 - 2048)) == SHAPE
            assert call(plan=make_plan(noise_mode=0, sample_numel=1024)) == UNSUPPORTED
    assert bytes(buf) == bytes(512)  # nothing was written


class StubLib:
    "stands for the library: every launch returns 0 and is remembered by name with its arguments"

    def __init__(self):
        self.calls, self.args = [], []

    def skr_strerror(self, code):
        return {7: b"request outside kernel coverage"}.get(code, b"error")

    def __getattr__(self, name):
        if not name.startswith("skr_step_launch"):
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


def make_rows(batch=None):
    rows = _hip.IndexedRows.__new__(_hip.IndexedRows)  # (no device tensors: the fields record / refill touch)
    rows.device, rows.slots, rows.batch, rows.guided = torch.device("cpu"), 3, batch, True
    rows.mode, rows.cursor, rows.length, rows.slot = "record", 0, 0, 0
    rows.structures, rows.shapeless, rows.host = [], [], []
    rows.rows_dev, rows.index_dev, rows.sample_index_dev = Pointer(0x7000), Pointer(0x8000), Pointer(0x9000) if batch is not None else None
    return rows


def make_guide(scale=7.3, slot=1, stored=True):
    return _hip.StepGuidanceC(0x1000, 0x3000 if stored else None, scale, slot, 0)


def launch(rows, lib, plan, guide, numel=2 * 4096):
    return rows.launch(lib, plan, None, 0x2000, None, 0x4000, numel, None, guide=guide)


def test_a_guided_launch_is_recorded_with_its_scale_in_convert_k0_and_run_through_the_guided_entry():
    lib = StubLib()
    rows = make_rows()
    plan = make_plan()
    assert launch(rows, lib, plan, make_guide()) == 0 and launch(rows, lib, make_plan(), None) == 0
    assert lib.calls == ["skr_step_launch_guided", "skr_step_launch"]
    row = rows.host[0]
    assert row.convert_k[0] == 7.3 and [row.convert_k[k] for k in (1, 2, 3)] == [0.0, 0.0, 0.0]
    assert [row.coef0[k] for k in range(3)] == [1.0, 2.0, 3.0] and row.zeta0 == 0.5 and row.stream0 == 513
    assert rows.host[1].convert_k[0] == 0.0  # (a plain launch keeps the plan's conversion constants)
    # the structure says that the launch is guided, which operand the guided value replaces and whether it is stored; the scale is data
    full, shapeless = rows.structures[0], rows.shapeless[0]
    assert full[-3:] == ("guided", 1, True) and shapeless[-3:] == ("guided", 1, True)
    assert 4096 in full and 4096 not in shapeless
    assert rows.structures[1] == _hip.plan_structure(make_plan()) and "guided" not in rows.structures[1]
    assert _hip.plan_structure(plan, guide=make_guide(scale=1.5)) == full
    assert _hip.plan_structure(plan, guide=make_guide(stored=False))[-1] is False


def test_refill_writes_another_scale_and_emit_launches_the_row_forms():
    lib = StubLib()
    rows = make_rows()
    assert launch(rows, lib, make_plan(), make_guide()) == 0
    rows.length = 1
    rows.begin("refill", 2)
    other = make_plan(sample_numel=8192)  # a dry run on one sample: the sample size is shape-like
    other.coef0[2] = 9.0
    assert launch(rows, lib, other, make_guide(scale=3.3), numel=8192) == 0
    assert lib.calls[-1] == "skr_step_launch_guided"
    assert len(rows.host) == 3 and rows.host[2].convert_k[0] == 3.3 and rows.host[2].coef0[2] == 9.0 and rows.host[0].convert_k[0] == 7.3
    with pytest.raises(_hip.SkrampleHipError, match="more launches"):
        launch(rows, lib, make_plan(), make_guide())
    rows.begin("emit")
    assert launch(rows, lib, make_plan(), make_guide(scale=-1.0)) == 0  # (the scale of an emitted launch is the row's, not the descriptor's)
    assert lib.calls[-1] == NAMES[0] and lib.args[-1][6:9] == (0x7000, 0x8000, 0)
    each = make_rows(batch=2)
    assert launch(each, lib, make_plan(noise_mode=0, sample_numel=0, zeta0=0.0), make_guide()) == 0
    each.length = 1
    each.begin("emit")
    assert launch(each, lib, make_plan(noise_mode=0, sample_numel=0, zeta0=0.0), make_guide()) == 0
    assert lib.calls[-1] == NAMES[1] and lib.args[-1][6:9] == (0x7000, 0x9000, 0)
    assert lib.args[-1][0]._obj.sample_numel == 4096  # a launch without noise carries no sample size: the captured batch gives it


@pytest.mark.parametrize("what", ["slot", "stored", "plain_for_guided", "guided_for_plain", "operand_count", "dtype"])
def test_refill_rejects_a_launch_with_another_slot_or_structure(what):
    lib = StubLib()
    rows = make_rows()
    assert launch(rows, lib, make_plan(), None if what == "guided_for_plain" else make_guide()) == 0
    rows.length = 1
    rows.begin("refill", 1)
    plan, guide = make_plan(), make_guide()
    if what == "slot":
        guide = make_guide(slot=2)
    elif what == "stored":
        guide = make_guide(stored=False)
    elif what == "plain_for_guided":
        guide = None
    elif what == "operand_count":
        plan = make_plan(n=4)
    elif what == "dtype":
        plan = make_plan(dtype=_hip.F16)
    before = len(lib.calls)
    with pytest.raises(_hip.SkrampleHipError, match="different structure than the captured loop: re-capture"):
        launch(rows, lib, plan, guide)
    assert len(lib.calls) == before  # nothing was launched
    rows.begin("emit")
    if what != "guided_for_plain":
        with pytest.raises(_hip.SkrampleHipError, match="differs in structure between the recording pass and the capture"):
            launch(rows, lib, plan, guide)


@pytest.mark.parametrize(
    "plan_fields,numel,says",
    [
        ({"out0_dtype": _hip.NONE, "n_terms": 1, "n_group_a": 1}, 2 * 4096, "guidance-only"),  # UniPC / SPC, set_inpaint, compute_scale=None, channels-last
        ({"acc_f64": 1}, 2 * 4096, "float64"),  # compute_scale=float64
        ({"n_group_a": 2}, 2 * 4096, "one 16- or 32-bit dtype"),  # a second dtype group (fp32)
        ({"out0_dtype": _hip.F32}, 2 * 4096, "one 16- or 32-bit dtype"),
        ({"dtype_a": _hip.F64, "out0_dtype": _hip.F64}, 2 * 4096, "one 16- or 32-bit dtype"),
        ({"sample_numel": 1024}, 2 * 1024, "2048"),  # samples below a chunk under a draw
        ({"noise_mode": 0}, 2 * 4096 + 8, "2048"),  # a ragged launch
    ],
)
def test_record_mode_refuses_what_the_row_kernel_does_not_cover(plan_fields, numel, says):
    lib = StubLib()
    rows = make_rows()
    with pytest.raises(_hip.SkrampleHipError) as caught:
        launch(rows, lib, make_plan(**plan_fields), make_guide(slot=0), numel=numel)
    assert "request outside kernel coverage" in str(caught.value) and says in str(caught.value)
    assert lib.calls == [] and rows.host == [] and rows.structures == []  # refused before anything ran or was recorded


def test_a_hook_not_created_for_guidance_still_raises_with_the_reason(monkeypatch):
    "a loop captured without guidance_scale, or any other object installed as the hook"
    monkeypatch.setattr(_hip, "load", lambda: StubLib())
    plain = make_rows()
    plain.guided = False
    bare = make_rows()
    del bare.guided  # (a recorder built by hand, as the other host tests build theirs)
    u = torch.zeros(8)
    for hook in (plain, bare, object()):
        _hip.indexed = hook
        try:
            with pytest.raises(_hip.SkrampleHipError, match="captured loops"):
                _hip.launch_step_guided(make_plan(), [u, u, u], u, u, u, 7.5, 1, None, 8, torch.device("cpu"))
        finally:
            _hip.indexed = None
    assert plain.host == [] and plain.cursor == 0


def test_no_cyclic_collection_runs_while_a_loop_is_captured():
    "graphs._no_collection: the collector is off inside (a dead cycle around a captured loop must not be destroyed under a capturing stream), and as it was afterwards"
    import gc

    from skrample_amd import graphs

    class Cycle:
        def __init__(self, log):
            self.me, self.log = self, log

        def __del__(self):
            self.log.append(gc.isenabled())

    assert gc.isenabled()
    log = []
    with graphs._no_collection():
        assert not gc.isenabled()
        for _ in range(3 * gc.get_threshold()[0]):  # allocations enough to tip the collector's counters, were it on
            Cycle(log)
        assert log == []  # nothing was collected
    assert gc.isenabled()
    gc.collect()
    assert log and all(log)  # the cycles were collected afterwards, outside
    with pytest.raises(RuntimeError):
        with graphs._no_collection():
            raise RuntimeError("a refused capture")
    assert gc.isenabled()
    gc.disable()
    try:
        with graphs._no_collection():
            pass
        assert not gc.isenabled()  # (a caller's own setting is kept)
    finally:
        gc.enable()
    source = open(graphs.__file__).read()
    assert source.count("torch.cuda.graph(graph)") == source.count("with _no_collection(), torch.cuda.graph(graph)") == 2
