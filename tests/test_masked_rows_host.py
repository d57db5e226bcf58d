"""Masked steps with device-resident rows, without a device: the two C ABI declarations and their binding, and the row recorder
(_hip.IndexedRows) in its record and refill modes, driven with a stub library whose launch functions return 0."""

import ctypes
import os
import re

import pytest
import torch

from skrample_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("skr_step_launch_masked_indexed", "skr_step_launch_masked_indexed_per_sample")


def test_header_declares_the_two_entries_and_the_binding_lists_them():
    header = open(os.path.join(ROOT, "include", "skrample_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    ws = r"\s*"
    common = (r"const\s+skr_step_plan\s*\*\s*plan", r"const\s+void\s*\*\s*const\s*\*\s*inputs", r"void\s*\*\s*out", r"const\s+skr_step_mask\s*\*\s*mask",
              r"const\s+uint64_t\s*\*\s*seeds_dev", r"int64_t\s+numel", r"const\s+skr_step_row\s*\*\s*rows_dev")  # fmt: skip
    tails = {NAMES[0]: r"const\s+int32_t\s*\*\s*index_dev", NAMES[1]: r"const\s+int32_t\s*\*\s*sample_index_dev"}
    for name in NAMES:
        args = (*common, tails[name], r"int32_t\s+row_offset", r"void\s*\*\s*stream")
        assert re.search(rf"^int\s+{name}{ws}\({ws}" + rf"{ws},{ws}".join(args) + rf"{ws}\){ws};", flat, flags=re.M), name
        assert name in _hip.EXPORTS
    assert re.search(r"#define\s+SKR_ABI_VERSION\s+15\b", header) and _hip.ABI_VERSION == 15  # purely additive
    assert re.search(r"#define\s+SKR_ROW_TERMS\s+16\b", header) and _hip.ROW_TERMS == 16
    if os.path.isfile(_hip.LIB_PATH):
        lib = _hip.load()
        for name in NAMES:
            entry = getattr(lib, name)
            assert len(entry.argtypes) == 10 and entry.restype is ctypes.c_int
        assert lib.skr_abi_version() == 15
        # argument checks run on the host, ahead of any device work
        plan, desc = _hip.StepPlanC(), _hip.StepMaskC()
        for name in NAMES:
            assert getattr(lib, name)(ctypes.byref(plan), None, None, ctypes.byref(desc), None, 8, None, None, 0, None) == 1  # SKR_ERR_NULL: no rows


class StubLib:
    "stands for the library: every launch returns 0 and is remembered by name"

    def __init__(self):
        self.calls = []

    def skr_strerror(self, code):
        return {7: b"request outside kernel coverage"}.get(code, b"error")

    def __getattr__(self, name):
        if not name.startswith("skr_step_launch"):
            raise AttributeError(name)

        def launch(*args):
            self.calls.append(name)
            return 0

        return launch


def make_rows(batch=None):
    rows = _hip.IndexedRows.__new__(_hip.IndexedRows)  # (no device tensors: the fields record / refill touch)
    rows.device, rows.slots, rows.batch = torch.device("cpu"), 3, batch
    rows.mode, rows.cursor, rows.length, rows.slot = "record", 0, 0, 0
    rows.structures, rows.shapeless, rows.host = [], [], []
    rows.rows_dev, rows.index_dev, rows.sample_index_dev = None, None, None
    return rows


def make_plan(n=3, dtype=_hip.BF16, sample_numel=4096, **fields):
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = n
    plan.dtype_a = plan.out0_dtype = dtype
    plan.dtype_b, plan.out1_dtype = _hip.F32, _hip.NONE
    plan.sample_numel = sample_numel
    for k in range(n):
        plan.coef0[k], plan.coef1[k] = 1.0 + k, -0.25 * (k + 1)
    plan.zeta0, plan.stream0 = 0.5, 513
    for key, value in fields.items():
        setattr(plan, key, value)
    return plan


def make_mask(dtype=_hip.BF16, mask_numel=1024, batch_stride=1024):
    return _hip.StepMaskC(0x1000, dtype, 0, mask_numel, batch_stride)


def launch(rows, lib, plan, mask, numel=2 * 4096):
    return rows.launch(lib, plan, None, 0x2000, None, None, numel, None, mask=mask)


def recorded(lib, masks=(True,)):
    "a recorder with one launch recorded per entry of `masks` (masked or plain), switched to refill mode for slot 1"
    rows = make_rows()
    for masked in masks:
        assert launch(rows, lib, make_plan(), make_mask() if masked else None) == 0
    rows.length = len(rows.host)
    rows.begin("refill", 1)
    return rows


def test_a_masked_launch_is_recorded_with_its_known_form_and_run_through_the_masked_entry():
    lib = StubLib()
    rows = make_rows()
    plan = make_plan()
    assert launch(rows, lib, plan, make_mask()) == 0 and launch(rows, lib, make_plan(), None) == 0
    assert lib.calls == ["skr_step_launch_masked", "skr_step_launch"]
    row = rows.host[0]
    assert [row.coef1[k] for k in range(3)] == [plan.coef1[k] for k in range(3)] == [-0.25, -0.5, -0.75]
    assert [row.coef0[k] for k in range(3)] == [1.0, 2.0, 3.0] and row.zeta0 == 0.5 and row.stream0 == 513
    assert all(row.coef1[k] == 0.0 for k in range(3, _hip.ROW_TERMS))
    # the structure says that the launch is masked, with which mask dtype and whether one mask serves the batch; mask_numel is shape-like
    full, shapeless = rows.structures[0], rows.shapeless[0]
    assert full[-4:] == ("masked", _hip.BF16, False, 1024) and shapeless[-4:] == ("masked", _hip.BF16, False, None)
    assert 4096 in full and 4096 not in shapeless  # (sample_numel goes the same way)
    assert rows.structures[1] == _hip.plan_structure(make_plan()) and "masked" not in rows.structures[1]
    assert _hip.plan_structure(plan, mask=make_mask(batch_stride=0))[-2] is True


def test_refill_overwrites_the_slot_and_checks_the_structure():
    lib = StubLib()
    rows = recorded(lib, (True, False))
    other = make_plan()
    other.coef1[0], other.coef0[2] = 0.125, 7.0
    # a dry run on one sample: its mask_numel and sample size may differ (shape-like), and it has no batch stride to compare
    assert launch(rows, lib, make_plan(sample_numel=8192), make_mask(mask_numel=2048, batch_stride=0), numel=8192) == 0
    rows.begin("refill", 1)
    assert launch(rows, lib, other, make_mask()) == 0 and launch(rows, lib, make_plan(), None) == 0
    assert lib.calls[-2:] == ["skr_step_launch_masked", "skr_step_launch"]
    assert len(rows.host) == 4 and rows.host[2].coef1[0] == 0.125 and rows.host[2].coef0[2] == 7.0 and rows.host[0].coef1[0] == -0.25
    with pytest.raises(_hip.SkrampleHipError, match="more launches"):
        launch(rows, lib, make_plan(), None)


@pytest.mark.parametrize("what", ["plain_for_masked", "masked_for_plain", "mask_dtype", "stride_0_for_per_sample", "per_sample_for_stride_0", "operand_count"])
def test_structure_mismatches_are_the_re_capture_error(what):
    lib = StubLib()
    base_mask = make_mask(batch_stride=0) if what == "per_sample_for_stride_0" else make_mask()
    rows = make_rows()
    masked_first = what != "masked_for_plain"
    assert launch(rows, lib, make_plan(), base_mask if masked_first else None) == 0
    rows.length = 1
    rows.begin("refill", 1)
    plan, mask = make_plan(), make_mask()
    if what == "plain_for_masked":
        mask = None
    elif what == "mask_dtype":
        mask = make_mask(dtype=_hip.F16)
    elif what == "stride_0_for_per_sample":
        mask = make_mask(batch_stride=0)
    elif what == "operand_count":
        plan = make_plan(n=4)
    before = len(lib.calls)
    with pytest.raises(_hip.SkrampleHipError, match="different structure than the captured loop: re-capture"):
        launch(rows, lib, plan, mask)  # (two samples: the batch stride is compared)
    assert len(lib.calls) == before  # nothing was launched


def test_the_capture_pass_checks_the_full_structure():
    "emit mode: mask_numel and the batch stride are part of what the recording pass froze"
    lib = StubLib()
    for changed in (make_mask(mask_numel=2048, batch_stride=2048), make_mask(batch_stride=0), None):
        rows = make_rows()
        assert launch(rows, lib, make_plan(), make_mask()) == 0
        rows.length = 1
        rows.begin("emit")
        with pytest.raises(_hip.SkrampleHipError, match="differs in structure between the recording pass and the capture"):
            launch(rows, lib, make_plan(), changed)


@pytest.mark.parametrize(
    "plan_fields,mask_fields,numel,says",
    [
        ({"sample_numel": 1024}, {}, 2 * 1024, "2048"),  # samples below a chunk
        ({"sample_numel": 35 * 2048}, {"mask_numel": 35, "batch_stride": 35}, 2 * 35 * 2048, "multiple of 8"),
        ({"n_group_a": 2}, {}, 2 * 4096, "one 16- or 32-bit dtype"),  # a second dtype group (fp32)
        ({"out0_dtype": _hip.F32}, {}, 2 * 4096, "one 16- or 32-bit dtype"),
        ({}, {"dtype": _hip.F32}, 2 * 4096, "one 16- or 32-bit dtype"),
        ({"acc_f64": 1}, {}, 2 * 4096, "float64"),  # compute_scale=float64
    ],
)
def test_record_mode_refuses_what_the_row_kernel_does_not_cover(plan_fields, mask_fields, numel, says):
    lib = StubLib()
    rows = make_rows()
    with pytest.raises(_hip.SkrampleHipError) as caught:
        launch(rows, lib, make_plan(**plan_fields), make_mask(**mask_fields), numel=numel)
    assert "request outside kernel coverage" in str(caught.value) and says in str(caught.value)
    assert lib.calls == [] and rows.host == [] and rows.structures == []  # refused before anything ran or was recorded
    assert launch(make_rows(), lib, make_plan(**plan_fields), None, numel=numel) == 0  # (a plain launch of that plan is not this check's business)


def test_a_per_sample_recorder_still_asks_for_whole_chunks_first():
    lib = StubLib()
    rows = make_rows(batch=2)
    with pytest.raises(_hip.SkrampleHipError, match="per-sample rows need samples of whole 2048-element chunks"):
        launch(rows, lib, make_plan(sample_numel=1024), make_mask(), numel=2 * 1024)
