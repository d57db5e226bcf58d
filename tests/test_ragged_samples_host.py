"""Ragged samples without a GPU: which sample sizes `RollingBatch` and the recorder of captured loops (`_hip.IndexedRows`) let through to
the ragged form of the table launches (csrc/skr_step_ragged.hip), on stub rows and a stub library -- nothing here enqueues device work --
and what the C entries answer where every check precedes the launch."""

import ctypes

import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.rolling import RollingBatch
from skrample_amd.sampling import structured as PT

WIDE = [("x",), ("o",), ("pi", -1), ("po", -1)]


def stub_plan(n_terms: int, two: bool = False) -> _hip.StepPlanC:
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = n_terms
    plan.dtype_a = plan.dtype_b = plan.out0_dtype = _hip.BF16
    plan.out1_dtype = _hip.BF16 if two else _hip.NONE
    for k in range(n_terms):
        plan.coef0[k] = 1.0 + k
    return plan


class StubBatch(RollingBatch):
    "the dry run gives a DPM-2-like ramp-up (2, 4, 4, ... operands); launches are counted, not made"

    launches = 0
    two = False

    def _trace(self, wrapper, steps, seed):
        return [(stub_plan(min(2 * (i + 1), 4), two=self.two), WIDE[: min(2 * (i + 1), 4)], 100.0 - i) for i in range(steps)]

    def _launch(self, arr, out0, out1):
        self.launches += 1


class TwoOutputBatch(StubBatch):
    two = True


def wrapper():
    return PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Scaled())


def test_the_sample_sizes_the_ragged_form_takes():
    for sn, ok in ((2304, True), (2056, True), (64512, True), (2**31 - 8, True), (2048, False), (65536, False), (1024, False), (2040, False), (2052, False), (2500, False),
                   (2**31 + 8, False), (0, False)):  # fmt: skip
        assert _hip.ragged_sample(sn) is ok, sn
    # every usual SDXL latent bucket is whole chunks or ragged: all of them are served
    for h, w in ((128, 128), (160, 96), (192, 80), (144, 112), (168, 96), (152, 104), (176, 88), (184, 88), (200, 80), (216, 72)):
        for sn in (4 * h * w,):
            assert sn % 2048 == 0 or _hip.ragged_sample(sn), (h, w)


def test_the_constructor_accepts_ragged_units_and_keeps_its_refusals():
    batch = StubBatch(wrapper, torch.zeros(4, 4, 24, 24, dtype=torch.bfloat16), capacity=4)  # 2304 elements a sample
    assert batch.ragged and batch.sample_numel == 2304 and batch.plan.sample_numel == 2304 and batch.numel == 4 * 2304
    x = torch.ones(4, 24, 24, dtype=torch.bfloat16)
    batch.admit(1, x, wrapper(), 3)
    assert batch.index_vector() == [-1, 128, -1, -1]
    assert batch.step(torch.zeros(4, 4, 24, 24, dtype=torch.bfloat16)) == [] and batch.launches == 1
    assert not StubBatch(wrapper, torch.zeros(4, 4, 32, 32, dtype=torch.bfloat16), capacity=4).ragged
    with pytest.raises(ValueError, match="per-sample rows need samples of whole 2048-element chunks, not 1024 elements"):
        StubBatch(wrapper, torch.zeros(4, 4, 16, 16, dtype=torch.bfloat16), capacity=4)
    with pytest.raises(ValueError, match="per-sample rows need samples of whole 2048-element chunks, not 2500 elements"):  # no multiple of 8
        StubBatch(wrapper, torch.zeros(4, 4, 25, 25, dtype=torch.bfloat16), capacity=4)


def test_the_constructor_refuses_what_has_no_ragged_kernel():
    example = torch.zeros(4, 4, 24, 24, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="guided together with ragged samples"):
        StubBatch(wrapper, example, capacity=4, guided=True)
    with pytest.raises(ValueError, match="inpaint_mask_shape together with ragged samples"):
        StubBatch(wrapper, example, capacity=4, inpaint_mask_shape=(1, 24, 24))
    with pytest.raises(_hip.SkrampleHipError, match="UniPC on ragged samples"):
        StubBatch(lambda: PD.SkrampleWrapperScheduler(PT.UniPC(order=2), PS.Scaled()), example, capacity=4)
    with pytest.raises(_hip.SkrampleHipError, match="SPC on ragged samples"):
        StubBatch(lambda: PD.SkrampleWrapperScheduler(PT.SPC(), PS.Scaled()), example, capacity=4)
    with pytest.raises(_hip.SkrampleHipError, match="ragged samples .* single-output launches only"):  # whatever else the dry run turns up
        TwoOutputBatch(wrapper, example, capacity=4)
    TwoOutputBatch(wrapper, torch.zeros(4, 4, 32, 32, dtype=torch.bfloat16), capacity=4)  # whole chunks: as ever


# ---- the recorder of captured loops -------------------------------------------------------------------------------------------------
class StubLib:
    "stands for the library: every launch returns 0 and is remembered by name with its plan's sample size"

    def __init__(self):
        self.calls = []

    def skr_strerror(self, code):
        return {7: b"request outside kernel coverage"}.get(code, b"error")

    def __getattr__(self, name):
        if not name.startswith("skr_step_launch"):
            raise AttributeError(name)

        def launch(plan, *args):
            self.calls.append((name, plan._obj.sample_numel))
            return 0

        return launch


def make_rows(batch=None, samples=None):
    rows = _hip.IndexedRows.__new__(_hip.IndexedRows)  # (no device tensors: the fields record / emit touch)
    rows.device, rows.slots, rows.batch, rows.samples = torch.device("cpu"), 3, batch, samples
    rows.guided = rows.rescaled = False
    rows.mode, rows.cursor, rows.length, rows.slot = "record", 0, 0, 0
    rows.structures, rows.shapeless, rows.host = [], [], []
    rows.rows_dev = rows.index_dev = torch.zeros(1, dtype=torch.int32)
    rows.sample_index_dev = torch.zeros(batch, dtype=torch.int32) if batch is not None else None
    return rows


def make_plan(n=3, sample_numel=2304, **fields):
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = n
    plan.dtype_a = plan.dtype_b = plan.out0_dtype = _hip.BF16
    plan.out1_dtype = _hip.NONE
    plan.sample_numel = sample_numel
    for key, value in fields.items():
        setattr(plan, key, value)
    return plan


def launch(rows, lib, plan, numel, **more):
    return rows.launch(lib, plan, None, 0x2000, None, None, numel, None, **more)


@pytest.mark.parametrize("batch", [None, 3])
def test_record_mode_lets_a_ragged_single_output_launch_through(batch):
    lib, rows = StubLib(), make_rows(batch=batch, samples=3)
    assert launch(rows, lib, make_plan(noise_mode=1), 3 * 2304) == 0
    assert launch(rows, lib, make_plan(sample_numel=0), 3 * 2304) == 0  # a launch without noise carries no sample size
    assert [name for name, _ in lib.calls] == ["skr_step_launch"] * 2 and len(rows.host) == 2
    rows.length = 2
    rows.begin("emit")
    assert launch(rows, lib, make_plan(noise_mode=1), 3 * 2304) == 0 and launch(rows, lib, make_plan(sample_numel=0), 3 * 2304) == 0
    entry = "skr_step_launch_indexed_per_sample" if batch else "skr_step_launch_indexed"
    assert lib.calls[2:] == [(entry, 2304), (entry, 2304)]  # the captured batch gave the second one its sample size


def test_emit_leaves_whole_chunk_launches_without_a_sample_size_alone():
    lib, rows = StubLib(), make_rows(samples=2)
    assert launch(rows, lib, make_plan(sample_numel=0), 2 * 3072) == 0  # whole chunks in all: the whole-chunk kernel takes it, as ever
    rows.length = 1
    rows.begin("emit")
    assert launch(rows, lib, make_plan(sample_numel=0), 2 * 3072) == 0
    assert lib.calls[-1] == ("skr_step_launch_indexed", 0)


@pytest.mark.parametrize("batch", [None, 3])
@pytest.mark.parametrize("fields", [dict(out1_dtype=_hip.BF16), dict(out1_dtype=_hip.BF16, convert_to=1, convert_from=2), dict(acc_f64=1)], ids=["two_outputs", "conversion", "acc_f64"])
def test_record_mode_refuses_any_other_ragged_launch_before_any_capture(fields, batch):
    lib, rows = StubLib(), make_rows(batch=batch, samples=3)
    with pytest.raises(_hip.SkrampleHipError, match="request outside kernel coverage: ragged samples"):
        launch(rows, lib, make_plan(noise_mode=1, **fields), 3 * 2304)
    assert lib.calls == [] and rows.host == []  # nothing ran, nothing was recorded
    assert launch(rows, lib, make_plan(sample_numel=4096, noise_mode=1, **fields), 3 * 4096) == 0  # whole chunks: the library decides, as ever


def test_record_mode_keeps_its_refusals_for_per_sample_rows():
    lib = StubLib()
    for numel in (3 * 1024, 3 * 2052, 3 * 2304 + 8):  # below a chunk, no multiple of 8, not the batch's samples
        with pytest.raises(_hip.SkrampleHipError, match="per-sample rows need samples of whole 2048-element chunks"):
            launch(make_rows(batch=3), lib, make_plan(sample_numel=0), numel)
    mask = _hip.StepMaskC(0x1000, _hip.BF16, 0, 2304, 2304)
    with pytest.raises(_hip.SkrampleHipError, match="per-sample rows need samples of whole 2048-element chunks"):  # masked rows have no ragged form
        launch(make_rows(batch=3), lib, make_plan(), 3 * 2304, mask=mask)
    with pytest.raises(_hip.SkrampleHipError, match="masked rows need samples of whole 2048-element chunks"):
        launch(make_rows(samples=3), lib, make_plan(), 3 * 2304, mask=mask)
    assert lib.calls == []


# ---- the C entries: every check precedes the launch -----------------------------------------------------------------------------------
def test_argument_checks_of_the_row_entries_without_gpu():
    "host buffers stand in (16-byte aligned; no check dereferences them): what stays refused, with the codes and the order it had"
    lib = _hip.load()
    rows = (_hip.StepRowC * 1)()
    index = (ctypes.c_int32 * 4)()
    buf = (ctypes.c_char * 64)()
    base = (ctypes.addressof(buf) + 15) & ~15
    ptrs = (ctypes.c_void_p * 2)(base, base)
    seeds = (ctypes.c_uint64 * 4)()
    table = (ctypes.addressof(rows), ctypes.addressof(index), 0, None)
    for name in ("skr_step_launch_indexed", "skr_step_launch_indexed_per_sample", "skr_step_launch_rolling"):
        call = getattr(lib, name)
        per_sample = name != "skr_step_launch_indexed"
        for noise_mode in (0, 1):
            sd = ctypes.addressof(seeds) if noise_mode else None
            for sample in (1024, 264, 2052):
                plan = make_plan(n=2, sample_numel=sample, noise_mode=noise_mode)
                assert call(ctypes.byref(plan), ptrs, base, None, sd, 3 * sample, *table) == 7, (name, sample)  # SKR_ERR_UNSUPPORTED
            for fields in (dict(out1_dtype=_hip.BF16), dict(out1_dtype=_hip.BF16, convert_to=1, convert_from=2), dict(acc_f64=1), dict(n_terms=17, n_group_a=17)):
                plan = make_plan(n=2, noise_mode=noise_mode, **fields)
                many = (ctypes.c_void_p * 17)(*([base] * 17))
                assert call(ctypes.byref(plan), many, base, base, sd, 3 * 2304, *table) == 7, (name, fields)
            plan = make_plan(n=2, noise_mode=noise_mode)
            # samples that do not divide numel: SKR_ERR_SHAPE wherever the form needs the sample size (a whole-batch launch without noise does not)
            assert call(ctypes.byref(plan), ptrs, base, None, sd, 3 * 2304 + 8, *table) == (5 if per_sample or noise_mode else 7), name
            assert call(ctypes.byref(plan), ptrs, base, None, sd, 3 * 2304, table[0], table[1], -1, None) == 7  # a negative row offset
            assert call(ctypes.byref(plan), ptrs, base + 2, None, sd, 3 * 2304, *table) == 4  # SKR_ERR_ALIGN, ahead of the sample size
            plan = make_plan(n=2, sample_numel=0, noise_mode=noise_mode)  # a ragged numel and no usable sample size
            assert call(ctypes.byref(plan), ptrs, base, None, sd, 3 * 2304, *table) == (5 if per_sample or noise_mode else 7), name
