"""Dynamic thresholding in rolling batches without a GPU: the bookkeeping of `RollingBatch(..., thresholded=True)` on stub rows and a stub
library (the dry run and the library are replaced, as in tests/test_guided_rolling_host.py: nothing here enqueues device work)."""

import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.rolling import RollingBatch
from skrample_amd.sampling import structured as PT

HISTORY = [("x",), ("o",), ("po", -1), ("po", -2)]
UNIT = (4, 32, 32)


def stub_plan(roles, scale, a, b, ratio, max_value):
    "coef0[j] = scale * (j + 1), and the step's thresholding values where a traced plan carries them"
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = len(roles)
    plan.dtype_a = plan.dtype_b = plan.out0_dtype = _hip.BF16
    plan.out1_dtype = _hip.NONE
    for j in range(len(roles)):
        plan.coef0[j] = scale * (j + 1)
    plan.convert_k[0], plan.convert_k[1], plan.convert_k[2], plan.convert_k[3] = a, b, ratio, max_value
    return plan


class Lib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def launch(*args):
            self.calls.append((name, args))
            return 0

        return launch


class StubBatch(RollingBatch):
    "the dry run gives an Adams-3-like ramp-up (2, 3, 4, 4, ... operands) with a = 1 / (i + 1) and b = -i; the wrapper's setting is its own"

    def _trace(self, wrapper, steps, seed):
        ratio, max_value = wrapper._thresholding_next
        return [(stub_plan(HISTORY[: min(i + 2, 4)], 10.0 * (i + 1), 1.0 / (i + 1), -float(i), ratio, max_value), HISTORY[: min(i + 2, 4)], 100.0 - i) for i in range(steps)]


def wrapper(setting=(0.995, 1.5)):
    w = PD.SkrampleWrapperScheduler(PT.Adams(order=3), PS.Scaled())
    if setting is not None:
        w.set_thresholding(*setting)
    return w


@pytest.fixture
def lib(monkeypatch):
    stub = Lib()
    monkeypatch.setattr(_hip, "load", lambda: stub)
    monkeypatch.setattr(_hip, "current_stream_ptr", lambda device: 0)
    return stub


def make_batch(capacity=4):
    return StubBatch(wrapper, torch.zeros(capacity, *UNIT, dtype=torch.bfloat16), capacity=capacity, thresholded=True)


@pytest.mark.parametrize("setting", [(0.995, 1.5), (0.5, 1.0)], ids=["select", "plain_clip"])
def test_rows_carry_what_a_captured_loop_records_for_the_same_launches(setting):
    batch = make_batch()
    assert (batch.slot, batch.xslot, batch.keep) == (1, 0, 2) and not any(batch.plan.convert_k)
    assert batch.scale.shape == (4,) and batch.scale.dtype == torch.float32 and batch._threshold_ws.numel() == _hip.threshold_workspace(batch.numel, batch.sample_numel)
    batch.admit(1, torch.zeros(UNIT, dtype=torch.bfloat16), wrapper(setting), 4)
    recorder = _hip.IndexedRows(torch.device("cpu"), samples=1, thresholded=True)
    for i, row in enumerate(batch._requests[1].rows):
        plan = stub_plan(HISTORY[: min(i + 2, 4)], 10.0 * (i + 1), 1.0 / (i + 1), -float(i), *setting)
        want = recorder.row_from(plan)  # (IndexedRows.launch_thresholded writes thr.a, thr.b, ratio, maximum over convert_k[0..3]: the plan's here)
        assert list(row.convert_k) == list(want.convert_k) == [1.0 / (i + 1), -float(i), *setting]
        assert list(row.coef0) == list(want.coef0) and not any(row.coef1)


def test_a_tick_is_the_statistic_then_the_step_on_the_same_table_and_the_ring_rotates(lib):
    batch = make_batch()
    batch.admit(0, torch.zeros(UNIT, dtype=torch.bfloat16), wrapper(), 6)
    own, stores = {t.data_ptr() for t in batch._p}, []
    assert len(batch._p) == len(batch._x) == batch.keep + 2 and all(any(t is r for r in batch.ring_tensors()) for t in batch._p)
    for tick in range(6):
        out, latents = torch.zeros(4, *UNIT, dtype=torch.bfloat16), batch.latents
        assert batch.step(out) == ([0] if tick == 5 else [])
        (first, stat), (second, step) = lib.calls[-2:]
        assert (first, second) == _hip.THRESHOLD_ROLLING and len(stat) == 11 and len(step) == 10
        assert stat[:5] == (latents.data_ptr(), out.data_ptr(), _hip.BF16, batch.numel, batch.sample_numel)
        table = (batch.rows_dev.data_ptr(), batch.index_dev.data_ptr(), 0)
        assert stat[5:8] == step[6:9] == table and stat[8:10] == (batch.scale.data_ptr(), batch._threshold_ws.data_ptr())
        thr, ptrs = step[3]._obj, list(step[1])
        assert (thr.scale_dev, thr.slot, thr.xslot, thr.sample_numel, thr.reserved) == (batch.scale.data_ptr(), 1, 0, batch.sample_numel, 0)
        assert ptrs[:2] == [latents.data_ptr(), out.data_ptr()] and step[2] == batch.latents.data_ptr() and step[5] == batch.numel
        assert thr.x0_out in own and thr.x0_out not in ptrs  # the entry no operand reads
        stores.append(thr.x0_out)
        assert tick < 1 or ptrs[2] == stores[tick - 1]  # ("po", -1): what the last tick stored
        assert tick < 2 or ptrs[3] == stores[tick - 2]
    assert stores[4] == stores[0] and len(set(stores[:4])) == 4  # a ring of keep + 2
    assert batch._outputs == [] and batch._stamps == [] and batch.index_dev.tolist() == [5, -1, -1, -1]


def test_a_wrapper_without_thresholding_is_refused_by_name_and_leaves_no_trace(lib):
    batch = make_batch()
    with pytest.raises(ValueError, match="set_thresholding"):
        batch.admit(0, torch.zeros(UNIT, dtype=torch.bfloat16), wrapper(None), 3)
    assert batch.free(0) and not batch.rows_dev.any() and lib.calls == []
    with pytest.raises(ValueError, match="set_thresholding"):
        StubBatch(lambda: wrapper(None), torch.zeros(2, *UNIT, dtype=torch.bfloat16), capacity=2, thresholded=True)
