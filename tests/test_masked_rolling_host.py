"""In-painting in rolling batches without a GPU: the new export at the C boundary, and the bookkeeping of a masked
`skrample_amd.rolling.RollingBatch` on stub rows (the dry run and the launch are replaced, as in tests/test_rolling_host.py: nothing
here enqueues device work)."""

import ctypes
import os
import re

import pytest
import torch
from conftest import ROOT

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.rolling import RollingBatch
from skrample_amd.sampling import structured as PT

NAME = "skr_step_launch_masked_rolling"
HISTORY = [("x",), ("o",), ("po", -1), ("po", -2)]
UNIT, MASK = (4, 32, 32), (1, 32, 32)


def test_export_is_declared_listed_and_built():
    header = open(os.path.join(ROOT, "include", "skrample_hip.h")).read()
    assert re.search(r"^int " + NAME + r"\(", header, flags=re.M)
    assert "There is no rolling form" not in header
    assert NAME in _hip.EXPORTS
    lib = _hip.load()
    assert hasattr(lib, NAME) and lib.skr_step_launch_masked_rolling.argtypes == lib.skr_step_launch_masked_indexed_per_sample.argtypes
    assert lib.skr_abi_version() == _hip.ABI_VERSION  # purely additive


def test_argument_validation_without_gpu():
    "the NULL tests come first and dereference nothing"
    lib = _hip.load()
    plan, desc = _hip.StepPlanC(), _hip.StepMaskC()
    rows = (_hip.StepRowC * 1)()
    index = (ctypes.c_int32 * 2)()
    for entry in (lib.skr_step_launch_masked_rolling, lib.skr_step_launch_masked_indexed_per_sample):
        assert entry(ctypes.byref(plan), None, None, ctypes.byref(desc), None, 4096, None, ctypes.addressof(index), 0, None) == 1  # SKR_ERR_NULL: no rows
        assert entry(ctypes.byref(plan), None, None, ctypes.byref(desc), None, 4096, ctypes.addressof(rows), None, 0, None) == 1  # no index
        assert entry(ctypes.byref(plan), None, None, None, None, 4096, ctypes.addressof(rows), ctypes.addressof(index), 0, None) == 1  # no mask descriptor
        assert entry(None, None, None, ctypes.byref(desc), None, 4096, ctypes.addressof(rows), ctypes.addressof(index), 0, None) == 1  # no plan


# ---- a masked RollingBatch on stub rows ----------------------------------------------------------------------------------------------
def stub_plan(roles, scale, known):
    "coef0[j] = scale * (j + 1) for the step's own operands (zero for orig / znoise); coef1 = `known`: {role: value}"
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = len(roles)
    plan.dtype_a = plan.dtype_b = plan.out0_dtype = _hip.BF16
    plan.out1_dtype = _hip.NONE
    for j, role in enumerate(roles):
        plan.coef0[j] = 0.0 if role[0] in ("orig", "znoise") else scale * (j + 1)
        plan.coef1[j] = known.get(role, 0.0)
    return plan


class StubBatch(RollingBatch):
    """the dry run gives an Adams-3-like ramp-up (2, 3, 4, 4, ... operands of the step itself); a wrapper with set_inpaint in force adds
    the original and the re-noising tensor behind them (the last step: the original alone); launches are recorded, not made"""

    def __init__(self, *args, **kwargs):
        self.launched, self.traces = [], 0
        super().__init__(*args, **kwargs)

    def _trace(self, wrapper, steps, seed):
        self.traces += 1
        masked = getattr(wrapper, "_inpaint", None) is not None
        found = []
        for i in range(steps):
            roles, known = HISTORY[: min(i + 2, 4)], {}
            if masked:
                last = i == steps - 1
                roles = roles + ([("orig",)] if last else [("orig",), ("znoise",)])
                known = {("orig",): 1.0} if last else {("orig",): 0.5 + i, ("znoise",): 0.25 + i}
            found.append((stub_plan(roles, 10.0 * (i + 1), known), roles, 100.0 - i))
        return found

    def _launch(self, arr, out0, out1):
        self.launched.append((list(arr), out0, out1))


def wrapper():
    return PD.SkrampleWrapperScheduler(PT.Adams(order=3), PS.Scaled())


def masked_batch(capacity=4, **options):
    return StubBatch(wrapper, torch.zeros(capacity, *UNIT, dtype=torch.bfloat16), capacity=capacity, inpaint_mask_shape=MASK, **options)


def inpaint_of(seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(MASK, generator=g).bfloat16(), torch.randn(UNIT, generator=g).bfloat16(), torch.randn(UNIT, generator=g).bfloat16()


def test_orig_and_znoise_get_slots_behind_the_history():
    batch = masked_batch()
    assert batch.masked and batch.roles == HISTORY + [("orig",), ("znoise",)] and batch.plan.n_terms == 6
    assert tuple(batch.mask.shape) == (4, *MASK) and bool((batch.mask == 1).all()) and batch.mask.dtype == torch.bfloat16
    assert tuple(batch.original.shape) == tuple(batch.noise.shape) == (4, *UNIT)
    desc = batch._mask_desc
    assert (desc.mask, desc.dtype, desc.mask_numel, desc.batch_stride) == (batch.mask.data_ptr(), _hip.BF16, 1024, 1024)  # always one mask per slot
    out = torch.zeros(4, *UNIT, dtype=torch.bfloat16)
    assert batch._bind(("orig",), out) is batch.original and batch._bind(("znoise",), out) is batch.noise


def test_rows_of_an_inpainting_request():
    batch = masked_batch()
    x = torch.zeros(UNIT, dtype=torch.bfloat16)
    mask, original, noise = inpaint_of()
    w = wrapper()
    batch.admit(2, x, w, 5, inpaint=(mask, original, noise))
    assert torch.equal(batch.mask[2], mask) and torch.equal(batch.original[2], original) and torch.equal(batch.noise[2], noise)
    assert bool((batch.mask[[0, 1, 3]] == 1).all()) and not batch.original[[0, 1, 3]].any()
    held = w._inpaint  # one-sample views of the batch's own tensors: the dry run steps on them
    assert [t.data_ptr() for t in held] == [batch.mask[2:3].data_ptr(), batch.original[2:3].data_ptr(), batch.noise[2:3].data_ptr()]
    rows = batch._requests[2].rows
    at_orig, at_noise = batch.roles.index(("orig",)), batch.roles.index(("znoise",))
    # operand order is preserved: the step's own operands keep their slots and values, the ramp-up's missing history is zero in both forms
    assert [list(r.coef0)[:6] for r in rows[:3]] == [[10.0, 20.0, 0.0, 0.0, 0.0, 0.0], [20.0, 40.0, 60.0, 0.0, 0.0, 0.0], [30.0, 60.0, 90.0, 120.0, 0.0, 0.0]]
    assert [(r.coef1[at_orig], r.coef1[at_noise]) for r in rows] == [(0.5, 0.25), (1.5, 1.25), (2.5, 2.25), (3.5, 3.25), (1.0, 0.0)]
    last = rows[-1]  # the known form of the last step is the original alone: an exact zero in the znoise slot, in both forms
    assert bytes(ctypes.c_double(last.coef0[at_noise])) == bytes(ctypes.c_double(last.coef1[at_noise])) == bytes(8)
    assert all(r.coef1[k] == 0.0 for r in rows for k in range(4)) and not any(list(last.coef0)[6:]) and not any(list(last.coef1)[6:])
    stored = bytes(batch.rows_dev[2 * batch.max_steps * batch.row_bytes :][: 5 * batch.row_bytes].numpy())
    assert stored == b"".join(bytes(r) for r in rows)


def test_a_plain_request_shares_the_batch():
    batch = masked_batch()
    x = torch.zeros(UNIT, dtype=torch.bfloat16)
    batch.admit(1, x, wrapper(), 4, inpaint=inpaint_of(1))
    batch.mask[3].fill_(0.25)  # what an earlier occupant left
    batch.admit(3, x, wrapper(), 4)
    assert bool((batch.mask[3] == 1).all())
    at_orig, at_noise = batch.roles.index(("orig",)), batch.roles.index(("znoise",))
    for r in batch._requests[3].rows:
        assert not any(r.coef1) and r.coef0[at_orig] == r.coef0[at_noise] == 0.0  # orig / znoise absent, nothing in the known form
    assert [list(r.coef0)[:4] for r in batch._requests[3].rows[:2]] == [[10.0, 20.0, 0.0, 0.0], [20.0, 40.0, 60.0, 0.0]]
    out = torch.zeros(4, *UNIT, dtype=torch.bfloat16)
    assert batch.step(out) == [] and len(batch.launched) == 1
    ptrs, out0, out1 = batch.launched[0]
    assert ptrs[4:] == [batch.original.data_ptr(), batch.noise.data_ptr()] and out0 is batch.latents and out1 is None
    assert batch.index_dev.tolist() == [-1, 128, -1, 384]


def test_admit_refusals_come_before_anything_is_uploaded():
    plain = StubBatch(wrapper, torch.zeros(4, *UNIT, dtype=torch.bfloat16), capacity=4)
    batch = masked_batch()
    x = torch.zeros(UNIT, dtype=torch.bfloat16)
    mask, original, noise = inpaint_of(2)
    traces = (plain.traces, batch.traces)
    with pytest.raises(ValueError, match="inpaint_mask_shape"):
        plain.admit(0, x, wrapper(), 4, inpaint=(mask, original, noise))
    with pytest.raises(ValueError, match="three tensors"):
        batch.admit(0, x, wrapper(), 4, inpaint=(mask, original))
    with pytest.raises(ValueError, match="a mask of shape"):
        batch.admit(0, x, wrapper(), 4, inpaint=(mask[0], original, noise))
    with pytest.raises(ValueError, match="a mask of shape"):
        batch.admit(0, x, wrapper(), 4, inpaint=(mask.expand(4, 32, 32), original, noise))
    with pytest.raises(ValueError, match="original_samples of shape"):
        batch.admit(0, x, wrapper(), 4, inpaint=(mask, original.float(), noise))
    with pytest.raises(ValueError, match="noise of shape"):
        batch.admit(0, x, wrapper(), 4, inpaint=(mask, original, noise[:2]))
    held = wrapper()
    held.set_inpaint(mask.unsqueeze(0), original.unsqueeze(0), noise.unsqueeze(0))
    with pytest.raises(ValueError, match="set_inpaint in force"):
        batch.admit(0, x, held, 4)
    assert (plain.traces, batch.traces) == traces and not batch.rows_dev.any() and not plain.rows_dev.any()
    assert bool((batch.mask == 1).all()) and not batch.original.any() and not batch.noise.any() and batch.free(0) and plain.free(0)
    batch.admit(0, x, wrapper(), 4, inpaint=(mask.unsqueeze(0) > 0.5, original.unsqueeze(0), noise.unsqueeze(0)))  # a leading 1, a bool mask
    assert torch.equal(batch.mask[0], (mask > 0.5).bfloat16())
    with pytest.raises(ValueError, match="multiple of 8"):
        StubBatch(wrapper, torch.zeros(2, 2048, 1, 4, dtype=torch.bfloat16), capacity=2, inpaint_mask_shape=(1, 4))
    with pytest.raises(ValueError, match="not the mask of one"):
        StubBatch(wrapper, torch.zeros(4, *UNIT, dtype=torch.bfloat16), capacity=4, inpaint_mask_shape=(1, 16, 32))


def test_a_batch_without_a_mask_shape_is_what_it_was(monkeypatch):
    plain = StubBatch(wrapper, torch.zeros(4, *UNIT, dtype=torch.bfloat16), capacity=4)
    assert plain.masked is False and plain.roles == HISTORY
    assert not any(hasattr(plain, name) for name in ("mask", "original", "noise", "mask_shape", "mask_numel", "_mask_desc"))
    calls = []

    class Lib:
        def skr_step_launch_rolling(self, *args):
            calls.append(("skr_step_launch_rolling", args))
            return 0

        def skr_step_launch_masked_rolling(self, *args):
            calls.append(("skr_step_launch_masked_rolling", args))
            return 0

    monkeypatch.setattr(_hip, "load", lambda: Lib())
    monkeypatch.setattr(_hip, "current_stream_ptr", lambda device: 0)
    out = torch.zeros(4, *UNIT, dtype=torch.bfloat16)
    arr = (ctypes.c_void_p * 1)(out.data_ptr())
    RollingBatch._launch(plain, arr, out, None)
    assert [name for name, _ in calls] == ["skr_step_launch_rolling"] and len(calls[0][1]) == 10
    masked = masked_batch()
    RollingBatch._launch(masked, arr, out, None)
    name, args = calls[1]
    assert name == "skr_step_launch_masked_rolling" and len(args) == 10
    assert args[2] == out.data_ptr() and args[5] == masked.numel and args[6] == masked.rows_dev.data_ptr() and args[7] == masked.index_dev.data_ptr() and args[8] == 0
