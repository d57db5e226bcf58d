"""Projected guidance in rolling batches without a GPU: the two entries in the header, in EXPORTS and in the built library and outside the
launch table; the keyword and its refusals; and the rows `RollingBatch(..., guided=True, projected=True)` writes at admit(), on a stub dry run
(as in tests/test_thresholding_rolling_host.py: nothing here enqueues device work)."""

import inspect
import os

import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.pytorch import noise as generators
from skrample_amd.rolling import RollingBatch
from skrample_amd.sampling import structured as PT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROLES, UNIT = [("x",), ("o",), ("po", -1)], (4, 32, 16)


class StubBatch(RollingBatch):
    "the dry run gives a DPM-2-like ramp-up (2, 3, 3, ... operands) with coef0[j] = 10 (i + 1) (j + 1)"

    def _trace(self, wrapper, steps, seed):
        traced = []
        for i in range(steps):
            plan, roles = _hip.StepPlanC(), ROLES[: min(i + 2, 3)]
            plan.n_terms = plan.n_group_a = len(roles)
            plan.dtype_a = plan.dtype_b = plan.out0_dtype = _hip.BF16
            plan.out1_dtype, plan.stream1 = _hip.NONE, 77  # (whatever a traced plan holds there: the row's stream1 is the batch's to write)
            for j in range(len(roles)):
                plan.coef0[j] = 10.0 * (i + 1) * (j + 1)
            traced.append((plan, roles, 100.0 - i))
        return traced


def wrapper(setting=(0.0, 10.0, -0.5), sampler=None, **fields):
    w = PD.SkrampleWrapperScheduler(sampler if sampler is not None else PT.DPM(order=2), PS.Scaled(), **fields)
    if setting is not None:
        w.set_projected_guidance(*setting)
    return w


example = lambda capacity=3, unit=UNIT, dtype=torch.bfloat16: torch.zeros(capacity, *unit, dtype=dtype)  # noqa: E731


def test_names_and_signatures():
    header, lib = open(os.path.join(ROOT, "include", "skrample_hip.h")).read(), _hip.load()
    for name in _hip.PROJECTED_ROLLING:
        assert f"int {name}(" in header and name in _hip.EXPORTS and getattr(lib, name) is not None
        assert all(name != entry for entry, _ in _hip.ENTRIES.values())
    assert _hip.PROJECTED_ROLLING == ("skr_projected_guidance_coef_rolling", "skr_projected_guided_step_launch_rolling") and len(_hip.ENTRIES) == 22
    built = inspect.signature(RollingBatch.__init__).parameters
    assert list(built)[-2:] == ["thresholded", "projected"] and built["projected"].default is False
    assert list(inspect.signature(RollingBatch.step_guided).parameters) == ["self", "uncond", "cond"]


REFUSED = {  # (make_wrapper, keywords, what the refusal names)
    "unguided": (wrapper, dict(guided=False), "projected=True needs guided=True"),
    "rescaled": (wrapper, dict(rescaled=True), "projected together with rescaled"),
    "thresholded": (wrapper, dict(thresholded=True), "projected together with thresholded"),
    "inpaint": (wrapper, dict(inpaint_mask_shape=(1, 32, 16)), "projected together with inpaint_mask_shape"),
    "ragged": (wrapper, dict(unit=(4, 18, 32)), "projected together with ragged samples"),
    "plain_wrapper": (lambda: wrapper(None), {}, "set_projected_guidance"),
    "UniPC": (lambda: wrapper(sampler=PT.UniPC(order=2)), {}, "projected step of UniPC"),
    "SPC": (lambda: wrapper(sampler=PT.SPC()), {}, "projected step of SPC"),
    "compute_scale": (lambda: wrapper(compute_scale=None), {}, "compute_scale=None"),
    "fp64": (wrapper, dict(dtype=torch.float64), "fp64"),
    "offset": (lambda: wrapper(sampler=PT.DPM(order=2, stochasticity=1.0), noise_type=generators.Offset), {}, "projected together with Offset noise"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_refused_by_name_when_the_batch_is_built(case):
    make, options, says = REFUSED[case]
    options = {"guided": True, **options}
    given = example(2, options.pop("unit", UNIT), options.pop("dtype", torch.bfloat16))
    with pytest.raises((_hip.SkrampleHipError, ValueError), match=says):
        RollingBatch(make, given, capacity=2, projected=True, **options)


@pytest.mark.parametrize("beta", [-0.5, 0.0, -0.0])
def test_rows_carry_the_setting_and_the_first_momentum_row_starts_the_average(beta):
    batch = StubBatch(wrapper, example(), capacity=3, guided=True, projected=True)
    assert batch.slot == 1 and batch.momentum_buf.shape == (3, *UNIT) and batch.momentum_buf.dtype == torch.bfloat16
    assert (batch.coef.shape, batch.coef.dtype) == ((6,), torch.float32) and batch._projected_partials.numel() == _hip.projected_partials(batch.numel, batch.sample_numel)
    batch.admit(1, example()[0], wrapper((0.5, 30.0, beta)), 3, guidance_scale=[3.0, 4.0, 5.0])
    for i, row in enumerate(batch._requests[1].rows):
        assert list(row.convert_k) == [3.0 + i, 0.5, 30.0, beta] and row.stream1 == (1 if i == 0 and beta != 0.0 else 0)
        assert list(row.coef0)[:3] == [10.0 * (i + 1), 20.0 * (i + 1), 30.0 * (i + 1) if i else 0.0] and not any(row.coef1)


def test_admit_refuses_the_wrapper_that_does_not_match_the_batch():
    batch = StubBatch(wrapper, example(), capacity=3, guided=True, projected=True)
    with pytest.raises(ValueError, match="set_projected_guidance"):
        batch.admit(0, example()[0], wrapper(None), 3, guidance_scale=7.5)
    plain = StubBatch(lambda: wrapper(None), example(), capacity=3, guided=True)
    with pytest.raises(_hip.SkrampleHipError, match="no row form.*projected=True"):
        plain.admit(0, example()[0], wrapper(), 3, guidance_scale=7.5)
    assert batch.free(0) and plain.free(0) and not batch.rows_dev.any()
