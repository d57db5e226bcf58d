"""The row forms of adaptive projected guidance without a device: the four entries in the header, in EXPORTS and in the built library and
outside the launch table, the argument checks of one statistic entry and one step entry in their documented order, and the keyword
refusals of capture_sampling_loop."""

import ctypes
import os

import pytest
import torch
from test_projected_guidance_host import ALIGN, DTYPE, NULL, OK, SHAPE, TERMS, UNSUPPORTED, aligned_buffer, wrapper

from skrample_amd import _hip, graphs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [stem + form for stem in ("skr_projected_guidance_coef", "skr_projected_guided_step_launch") for form in ("_indexed", "_indexed_per_sample")]


def test_entries_are_declared_exported_built_and_outside_the_table():
    header, lib = open(os.path.join(ROOT, "include", "skrample_hip.h")).read(), _hip.load()
    for name in NAMES:
        assert f"int {name}(" in header and name in _hip.EXPORTS and getattr(lib, name) is not None
        assert all(name != entry for entry, _ in _hip.ENTRIES.values())
    assert len(_hip.ENTRIES) == 22


COEF_CASES = [  # (changed arguments, code): each case also breaks something checked later, so the order shows
    ({"mom": None, "numel": -1}, NULL), ({"rows": None, "sn": 0}, NULL), ({"index": None, "sn": 0}, NULL), ({"partials": None, "sn": 0}, NULL),
    ({"numel": -2048, "cond": 8}, SHAPE), ({"sn": 1}, SHAPE), ({"numel": 4095}, SHAPE),
    ({"numel": 0, "cond": 8, "dtype": 99}, OK),
    ({"cond": 8, "dtype": 99}, ALIGN), ({"mom": 8, "dtype": 99}, ALIGN), ({"coef": 2, "dtype": 99}, ALIGN),
    ({"dtype": 99, "sn": 8, "numel": 16}, DTYPE),
    ({"dtype": _hip.F64}, UNSUPPORTED), ({"sn": 2056, "numel": 4112}, UNSUPPORTED), ({"row_offset": -1}, UNSUPPORTED),
]  # fmt: skip


@pytest.mark.parametrize("changes,code", COEF_CASES)
def test_coef_row_entry_checks_in_their_documented_order(changes, code):
    "a pointer given as an int is the aligned buffer plus that offset; None is NULL; no launch is reached, so no memory is touched"
    _, good = aligned_buffer()
    a = {"uncond": 0, "cond": 0, "mom": 0, "dtype": _hip.BF16, "numel": 4096, "sn": 2048, "rows": 0, "index": 0, "row_offset": 1, "coef": 0, "partials": 0, **changes}
    ptr = lambda k: None if a[k] is None else good + a[k]  # noqa: E731
    status = _hip.load().skr_projected_guidance_coef_indexed_per_sample(ptr("uncond"), ptr("cond"), ptr("mom"), a["dtype"], a["numel"], a["sn"], ptr("rows"), ptr("index"),
                                                                        a["row_offset"], ptr("coef"), None, ptr("partials"), None)  # fmt: skip
    assert status == code


STEP_CASES = [  # (changed fields: the plan's, proj_..., guide_..., or the call's, code)
    ({"rows": None, "n_terms": 99}, NULL), ({"proj": None, "n_terms": 99}, NULL), ({"noise_mode": 1, "n_terms": 99}, NULL),
    ({"n_terms": 17, "numel": -1}, TERMS), ({"guide_slot": 2, "numel": -1}, TERMS),
    ({"numel": -1, "noise_mode": 3}, SHAPE),
    ({"noise_mode": 3, "proj_sample_numel": 0}, UNSUPPORTED), ({"proj_reserved": 1, "proj_sample_numel": 0}, UNSUPPORTED), ({"acc_f64": 1, "proj_sample_numel": 0}, UNSUPPORTED),
    ({"out0_dtype": _hip.NONE, "proj_sample_numel": 0}, UNSUPPORTED),
    ({"proj_sample_numel": 5, "guide_cond": None}, SHAPE),
    ({"numel": 0, "inputs": None, "out": None, "guide_cond": None}, OK),
    ({"guide_cond": None, "out": 8}, NULL), ({"proj_diff": None, "out": 8}, NULL), ({"inputs": None}, NULL),
    ({"proj_diff": 8, "dtype_a": 99}, ALIGN), ({"proj_coef_dev": 2, "dtype_a": 99}, ALIGN),
    ({"dtype_a": _hip.F64, "dtype_b": _hip.F64, "out0_dtype": _hip.F64}, DTYPE), ({"dtype_a": 99, "row_offset": -1}, DTYPE),
    ({"row_offset": -1}, UNSUPPORTED), ({"proj_sample_numel": 8, "numel": 16}, UNSUPPORTED),
]  # fmt: skip


@pytest.mark.parametrize("changes,code", STEP_CASES)
def test_step_row_entry_checks_in_their_documented_order(changes, code):
    _, good = aligned_buffer()
    at = lambda v: None if v is None else good + v  # noqa: E731
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = 2
    plan.dtype_a = plan.dtype_b = plan.out0_dtype = _hip.BF16
    plan.out1_dtype = _hip.NONE
    proj, guide = _hip.StepProjectionC(good, good, 2048, 0), _hip.StepGuidanceC(good, good, 0.0, 0, 0)
    call = {"numel": 4096, "out": 0, "inputs": (ctypes.c_void_p * 2)(good, good), "proj": proj, "rows": 0, "row_offset": 1}
    for k, v in changes.items():
        if k in call:
            call[k] = v
        elif k.startswith(("proj_", "guide_")):
            target, field = (proj, k[5:]) if k.startswith("proj_") else (guide, k[6:])
            setattr(target, field, at(v) if field in ("coef_dev", "diff", "cond", "guided_out") else v)
        else:
            setattr(plan, k, v)
    status = _hip.load().skr_projected_guided_step_launch_indexed(ctypes.byref(plan), call["inputs"], at(call["out"]), ctypes.byref(guide),
                                                                  ctypes.byref(proj) if call["proj"] is not None else None, None, call["numel"], at(call["rows"]), None,
                                                                  call["row_offset"], None)  # fmt: skip
    assert status == code


def test_capture_keyword_refusals():
    x, model = torch.zeros(2, 4, 32, 16), lambda s, t: (s, s)
    w = wrapper(eta=0.0, norm_threshold=2.0, momentum=-0.5)
    with pytest.raises(ValueError, match="guidance_scale"):
        graphs.capture_sampling_loop(w, model, x, 4, projected=True)
    for beside in ({"rescaled": True, "indexed": True}, {"thresholded": True}, {"guidance_rescale": 0.5}):
        with pytest.raises(ValueError, match="projected=True stands beside neither"):
            graphs.capture_sampling_loop(w, model, x, 4, guidance_scale=5.0, projected=True, **beside)
    with pytest.raises(ValueError, match="set_projected_guidance"):
        graphs.capture_sampling_loop(wrapper(), model, x, 4, guidance_scale=5.0, projected=True)
    with pytest.raises(_hip.SkrampleHipError, match="no row form.*projected=True"):
        graphs.capture_sampling_loop(w, model, x, 4, guidance_scale=5.0)
