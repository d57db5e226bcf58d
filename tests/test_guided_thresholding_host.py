"""Guided dynamic thresholding without a device: both entries in the header, in EXPORTS and in the built library, their argument checks
in the documented order, and host-resident tensors under set_thresholding(..., fuse_guidance=True) against the default wrapper."""

import ctypes
import os

import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.sampling import structured as PT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NULL, DTYPE, TERMS, ALIGN, SHAPE, LAUNCH, UNSUPPORTED = range(8)
NAMES = ("skr_guided_threshold_scale", "skr_guided_thresholded_step_launch")


def test_entries_are_declared_exported_and_built():
    header = open(os.path.join(ROOT, "include", "skrample_hip.h")).read()
    lib = _hip.load()
    for name in NAMES:
        assert f"int {name}(" in header and name in _hip.EXPORTS and getattr(lib, name) is not None
    assert _hip.ABI_VERSION == 15 and lib.skr_abi_version() == 15 and len(_hip.ENTRIES) == 22


def aligned_buffer():
    buf = (ctypes.c_char * 128)()
    return buf, ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16


SCALE_CASES = [  # (changed arguments, code): each case also breaks something checked later, so the order shows
    ({"sample": None, "numel": -1}, NULL), ({"cond": None, "sn": 0}, NULL), ({"uncond": None}, NULL), ({"ws": None, "sn": 0}, NULL),
    ({"numel": -8, "cond": 8}, SHAPE), ({"sn": 0}, SHAPE), ({"numel": 12}, SHAPE),
    ({"numel": 0, "cond": 8, "dtype": 99, "ratio": 2.0}, OK),
    ({"cond": 8, "dtype": 99}, ALIGN), ({"uncond": 8, "dtype": 99}, ALIGN), ({"scale": 2, "dtype": 99}, ALIGN),
    ({"dtype": _hip.F64, "ratio": 0.0}, DTYPE), ({"dtype": 99}, DTYPE),
    ({"ratio": 0.0}, UNSUPPORTED), ({"ratio": 1.0001}, UNSUPPORTED), ({"ratio": float("nan")}, UNSUPPORTED),
]  # fmt: skip


@pytest.mark.parametrize("changes,code", SCALE_CASES)
def test_scale_entry_checks_in_their_documented_order(changes, code):
    "a pointer given as an int is the aligned buffer plus that offset; None is NULL; no launch is reached, so no memory is touched"
    _, good = aligned_buffer()
    a = {"sample": 0, "uncond": 0, "cond": 0, "dtype": _hip.BF16, "ratio": 0.995, "numel": 16, "sn": 8, "scale": 0, "ws": 0, **changes}
    ptr = lambda k: None if a[k] is None else good + a[k]  # noqa: E731
    status = _hip.load().skr_guided_threshold_scale(ptr("sample"), ptr("uncond"), ptr("cond"), a["dtype"], 7.3, 1.0, -1.0, a["ratio"], 1.5, a["numel"], a["sn"],
                                                    ptr("scale"), ptr("ws"), None)  # fmt: skip
    assert status == code


STEP_CASES = [  # (changed fields: plan's, thr_..., guide_..., or the call's numel / out / inputs, code)
    ({"guide": None}, NULL), ({"noise_mode": 1, "zeta0": 0.5, "n_terms": 99}, NULL),
    ({"n_terms": 17, "numel": -1}, TERMS), ({"thr_xslot": 0, "numel": -1}, TERMS), ({"guide_slot": 1, "numel": -1}, TERMS),
    ({"numel": -1, "noise_mode": 3}, SHAPE),
    ({"out0_dtype": _hip.NONE, "thr_x0_out": None, "noise_mode": 3}, NULL),
    ({"noise_mode": 3, "thr_sample_numel": 0}, UNSUPPORTED), ({"thr_reserved": 1, "thr_sample_numel": 0}, UNSUPPORTED),
    ({"guide_reserved": 1, "thr_sample_numel": 0}, UNSUPPORTED), ({"guide_guided_out": 0, "thr_sample_numel": 0}, UNSUPPORTED),
    ({"acc_f64": 1, "thr_sample_numel": 0}, UNSUPPORTED), ({"out0_dtype": _hip.NONE, "thr_sample_numel": 0}, UNSUPPORTED),
    ({"thr_sample_numel": 5, "guide_cond": None}, SHAPE),
    ({"numel": 0, "inputs": None, "out": None, "guide_cond": None}, OK),
    ({"guide_cond": None, "out": 8}, NULL), ({"inputs": None}, NULL),
    ({"guide_cond": 8, "dtype_a": 99}, ALIGN), ({"thr_x0_out": 8}, ALIGN), ({"thr_scale_dev": 2}, ALIGN),
    ({"dtype_a": _hip.F64, "dtype_b": _hip.F64, "out0_dtype": _hip.F64}, UNSUPPORTED), ({"dtype_a": 99}, DTYPE),
]  # fmt: skip


@pytest.mark.parametrize("changes,code", STEP_CASES)
def test_step_entry_checks_in_their_documented_order(changes, code):
    _, good = aligned_buffer()
    at = lambda v: None if v is None else good + v  # noqa: E731
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = 2
    plan.dtype_a = plan.dtype_b = plan.out0_dtype = _hip.BF16
    plan.out1_dtype = _hip.NONE
    thr = _hip.StepThresholdC(None, good, 1.0, -1.0, 8, 0, 1, 0)
    guide = _hip.StepGuidanceC(good, None, 7.3, 0, 0)
    call = {"numel": 16, "out": 0, "inputs": (ctypes.c_void_p * 2)(good, good), "guide": guide}
    for k, v in changes.items():
        if k in call:
            call[k] = v
        elif k.startswith(("thr_", "guide_")):
            target, field = (thr, k[4:]) if k.startswith("thr_") else (guide, k[6:])
            setattr(target, field, at(v) if field in ("x0_out", "scale_dev", "cond", "guided_out") else v)
        else:
            setattr(plan, k, v)
    status = _hip.load().skr_guided_thresholded_step_launch(ctypes.byref(plan), call["inputs"], at(call["out"]), ctypes.byref(guide) if call["guide"] is not None else None,
                                                            ctypes.byref(thr), None, call["numel"], None)  # fmt: skip
    assert status == code


@pytest.mark.parametrize("sampler", [PT.Euler(), PT.DPM(order=2), PT.UniPC(order=2)], ids=lambda s: type(s).__name__)
def test_host_tensors_under_fuse_guidance_have_the_default_wrappers_bits(sampler):
    steps, shape = 3, (2, 3, 8, 8)
    g = torch.Generator().manual_seed(3)
    x0, halves = torch.randn(shape, generator=g), [torch.randn((2, *shape), generator=g) for _ in range(steps)]
    runs = []
    for fuse in (True, False):
        w = PD.SkrampleWrapperScheduler(sampler, PS.Karras(PS.Scaled()))
        w.set_thresholding(0.9, 1.5, fuse_guidance=True) if fuse else w.set_thresholding(0.9, 1.5)
        w.set_timesteps(steps)
        x, got = x0 * float(w.init_noise_sigma), []
        for t, (u, c) in zip(w.timesteps, halves):
            x, p = w.step_guided(u, c, 5.0, t, x, return_dict=False)
            got += [x, p.materialize() if hasattr(p, "materialize") else p]
        runs.append(got)
    assert all(torch.equal(a, b) for a, b in zip(*runs))
