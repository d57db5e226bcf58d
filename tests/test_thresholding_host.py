"""Dynamic thresholding without a device: the argument checks of skr_threshold_scale and skr_thresholded_step_launch through the built
library, the struct's layout against the header, set_thresholding's validation, and the host-executor route against a float64 loop."""

import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.sampling import lazy, models
from skrample_amd.sampling import structured as PT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NULL, DTYPE, TERMS, ALIGN, SHAPE, LAUNCH, UNSUPPORTED = range(8)
OFFSETS = {"scale_dev": 0, "x0_out": 8, "a": 16, "b": 24, "sample_numel": 32, "slot": 40, "xslot": 44, "reserved": 48}


def reference_prediction(x, o, a, b, ratio, max_value):
    "the definition in numpy: x0 from three float32 operations, np.quantile of |x0| in float64, the clip and the division in float64"
    x0 = (np.float32(a) * x.astype(np.float32) + np.float32(b) * o.astype(np.float32)).astype(np.float64)
    q = np.quantile(np.abs(x0).reshape(len(x0), -1), ratio, axis=1).astype(np.float32).astype(np.float64)
    s = np.clip(q, 1.0, float(np.float32(max_value))).reshape((-1,) + (1,) * (x0.ndim - 1))
    return np.clip(x0, -s, s) / s


def test_scale_entry_checks_in_their_documented_order():
    lib = _hip.load()
    buf = (ctypes.c_char * 128)()
    good = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    call = lambda sample=good, output=good, dtype=_hip.BF16, ratio=0.995, numel=16, sn=8, scale=good, ws=good: lib.skr_threshold_scale(  # noqa: E731
        sample, output, dtype, 1.0, -1.0, ratio, 1.5, numel, sn, scale, ws, None)
    assert call(sample=None, numel=-1) == NULL and call(ws=None, sn=0) == NULL
    assert call(numel=-8) == SHAPE and call(sn=0) == SHAPE and call(numel=12) == SHAPE
    assert call(numel=0, sample=good + 8, dtype=99, ratio=2.0) == OK  # an empty launch ahead of everything behind it
    assert call(sample=good + 8, dtype=99) == ALIGN and call(scale=good + 2, dtype=99) == ALIGN
    assert call(dtype=_hip.F64, ratio=0.0) == DTYPE and call(dtype=99) == DTYPE
    for ratio in (0.0, -0.5, 1.0001, float("nan"), float("inf")):
        assert call(ratio=ratio) == UNSUPPORTED


def test_step_entry_checks_in_their_documented_order():
    lib = _hip.load()
    buf = (ctypes.c_char * 128)()
    good = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = 2
    plan.dtype_a = plan.dtype_b = plan.out0_dtype = _hip.BF16
    plan.out1_dtype = _hip.NONE
    thr = _hip.StepThresholdC(None, good, 1.0, -1.0, 8, 0, 1, 0)
    ops = (ctypes.c_void_p * 2)(good, good)

    def call(numel=16, out=good, inputs=ops, seeds=None, **changes):
        "one call with fields of the plan, or (named thr_...) of the threshold structure, changed for its duration"
        where = {k: (thr, k[4:]) if k.startswith("thr_") else (plan, k) for k in changes}
        saved = {k: getattr(*where[k]) for k in changes}
        for k, v in changes.items():
            setattr(*where[k], v)
        status = lib.skr_thresholded_step_launch(ctypes.byref(plan), inputs, out, ctypes.byref(thr), seeds, numel, None)
        for k, v in saved.items():
            setattr(*where[k], v)
        return status

    assert lib.skr_thresholded_step_launch(None, ops, good, ctypes.byref(thr), None, 16, None) == NULL
    assert lib.skr_thresholded_step_launch(ctypes.byref(plan), ops, good, None, None, 16, None) == NULL
    assert call(noise_mode=1, zeta0=0.5, n_terms=99) == NULL  # a launch that draws without seeds, ahead of the operand count
    assert call(n_terms=17, numel=-1) == TERMS and call(thr_slot=2, numel=-1) == TERMS and call(thr_xslot=-1) == TERMS and call(thr_xslot=0) == TERMS
    assert call(numel=-1, noise_mode=3) == SHAPE
    assert call(out0_dtype=_hip.NONE, thr_x0_out=None, noise_mode=3) == NULL  # no output at all
    for change in ({"noise_mode": 3}, {"out1_dtype": _hip.BF16}, {"chain": 1.0}, {"zeta1": 1.0}, {"convert_to": 1}, {"thr_reserved": 1}, {"acc_f64": 1}):
        assert call(thr_sample_numel=0, **change) == UNSUPPORTED
    assert call(out0_dtype=_hip.NONE, thr_sample_numel=0) == UNSUPPORTED and call(out0_dtype=_hip.NONE, out=None, n_terms=3, n_group_a=3, thr_sample_numel=0) == UNSUPPORTED
    assert call(thr_sample_numel=0) == SHAPE and call(thr_sample_numel=5) == SHAPE
    assert call(numel=0, inputs=None, out=None) == OK
    assert call(inputs=None) == NULL and call(out=None) == NULL and call(inputs=(ctypes.c_void_p * 2)(good, None)) == NULL
    assert call(out=good + 8) == ALIGN and call(thr_x0_out=good + 8) == ALIGN and call(thr_scale_dev=good + 2) == ALIGN
    assert call(dtype_a=_hip.F64, dtype_b=_hip.F64, out0_dtype=_hip.F64) == UNSUPPORTED
    assert call(dtype_a=99) == DTYPE and call(out0_dtype=_hip.F16) == DTYPE


def test_struct_and_workspace_match_the_header(tmp_path):
    assert {name: getattr(_hip.StepThresholdC, name).offset for name, _ in _hip.StepThresholdC._fields_} == OFFSETS and ctypes.sizeof(_hip.StepThresholdC) == 56
    assert _hip.ABI_VERSION == 15 and {"skr_threshold_scale", "skr_thresholded_step_launch"} <= set(_hip.EXPORTS)
    if shutil.which("gcc") is None:
        pytest.skip("no gcc on this box")
    sizes = [(6144, 2048), (24, 8), (3 * 2056, 2056)]
    checks = "".join(f'_Static_assert(offsetof(skr_step_threshold, {name}) == {off}, "{name}");\n' for name, off in OFFSETS.items())
    checks += "".join(f'_Static_assert(SKR_THRESHOLD_WORKSPACE({n}, {sn}) == {_hip.threshold_workspace(n, sn)}, "workspace");\n' for n, sn in sizes)
    src = tmp_path / "layout.c"
    src.write_text(f'#include <stddef.h>\n#include "{os.path.join(ROOT, "include", "skrample_hip.h")}"\n{checks}_Static_assert(sizeof(skr_step_threshold) == 56, "size");\nint main(void) {{ return 0; }}\n')
    done = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-c", str(src), "-o", str(tmp_path / "layout.o")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_set_thresholding_validates_and_refuses_a_change_mid_run():
    w = PD.SkrampleWrapperScheduler(PT.Euler(), PS.Karras(PS.Scaled()))
    for bad in ((0.0, 1.5), (1.5, 1.5), (float("nan"), 1.5), (True, 1.5), ("0.9", 1.5), (0.9, 0.0), (0.9, float("inf"))):
        with pytest.raises(lazy.SkrampleHipError, match="set_thresholding"):
            w.set_thresholding(*bad)
    w.set_thresholding(0.9, 2.0)
    assert w._thresholding is None  # takes effect from the next set_timesteps
    w.set_timesteps(4)
    assert w._thresholding == (0.9, 2.0)
    x = torch.randn(2, 3, 8, 8)
    w.step(torch.randn_like(x), w.timesteps[0], x)
    with pytest.raises(lazy.SkrampleHipError, match="middle of a run"):
        w.set_thresholding(None)
    w.set_timesteps(4)
    w.set_thresholding(None)
    w.set_timesteps(4)
    assert w._thresholding is None


@pytest.mark.parametrize("sampler", [PT.Euler(), PT.DPM(order=2), PT.UniPC(order=2)], ids=lambda s: type(s).__name__)
def test_host_route_follows_the_float64_loop(sampler):
    "fp32 CPU tensors through the host executor against numpy thresholding and the same wrapper under DataModel on float64 tensors"
    steps, shape, ratio, max_value = 4, (2, 3, 8, 8), 0.9, 1.5
    w = PD.SkrampleWrapperScheduler(sampler, PS.Karras(PS.Scaled()))
    ref = PD.SkrampleWrapperScheduler(sampler, PS.Karras(PS.Scaled()), models.DataModel(), compute_scale=torch.float64)
    w.set_thresholding(ratio, max_value)
    w.set_timesteps(steps), ref.set_timesteps(steps)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(shape, generator=g) * float(w.init_noise_sigma)
    xr = x.double()
    for i, t in enumerate(w.timesteps):
        out = torch.randn(shape, generator=g)
        a, b = w.model.x_weights(PT._ipoint(w.schedule, i / steps))
        p_ref = torch.from_numpy(reference_prediction(xr.float().numpy(), out.numpy(), a, b, ratio, max_value))
        x, p = w.step(out, t, x, return_dict=False)
        xr = ref.step(p_ref, t, xr, return_dict=False)[0]
        # x0 cancels two products: its fp32 form is off by an ulp of the larger one per operation, and p (|p| <= 1, s >= 1) inherits that;
        # the state sums p and the previous state with weights of order one
        bound = 4 * 2.0**-23 * max(1.0, float((a * xr).abs().max()), float((b * out).abs().max()))
        p = p.materialize() if isinstance(p, lazy.LazyTensor) else p
        torch.testing.assert_close(p.double(), p_ref, rtol=0, atol=bound)
        torch.testing.assert_close(x.double(), xr, rtol=2e-6, atol=4 * bound)
