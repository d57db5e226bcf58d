"""Masked steps (in-painting) without a device: the C ABI declaration and its binding, lazy.evaluate_masked through the host executor,
the mask layouts it accepts and refuses, and SkrampleWrapperScheduler.set_inpaint / clear_inpaint on CPU tensors.

The bound every comparison against float64 is held to (per element; derived, not tuned):
    2 (n + 4) u_acc M  +  u_out |ref|  +  tiny_out
n operands (+1 with noise), u_acc = 2^-24 (fp32 accumulation) or 2^-53, M = |m| (sum |coef0_k x_k| + |zeta0 N|) + |1 - m| sum |coef1_k x_k|,
u_out = 2^-8 / 2^-11 / 2^-24 / 2^-53 by output dtype, tiny_out its smallest subnormal.  n + 4 counts one rounding for every coefficient's
conversion, one for every fma and three for the blend; the factor 2 covers the second-order terms.  The host executor multiplies and adds
separately (3 n + 4 roundings); that stays inside 2 (n + 4) for the n <= 4 used here."""

import copy
import os
import pickle
import re

import numpy as np
import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.common import Point
from skrample_amd.sampling import lazy
from skrample_amd.sampling import structured as PT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U_OUT = {torch.bfloat16: 2.0**-8, torch.float16: 2.0**-11, torch.float32: 2.0**-24, torch.float64: 2.0**-53}
TINY = {torch.bfloat16: 2.0**-133, torch.float16: 2.0**-24, torch.float32: 2.0**-149, torch.float64: 2.0**-1074}


def bound(n, magnitude, ref, out_dtype, u_acc=2.0**-24):
    return 2 * (n + 4) * u_acc * magnitude + U_OUT[out_dtype] * np.abs(ref) + TINY[out_dtype]


def f64(t):
    return t.detach().cpu().double().numpy()


def test_header_declares_the_entry_point_and_the_binding_lists_it():
    header = open(os.path.join(ROOT, "include", "skrample_hip.h")).read()
    assert re.search(r"int\s+skr_step_launch_masked\s*\(\s*const\s+skr_step_plan\s*\*", header)
    assert re.search(r"typedef\s+struct\s+skr_step_mask\s*\{", header)
    for field in ("mask", "dtype", "reserved", "mask_numel", "batch_stride"):
        assert re.search(rf"\b{field};", header), field
    assert re.search(r"#define\s+SKR_ABI_VERSION\s+15\b", header) and _hip.ABI_VERSION == 15
    assert "skr_step_launch_masked" in _hip.EXPORTS
    assert [name for name, _ in _hip.StepMaskC._fields_] == ["mask", "dtype", "reserved", "mask_numel", "batch_stride"]
    assert callable(_hip.launch_step_masked)


def test_mask_layouts():
    shape = (3, 4, 6, 8)
    assert lazy.mask_layout((3, 1, 6, 8), shape) == (48, 48)
    assert lazy.mask_layout((1, 1, 6, 8), shape) == (48, 0)
    assert lazy.mask_layout((3, 4, 6, 8), shape) == (192, 192)
    assert lazy.mask_layout((1, 4, 6, 8), shape) == (192, 0)
    assert lazy.mask_layout((6, 8), shape) == (48, 0)
    assert lazy.mask_layout((1, 6, 8), shape) == (48, 0)
    for bad in [(3, 4, 1, 8), (3, 1, 5, 8), (3, 1, 6, 1), (2, 1, 6, 8), (3, 1, 6), (5,), (1, 3, 1, 6, 8), ()]:
        with pytest.raises(lazy.SkrampleHipError):
            lazy.mask_layout(bad, shape)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("mask_shape", [(3, 1, 6, 8), (1, 1, 6, 8), (3, 4, 6, 8), (6, 8)])
def test_evaluate_masked_on_cpu_tensors_stays_within_the_float64_bound(dtype, mask_shape):
    shape = (3, 4, 6, 8)
    g = torch.Generator().manual_seed(7)
    x, o, orig, nz = (torch.randn(shape, generator=g).to(dtype) for _ in range(4))
    mask = torch.rand(mask_shape, generator=g).to(dtype)
    c = {"x": 1.25, "o": -0.75, "orig_s": 0.3, "orig_k": 0.9, "nz": 0.45}
    # `orig` takes part in both forms: one operand with two coefficients
    form = lazy.lift(x) * c["x"] + lazy.lift(o) * c["o"] + lazy.lift(orig) * c["orig_s"]
    known = lazy.lift(orig) * c["orig_k"] + lazy.lift(nz) * c["nz"]
    got = lazy.evaluate_masked(form, known, mask, dtype=dtype)
    assert got.dtype == dtype and tuple(got.shape) == shape
    m = np.broadcast_to(f64(mask).reshape((1,) * (4 - len(mask_shape)) + mask_shape), shape)
    s_terms = [c["x"] * f64(x), c["o"] * f64(o), c["orig_s"] * f64(orig)]
    k_terms = [c["orig_k"] * f64(orig), c["nz"] * f64(nz)]
    ref = m * sum(s_terms) + (1 - m) * sum(k_terms)
    mag = np.abs(m) * sum(np.abs(t) for t in s_terms) + np.abs(1 - m) * sum(np.abs(t) for t in k_terms)
    err = np.abs(f64(got) - ref)
    assert (err <= bound(4, mag, ref, dtype)).all(), float((err / bound(4, mag, ref, dtype)).max())


def test_evaluate_masked_refuses_what_it_does_not_cover():
    shape = (2, 4, 6, 8)
    x, orig = torch.randn(shape), torch.randn(shape)
    for bad in [(2, 4, 1, 8), (2, 1, 5, 8), (3, 1, 6, 8)]:
        with pytest.raises(lazy.SkrampleHipError):
            lazy.evaluate_masked(lazy.lift(x), lazy.lift(orig), torch.ones(bad))
    with pytest.raises(lazy.SkrampleHipError):  # a masked backward is out of scope: said so, not silently dropped
        lazy.evaluate_masked(lazy.lift(x.clone().requires_grad_()), lazy.lift(orig), torch.ones(2, 1, 6, 8))
    with pytest.raises(lazy.SkrampleHipError):
        lazy.evaluate_masked(lazy.lift(x), lazy.lift(torch.randn(2, 4, 6, 4)), torch.ones(6, 8))


SAMPLERS = {"euler": lambda: PT.Euler(), "dpm2": lambda: PT.DPM(order=2)}


@pytest.mark.parametrize("name", sorted(SAMPLERS))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_wrapper_inpaint_equals_the_unfused_lines_in_float64(name, dtype):
    """6 steps on CPU tensors: step() under set_inpaint against step() + add_noise() + the blend lines on a second, never-masked wrapper,
    the blend lines evaluated in float64 on the stored values.  The mask is binary, so the reference is either the step's own result or
    the re-noised original: the bound is applied with n = 2 (the known form's operands) and, where the step's result is kept, M = |ref|
    (the step's own M is no smaller), which asks no less."""
    shape, steps = (2, 4, 8, 8), 6
    make = lambda: PD.SkrampleWrapperScheduler(SAMPLERS[name](), PS.Karras(PS.Scaled()))  # noqa: E731
    masked, plain = make(), make()
    masked.set_timesteps(steps), plain.set_timesteps(steps)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(shape, generator=g).to(dtype)
    orig, nz = torch.randn(shape, generator=g).to(dtype), torch.randn(shape, generator=g).to(dtype)
    mask = torch.rand((2, 1, 8, 8), generator=g) > 0.4
    mask[:, :, 0, :], mask[:, :, 1, :] = True, False
    masked.set_inpaint(mask, orig, nz)
    ts = list(plain.timesteps)
    m = np.broadcast_to(f64(mask), shape)
    xa = xb = x
    for i, t in enumerate(ts):
        out = torch.randn(shape, generator=g).to(dtype)
        got, pred_a = masked.step(out, t, xa, return_dict=False)
        prev, pred_b = plain.step(out, t, xb, return_dict=False)
        if i + 1 < steps:  # scheduler.add_noise(original, noise, next timestep), in float64; after the last step the original itself
            point = Point(*plain.schedule_np[i + 1])
            known = float(point.alpha) * f64(orig) + float(point.sigma) * f64(nz)
            known_mag = abs(float(point.alpha)) * np.abs(f64(orig)) + abs(float(point.sigma)) * np.abs(f64(nz))
        else:
            known, known_mag = f64(orig), np.abs(f64(orig))
        ref = m * f64(prev) + (1 - m) * known
        mag = m * np.abs(f64(prev)) + (1 - m) * known_mag
        err = np.abs(f64(got) - ref)
        assert got.dtype == dtype and (err <= bound(2, mag, ref, dtype)).all(), (i, float(err.max()))
        assert torch.equal(torch.as_tensor(pred_a).float(), torch.as_tensor(pred_b).float())  # pred_original_sample is unchanged
        if i + 1 == steps:
            assert torch.equal(got[~mask.expand(shape)], orig[~mask.expand(shape)])
        xa = xb = got


@pytest.mark.parametrize("name", sorted(SAMPLERS))
def test_clear_inpaint_restores_the_plain_scheduler_bit_for_bit(name):
    shape, steps = (2, 4, 8, 8), 6
    make = lambda: PD.SkrampleWrapperScheduler(SAMPLERS[name](), PS.Karras(PS.Scaled()))  # noqa: E731
    cleared, never = make(), make()
    g = torch.Generator().manual_seed(13)
    x = torch.randn(shape, generator=g)
    outs = [torch.randn(shape, generator=g) for _ in range(steps)]
    cleared.set_inpaint(torch.ones(2, 1, 8, 8, dtype=torch.uint8), torch.randn(shape, generator=g), torch.randn(shape, generator=g))
    cleared.set_timesteps(steps)
    cleared.step(outs[0], cleared.timesteps[0], x)  # one masked step, then the run starts over without a mask
    cleared.clear_inpaint()
    cleared.set_timesteps(steps), never.set_timesteps(steps)
    xa = xb = x
    for i, t in enumerate(list(never.timesteps)):
        xa = cleared.step(outs[i], t, xa, return_dict=False)[0]
        xb = never.step(outs[i], t, xb, return_dict=False)[0]
        assert torch.equal(xa, xb), i


def test_copies_carry_the_inpaint_tensors():
    w = PD.SkrampleWrapperScheduler(PT.Euler(), PS.Scaled())
    g = torch.Generator().manual_seed(17)
    mask, orig, nz = torch.rand(2, 1, 8, 8, generator=g) > 0.5, torch.randn(2, 4, 8, 8, generator=g), torch.randn(2, 4, 8, 8, generator=g)
    w.set_inpaint(mask, orig, nz)
    assert w._inpaint[0].dtype == orig.dtype  # cast once, here
    for clone in (copy.deepcopy(w), pickle.loads(pickle.dumps(w))):
        got = clone._inpaint
        assert got is not None and torch.equal(got[0], mask.float()) and torch.equal(got[1], orig) and torch.equal(got[2], nz)
        clone.set_timesteps(4), w.set_timesteps(4)
        x, out = torch.randn(2, 4, 8, 8, generator=g), torch.randn(2, 4, 8, 8, generator=g)
        assert torch.equal(clone.step(out, clone.timesteps[0], x, return_dict=False)[0], w.step(out, w.timesteps[0], x, return_dict=False)[0])
    assert not hasattr(PD.RKUltraWrapperScheduler, "set_inpaint") and not hasattr(PD.DynasauRKWrapperScheduler, "set_inpaint")
    with pytest.raises(lazy.SkrampleHipError):
        w.set_inpaint(torch.ones(2, 4, 1, 8), orig, nz)
